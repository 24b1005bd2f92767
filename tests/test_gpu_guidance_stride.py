"""Option "guidance_stride" on the MI355X (hparams.sampling.guidance_stride): the HIP chains that compute the guidance update at
every n-th guided step and reuse it in between, against the restated chain of tests/stride_ref.py - the three guiding samplers
at strides 2 and 3, eager = captured, injected and Philox noise, every row of stride_cases.OPTION_CASES, draws - the identities
the option promises (a refresh step leaves the option-off roll, 0 / 1 / unset replay the parent's chain, a replay restarts the
state), the evaluations a reuse step runs, dr_step's state rule, windows with their blends and recording marks, the fused
geometry, the other precisions and sharding.  Inputs and references: tests/stride_cases.py, which
tests/test_guidance_stride_cpu.py shows to reuse.  Tolerance: agree / ATOL of tests/testlib.py; the observed margins are
recorded in profiles/stride_margins.txt.  The scenarios shared with the other guidance options are tests/stage_scenarios.py's;
every test here fails on an engine without the option, whose dr_set_option does not know the name."""
import functools

import pytest
import torch

from oracle import diffroll_ref as R
from testlib import ATOL, S, agree, assert_shared_frames_agree, inputs, make_model, maxdiff

import bf16_ref as Q
import blend_cases as BC
import f16_ref as H
import stage_scenarios as SS
import stride_cases as SC
import stride_ref as SR
from stage_scenarios import one

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

MAIN = SC.values(SC.MAIN)
NOTE = f" (bound {ATOL:.0e})"
NAME = "guidance_stride"


@pytest.fixture(autouse=True)
def integer_values(monkeypatch):
    """The shared scenarios write a stage's values to hparams.sampling as fractions of 10000; this stage's value is the integer."""
    monkeypatch.setattr(SS, "set_values", SC.set_values)


def record(name, d):
    """(the lines profiles/stride_margins.txt is made of)"""
    SS.margin(f"guidance_stride {name}", d, NOTE)


# ---------------------------------------------------------------------------------------------- 1. the chains
@pytest.mark.parametrize("stride", SC.STRIDES)
@pytest.mark.parametrize("sampler", SC.GUIDING)
def test_chain_vs_restatement(sampler, stride):
    hp, p, wav, x, noise = SC.setup()
    m = SC.stride_model(hp, p, sampler, stride)
    for philox, kw in ((False, dict(noise=noise)), (True, dict(seed=SC.PHILOX_SEED))):
        ref = SC.assert_active(sampler, stride, philox=philox)       # (the inputs reuse, before the engine's roll is looked at)
        roll, _ = m.sample(x, wav, **kw)                              # DR_ENAME (-> ValueError) before the option existed
        eager, _ = m.sample(x, wav, use_graph=False, **kw)
        assert torch.equal(roll, eager), maxdiff(roll.cpu(), eager.cpu())
        ok, d = agree(roll, ref)
        record(f"{sampler} w 3 stride {stride} n 20 {'philox' if philox else 'injected'}", d)
        assert ok, d
        assert not agree(roll, SC.reference(sampler, 0, philox=philox)[0])[0]
    assert m.engine.guidance_stride == stride
    assert m.engine.launch_state()["mode"] != "fused_stack+tail"


@pytest.mark.parametrize("name,kw,facade", SC.OPTION_CASES, ids=[c[0] for c in SC.OPTION_CASES])
def test_other_options_vs_restatement(name, kw, facade):
    hp, p, wav, x, noise = SC.setup()
    m = SC.stride_model(hp, p, "cfdg_ddpm_x0", SC.MAIN, **facade)
    ref = SC.assert_active("cfdg_ddpm_x0", SC.MAIN, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, noise=noise, use_graph=False)
    assert torch.equal(roll, eager)
    ok, d = agree(roll, ref)
    record(f"with {name}, w 3 stride {SC.MAIN}", d)
    assert ok, d
    assert not agree(roll, SC.reference("cfdg_ddpm_x0", 0, **kw)[0])[0]


def test_draws_vs_restatement():
    """Two draws of the two clips in one chain: one state per draw, the roll of the batch with the clips tiled."""
    hp, p, _, _, _ = SC.setup()
    wav, x, noise = inputs(2 * SC.B, SC.TN, 101)
    wav = wav[:SC.B]
    m = SC.stride_model(hp, p, "cfdg_ddpm_x0", SC.MAIN)
    got, _ = m.sample(x, wav, draws=2, noise=noise)
    tiled, _ = m.sample(x, wav.repeat(2, 1), noise=noise)
    assert torch.equal(got, tiled) and not torch.equal(got[0], got[SC.B])
    spec = R.frontend(wav.repeat(2, 1), hp, SC.TN)
    ref, sched = SR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, SC.N_STEPS, w=SC.W, guidance_stride=SC.MAIN)
    off, _ = SR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, SC.N_STEPS, w=SC.W)
    assert [what for _, what in sched].count("reuse") == 9 and float((ref - off).abs().max()) >= 100 * ATOL
    ok, d = agree(got, ref)
    record(f"with draws 2, w 3 stride {SC.MAIN} n 20", d)
    assert ok, d
    got_p, _ = m.sample(x, wav, draws=2, seed=5, first_sample=3)
    assert torch.equal(got_p, m.sample(x, wav.repeat(2, 1), seed=5, first_sample=3)[0])


# ---------------------------------------------------------------------------------------------- 2. identities
def test_a_refresh_step_leaves_the_option_off_roll():
    """dr_step over the visited steps (sample_trajectory): the row behind the chain's first guided step - a refresh - holds the
    bits of the option-off chain, the row behind the first reuse parts from it; under the interval [60, 140] every row up to and
    including the first refresh does, and the whole matches the restatement."""
    hp, p, wav, x, noise = SC.setup()
    m = SC.stride_model(hp, p, "cfdg_ddpm_x0", SC.MAIN)
    on, _ = m.sample_trajectory(x, wav, noise=noise)
    whole, _ = m.sample(x, wav, noise=noise)
    assert torch.equal(whole, on[-1])                 # the dr_step sequence is dr_sample's chain
    m.hparams.sampling.guidance_stride = None
    off, _ = m.sample_trajectory(x, wav, noise=noise)
    assert torch.equal(on[0], off[0]) and not torch.equal(on[1], off[1])
    ref, sched = SR.sample_chain(p, hp, "cfdg_ddpm_x0", x, SC.spec_of("cfdg_ddpm_x0"), noise, SC.N_STEPS, w=SC.W, guidance_stride=SC.MAIN,
                                 trajectory=True)
    assert sched[0][1] == "refresh" and sched[1][1] == "reuse"
    d = max(maxdiff(on[i].cpu(), ref[i]) for i in range(len(sched)))
    record(f"dr_step trajectory, every row, stride {SC.MAIN}", d)
    assert d <= ATOL, d
    _, whole, on, off, first = SS.steps_outside_the_interval(MAIN, (NAME,))
    assert torch.equal(on[first], off[first]) and not torch.equal(on[first + 1], off[first + 1])
    ok, d = agree(whole, SC.reference("cfdg_ddpm_x0", SC.MAIN, philox=True, interval=(60, 140))[0])
    record("interval [60, 140], Philox, dr_step sequence", d)
    assert ok, d


def test_stride_0_and_1_are_the_parents_chain_and_the_value_is_in_the_key():
    """A 4-step chain captured with the option unset; set to 2 and back it replays, no launch counted; under 2 another chain is
    captured (stage_scenarios.captured_under).  Then 1 and 0 are one key: the chain captured under 1 is the one 0 replays, and
    both hold the bits of the chain captured before the option was ever set."""
    with SS.captured_under(NAME, 0, 2, (NAME,)) as (eng, run, first, c2):
        assert torch.equal(run(), run())              # (the state restarts itself: 3. below)
        eng.set_option(NAME, 1)
        at_1, c1 = run(), eng.launch_counts()
        assert torch.equal(at_1, first) and c1 != c2  # (one chain is held: the parent's is captured again, the same bits)
        eng.set_option(NAME, 0)
        assert torch.equal(run(), first) and eng.launch_counts() == c1      # 0 replays what 1 captured
        eng.set_option(NAME, 1)
        assert torch.equal(run(), first) and eng.launch_counts() == c1
        assert torch.equal(run_eager(eng), first)


def run_eager(eng):
    _, x_T = chain_inputs(eng)
    return eng.sample("cfdg_ddpm_x0", x_T, None, w=SC.W, seed=SC.PHILOX_SEED, use_graph=False)


def chain_inputs(eng):
    _, _, _, x, _ = SC.setup()
    return eng, x.squeeze(1).to(eng.device).contiguous().clone()


@pytest.mark.parametrize("sampler,w", [("cfdg_ddpm_x0", 0.0), ("cfdg_ddim_x0", 0.0)])
def test_a_chain_at_weight_0_is_untouched(sampler, w):
    SS.unguided_chain_is_untouched(sampler, w, MAIN)


def test_replaying_the_captured_chain_restarts_the_state():
    """The captured chain launched twice on the state its first launch left, then after another chain (stride 3) wrote the state:
    the same bits each time, no launch counted - the chain's first guided step is a refresh baked into its node."""
    eng, x_T = SS.chain_engine(steps=8)

    def run(**kw):
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=SC.W, seed=SC.PHILOX_SEED, **kw)

    try:
        plain = run()
        eng.set_option(NAME, 2)
        first, c0 = run(), eng.launch_counts()
        assert not torch.equal(first, plain)
        assert torch.equal(run(), first) and torch.equal(run(), first) and eng.launch_counts() == c0
        assert torch.equal(run(use_graph=False), first)
        eng.set_option(NAME, 3)
        other = run()
        assert not torch.equal(other, first) and not torch.equal(other, plain) and torch.equal(run(use_graph=False), other)
        eng.set_option(NAME, 2)
        assert torch.equal(run(), first)
    finally:
        eng.set_option(NAME, 0)


# ---------------------------------------------------------------------------------------------- 3. evaluations
def test_a_reuse_step_runs_B_evaluations():
    """The fused geometry, eager, 20 guided steps at stride 2.  A 2 B evaluation of guided pairs contracts layer 0's conv once per
    pair in a launch of its own in front of the fused stack (dr_debug_launch_counts: counted where no tail kernel primed it); a
    B evaluation has none.  The chain counts 11 of them - its 11 refresh steps - and 20 input projections: the 9 reuse steps ran
    the conditional evaluation alone, as the steps outside a guidance interval do (tests/test_gpu_guidance_interval.py).  At
    stride 4: 6; with cfg_rescale in the option's place - every guided step beside the tail kernel, both evaluations - 20."""
    with SS.fused_geometry(MAIN) as (hp, p, m, wav, x):
        eng = m.engine

        def counts():
            c0, s0 = eng.launch_counts(), eng.launch_state()
            roll, _ = m.sample(x, wav, seed=5, use_graph=False)
            c1, s1 = eng.launch_counts(), eng.launch_state()
            assert s1["tail_launches"] == s0["tail_launches"] and s1["mode"] == "fused_stack", s1
            return (c1[0] - c0[0], c1[1] - c0[1], s1["stack_launches"] - s0["stack_launches"]), roll

        sched = SR.schedule(m.visited_steps(), 2, S)
        assert [what for _, what in sched].count("refresh") == 11
        assert counts()[0] == (20, 11, 20)
        m.hparams.sampling.guidance_stride = 4
        assert counts()[0] == (20, 6, 20)
        m.hparams.sampling.guidance_stride = None
        m.hparams.sampling.cfg_rescale = 0.7
        assert counts()[0] == (20, 20, 20)
        m.hparams.sampling.cfg_rescale = None


# ---------------------------------------------------------------------------------------------- 4. dr_step and the values
def test_values_and_refusals():
    """dr_set_option accepts 0, 1, 2 and 64 and refuses -1 and 65, stating the range; beside each forbidden partner dr_step and
    dr_sample answer DR_EINVAL naming the two options; a sampler that does not guide refuses a set value."""
    eng, xb = SS.chain_engine(steps=20)
    for ok in (0, 1, 2, 64):
        eng.set_option(NAME, ok)
        assert eng.guidance_stride == ok
    for bad in (-1, 65, 1000):
        with pytest.raises(ValueError, match=f"guidance_stride.*2 .. 64.*{bad}"):
            eng.set_option(NAME, bad)
    assert eng.guidance_stride == 64
    eng.set_option(NAME, 2)
    v = eng.visited_steps()
    partners = (("cfg_rescale", 7000, ()), ("cfg_project", 10000, ()), ("cfg_norm", 500, ()), ("cfg_momentum", -5000, ("cfg_project",)),
                ("x0_threshold", 9950, ("x0_clip",)))
    try:
        for name, value, needs in partners:
            for other in needs:
                eng.set_option(other, 1 if other == "x0_clip" else 10000)
            eng.set_option(name, value)
            named = "cfg_project = 10000" if name == "cfg_momentum" else f"{name} = {value}"      # (the first partner that is set)
            for call in (lambda: eng.step("cfdg_ddpm_x0", xb.clone(), None, v[0], w=SC.W),
                         lambda: eng.sample("cfdg_ddpm_x0", xb.clone(), None, w=SC.W, seed=1)):
                with pytest.raises(ValueError, match=f"guidance_stride = 2 does not combine with {named}"):
                    call()
            for other in (name,) + needs:
                eng.set_option(other, 0)
        for sampler in ("ddpm_x0", "ddim"):
            with pytest.raises(ValueError, match="does not guide: guidance_stride = 2"):
                eng.sample(sampler, xb.clone(), None, seed=1)
        eng.set_option(NAME, 1)                       # 1 is off: nothing is refused
        eng.set_option("cfg_rescale", 7000)
        eng.sample("cfdg_ddpm_x0", xb.clone(), None, w=SC.W, seed=1)
        eng.sample("ddpm_x0", xb.clone(), None, seed=1)
    finally:
        for name in (NAME, "cfg_rescale", "cfg_momentum", "cfg_project", "cfg_norm", "x0_threshold", "x0_clip"):
            eng.set_option(name, 0)
    eng.finish()


def test_dr_step_state_rule():
    from diffroll_amd.engine import EngineError
    eng, xb = SS.chain_engine(steps=20)
    v = eng.visited_steps()

    def step(t, x=None, w=SC.W):
        eng.step("cfdg_ddpm_x0", xb if x is None else x, None, t, w=w, seed=SC.PHILOX_SEED)

    eng.set_option(NAME, 2)
    try:
        whole = eng.sample("cfdg_ddpm_x0", xb.clone(), None, w=SC.W, seed=SC.PHILOX_SEED)
        x = xb.clone()
        with pytest.raises(EngineError, match=f"step {v[1]} reuses no stored guidance update - the step expected next is {v[0]}"):
            step(v[1], x)                             # a reuse without its refresh: dr_sample ended whatever was held
        for t in v:
            step(t, x)
        assert torch.equal(x, whole)                  # the sequence in order is accepted and equals the chain
        step(v[0])
        step(v[2])                                    # a refresh needs nothing, whatever came before
        with pytest.raises(EngineError, match=f"step {v[5]} reuses no stored guidance update - the step expected next is {v[3]}"):
            step(v[5])
        step(v[3])                                    # (a refusal changes nothing)
        step(v[4])
        step(v[5])
        eng.set_option(NAME, 4)                       # a change of the value between steps ends the state
        with pytest.raises(EngineError, match=f"the step expected next is {v[0]}"):
            step(v[6])                                # (ordinal 6 of stride 4: a reuse)
        step(v[4])                                    # (ordinal 4: a refresh)
        step(v[5])
        eng.set_option(NAME, 4)                       # the same value: nothing ends
        step(v[6])
        eng.set_option("x0_clip", 1)                  # an option change that ends a solver history ends the state
        with pytest.raises(EngineError, match="reuses no stored guidance update"):
            step(v[7])
        eng.set_option("x0_clip", 0)
        step(v[4])
        step(v[5], w=0.0)                             # a step at w = 0 does not guide: it neither reads nor ends the state
        step(v[5])
        # a refusal by this rule leaves the solver history alone, and the other way round
        eng.set_option(NAME, 2)
        eng.set_option("solver_order", 2)
        step(v[0])
        with pytest.raises(EngineError, match="continues no history"):
            step(v[2])                                # (a refresh: refused by the history's rule alone)
        step(v[1])
        step(v[2])
    finally:
        for name in ("solver_order", "x0_clip", NAME):
            eng.set_option(name, 0)
    eng.finish()


# ---------------------------------------------------------------------------------------------- 5. windows
def run_windows(m, batch, wavs, x_T, noise, mode, use_graph=True):
    return m._sample_windows(batch, wavs, x_T, noise, 1, 0, 0, use_graph, True, blend=mode).cpu()


def window_chain(recs, O, mode, stride, marks=()):
    """The restated chain over the windows of the recordings `recs` (blend_cases.recording tuples) in one batch."""
    hp, p = recs[0][0], recs[0][1]
    x = torch.cat([BC.windows_of(r[4].reshape(r[2].T_c, 88), r[2]) for r in recs], 0)
    z = torch.cat([BC.windows_of(r[5].reshape(-1, r[2].T_c, 88), r[2]) for r in recs], 1)
    spec = torch.cat([r[6] for r in recs], 0)
    return SR.sample_chain(p, hp, BC.SAMPLER, x, spec, z, 0, w=SC.W, O=O, mode=mode, marks=marks, guidance_stride=stride)[0][:, 0]


@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "linear"])
@pytest.mark.parametrize("O", BC.OS)
def test_windows_match_and_shared_frames_are_bit_identical(O, mode):
    """Three 32-frame windows of one recording sharing O frames, 4 steps at stride 2 (t = 2 reuses), under the mean and the
    linear cross-fade; then two recordings of 2 + 1 windows in one chain ("window_break")."""
    rec = BC.case(O)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, off = window_chain([rec], O, mode, SC.MAIN), window_chain([rec], O, mode, 0)
    assert maxdiff(ref, off) > 100 * ATOL             # (the case reuses)
    m = SC.stride_model(hp, p, BC.SAMPLER, SC.MAIN, n=0)
    got = run_windows(m, one(plan), [wav], [x_T], [noise], mode)
    assert_shared_frames_agree(got, plan)
    d = maxdiff(got, ref)
    record(f"windows O {O} blend {mode} w 3 stride {SC.MAIN}", d)
    assert d <= ATOL, d
    assert torch.equal(run_windows(m, one(plan), [wav], [x_T], [noise], mode, use_graph=False), got)
    a, b = BC.recording(O, 3400 + O, n=2), BC.recording(O, 3450 + O, n=1)
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = SC.stride_model(a[0], a[1], BC.SAMPLER, SC.MAIN, n=0)
    got = run_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]], mode)
    d = maxdiff(got, window_chain([a, b], O, mode, SC.MAIN, marks=(2,)))
    record(f"window_break O {O} blend {mode} w 3 stride {SC.MAIN}", d)
    assert d <= ATOL, d
    H = a[2].stride
    assert torch.equal(got[0, H:], got[1, :O]) and not torch.equal(got[1, H:], got[2, :O])
    assert torch.equal(got[:2], run_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]], mode))      # each recording equals its own chain


# ---------------------------------------------------------------------------------------------- 6. the fused geometry
def test_fused_geometry_guided_steps_report_fused_stack_and_unguided_ones_come_back():
    with SS.fused_geometry(MAIN) as (hp, p, m, wav, x):
        off = SS.fused_chain_with_the_options_off(m, wav, x, MAIN)
        g = SS.fused_guided_steps_leave_the_tail_kernel(m, wav, x)
        assert not torch.equal(off, g)
    _, sched = SS.fused_roll_vs_restatement(SR.sample_chain, MAIN, hp, p, wav, x, g, f"guidance_stride fused geometry w 3 stride {SC.MAIN} n 20", NOTE)
    assert [what for _, what in sched].count("reuse") == 9


# ---------------------------------------------------------------------------------------------- 7. the other precisions
def test_split_bf16_vs_restatement():
    _, sched = SS.split_bf16_vs_restatement(SR.sample_chain, MAIN, f"guidance_stride bf16x3 w 3 stride {SC.MAIN} n 8", NOTE)
    assert [what for _, what in sched].count("reuse") == 3


def test_bf16_chain_lies_in_the_restatements_band():
    """stage_scenarios.bf16_chain_lies_in_the_restatements_band under the stride, as in test_gpu_cfg_project.py."""
    (_, sched), _ = SS.bf16_chain_lies_in_the_restatements_band(SR.sample_chain, MAIN, "guidance_stride")
    assert [what for _, what in sched].count("reuse") == 3


def test_f16_chain_lies_in_the_restatements_band():
    """The same chain and band under precision "f16": bf16_ref's restated block with f16_ref's rounding (tests/test_gpu_f16.py)."""
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    chain = functools.partial(SR.sample_chain, p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, w=0.5, guidance_stride=SC.MAIN)
    ref = chain()[0]
    with Q.patched(H.rne, None):
        d_ref = Q.rms(chain()[0] - ref)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="f16")
    m.hparams.sampling.guidance_stride = SC.MAIN
    got = m.sample(x, wav, noise=nz)[0]
    d = Q.rms(got.cpu() - ref)
    print(f"\nguidance_stride f16 chain: rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (d, d_ref)
    assert torch.equal(m.sample(x, wav, noise=nz)[0], got)
    assert torch.equal(m.sample(x, wav, noise=nz, use_graph=False)[0], got)
    assert m.engine.guidance_stride == SC.MAIN


# ---------------------------------------------------------------------------------------------- 8. sharding
@pytest.mark.parametrize("G", [2, 3])
def test_sharded_equals_unsharded(G):
    """sample_sharded emulated for G ranks on one device: every rank's engine gets the stride from the model it is handed and
    holds the state of its rows; the gathered rolls are the one-rank chain's."""
    from diffroll_amd.distributed import sample_sharded_sequential
    hp, p, _, _, _ = SC.setup()
    wav, x, noise = inputs(3, SC.TN, 102)
    m = SC.stride_model(hp, p, "cfdg_ddpm_x0", SC.MAIN)
    for kw in (dict(noise=noise), dict(seed=6)):
        whole, _ = m.sample(x, wav, **kw)
        parts = sample_sharded_sequential(m, x, wav, kw.get("noise"), seed=kw.get("seed", 0), world_size=G)
        assert torch.equal(parts, whole)
    m.hparams.sampling.guidance_stride = None
    assert not torch.equal(m.sample(x, wav, seed=6)[0], whole)
