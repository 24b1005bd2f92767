"""Option "cfg_momentum" on the MI355X (hparams.sampling.cfg_momentum): the statistics launch in its momentum form and the state
it leaves, bit for bit against the CPU restatement of tests/momentum_ref.py (dr_debug_momentum: every shape class, both launch
forms, with and without a state, zero / inf / NaN inputs and states, window canvases; twice), then the HIP chains against the
restated chain - the three guiding samplers, every row of project_cases.OPTION_CASES, eager = captured and the captured chain
launched twice (the baked start) - the identities of the option at 0 and of steps that do not guide, dr_step's state rule,
windows and draws, the fused geometry and the two bf16 precisions.  Inputs and references: tests/momentum_cases.py, which
tests/test_cfg_momentum_cpu.py shows to carry momentum.  Tolerance: agree / ATOL of tests/test_gpu_respaced.py; the observed
margins are recorded in profiles/momentum_margins.txt."""
import numpy as np
import pytest
import torch

from test_gpu_cfg_project import one, project_model, run_windows, unconditional
from test_gpu_parity import make_model, maxdiff
from test_gpu_respaced import ATOL, S, agree
from test_gpu_x0_threshold import kernel_inputs, same_bits

import blend_cases as BC
import momentum_cases as MC
import momentum_ref as MR
import thresh_ref as TR

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

# (cfg_momentum, cfg_project, cfg_norm) of the kernel tests
TRIPLES = ((-5000, 10000, 500), (5000, 10000, 500), (-5000, 10000, 0), (5000, 10000, 0))


def momentum_model(hp, p, sampler, momentum, project, norm, **kw):
    """test_gpu_cfg_project.project_model with hparams.sampling.cfg_momentum = the value / 10000."""
    m = project_model(hp, p, sampler, project, norm, **kw)
    m.hparams.sampling.cfg_momentum = momentum / 10000.0 if momentum else None
    return m


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    """A committed engine whose options the kernel tests set; handed back with every one of them off."""
    hp, p, _, _, _ = MC.setup()
    eng = make_model(hp, p, sampler="cfdg_ddpm_x0").engine
    yield eng
    for name, value in (("window_overlap", 0), ("window_blend", 0), ("window_break", 0), ("draws", 1), ("cfg_momentum", 0), ("cfg_project", 0),
                        ("cfg_norm", 0)):
        eng.set_option(name, value)


def check_kernel(lab, c, u, states, groups, plan=None, note=()):
    """The launch on (c, u) at w = 3 under every triple of TRIPLES and every state of `states` (None: the step starts the state),
    twice; (a, b) and the state it leaves against the restatement, bit for bit.  Returns {(triple, state index): (ab, m)}."""
    want = {}
    try:
        for momentum, project, norm in TRIPLES:
            lab.set_option("cfg_project", project)
            lab.set_option("cfg_norm", norm)
            lab.set_option("cfg_momentum", momentum)      # DR_ENAME (-> ValueError) before the option existed
            for i, m_prev in enumerate(states):
                ab, m = MR.group_ab(c, u, 3.0, m_prev, momentum, project, norm, groups, plan)
                want[(momentum, project, norm), i] = (ab, m)
                got, state = lab.momentum_stats(c, u, m_prev, 3.0, groups=len(groups))
                again, state2 = lab.momentum_stats(c, u, m_prev, 3.0, groups=len(groups))
                ref = torch.from_numpy(ab)
                where = (note, momentum, project, norm, i)
                assert got.shape == ref.shape
                assert same_bits(got, ref), (where, got.cpu().tolist()[:4], ref.tolist()[:4])
                assert same_bits(state, m.reshape(state.shape)), (where, maxdiff(state.cpu(), m.reshape(state.shape)))
                assert same_bits(again, got) and same_bits(state2, state), where
    finally:
        for name in ("cfg_momentum", "cfg_project", "cfg_norm"):
            lab.set_option(name, 0)
    return want


def states_of(B, T, seed):
    """No state, and a random one of the size of the update c - u at w = 3."""
    return (None, 3.0 * torch.randn(B, T, 88, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize("B,T", [(1, 1), (3, 3), (2, 40), (2, 130)])
def test_statistics_and_state_are_bit_equal_to_the_restatement(lab, B, T):
    """(2, 130): three blocks, the last one partial."""
    moved = 0
    inputs = dict(kernel_inputs(B, T, 17 + T), zero=torch.zeros(B, T, 88))
    for name, c in inputs.items():
        u = unconditional(name, B, T)
        want = check_kernel(lab, c, u, states_of(B, T, 31 + T), TR.clip_groups(B), note=name)
        for (triple, i), (ab, m) in want.items():
            if name in ("only_nan", "specials"):
                assert tuple(ab[0]) == (0.0, 1.0), (name, triple, i)      # a non-finite group: exactly the identity
            if name == "one_nan":
                assert tuple(ab[B - 1]) == (0.0, 1.0) and torch.isnan(m).sum() == 1
            moved += int((ab[:, 0] != np.float32(0.0)).sum())
    assert moved > 0                                  # (some of these groups project)


def test_special_states(lab):
    """All-zero, inf and NaN states beside ordinary predictions: a zero state is the starting step's m (+-0 aside), a non-finite
    element stays non-finite and its roll gets the identity pair, the other roll is untouched by it."""
    B, T = 2, 40
    g = torch.Generator().manual_seed(77)
    c, u = 1.2 * torch.randn(B, T, 88, generator=g) + 0.5, torch.randn(B, T, 88, generator=g)
    base = 3.0 * torch.randn(B, T, 88, generator=g)
    inf, nan = base.clone(), base.clone()
    inf[1, 7, 3], inf[1, 8, 4] = float("inf"), float("-inf")
    nan[1, 39, 87] = float("nan")
    want = check_kernel(lab, c, u, (None, torch.zeros(B, T, 88), inf, nan, base), TR.clip_groups(B))
    for triple in TRIPLES:
        start, zero, w_inf, w_nan, plain = (want[triple, i] for i in range(5))
        assert torch.equal(zero[1], start[1]) and np.array_equal(zero[0], start[0])
        for ab, m in (w_inf, w_nan):
            assert tuple(ab[1]) == (0.0, 1.0) and tuple(ab[0]) == tuple(plain[0][0]) and not torch.isfinite(m[1]).all()
            assert torch.equal(m[0], plain[1][0])
        assert not np.array_equal(plain[0], start[0])


@pytest.mark.parametrize("T", [744, 745])
def test_either_side_of_the_form_switch(lab, T):
    """T * 88 = 65472 / 65560 elements: the last roll of the one-workgroup form and the first of the grid form."""
    g = torch.Generator().manual_seed(T)
    c, u = 1.2 * torch.randn(2, T, 88, generator=g) + 0.5, torch.randn(2, T, 88, generator=g)
    want = check_kernel(lab, c, u, states_of(2, T, T + 1), TR.clip_groups(2))
    assert all((np.abs(ab[:, 0]) > 0.05).all() for ab, _ in want.values())


@pytest.mark.parametrize("marks,draws", [((), 1), ((2,), 1), ((2,), 2)], ids=["one-recording", "mark-at-2", "mark-at-2-draws-2"])
@pytest.mark.parametrize("O", [1, 5, 16])
def test_window_canvases(lab, O, marks, draws):
    """32-frame windows, three per draw, under the three blend modes: one pair per recording over the blended predictions, and
    the state a step leaves is the same on the frames two windows share - given a state that is (what the update leaves)."""
    T, B = 32, 3 * draws
    groups = TR.window_groups(B, O, marks, draws)
    g = torch.Generator().manual_seed(5 + B + len(marks) + O)
    c = kernel_inputs(B, T, 23)["noise"] + 0.5
    u = torch.randn(B, T, 88, generator=g)
    shared = [(rows[j][0], rows[j + 1][0]) for rows in groups for j in range(len(rows) - 1)]      # (lower, upper) rows of a group
    assert shared
    prev = 3.0 * torch.randn(B, T, 88, generator=g)
    for lo, up in shared:
        prev[up, :O] = prev[lo, T - O:]
    try:
        lab.set_option("window_overlap", O)
        lab.set_window_breaks(marks)
        lab.set_option("draws", draws)
        for mode in (0, 1, 2):
            lab.set_option("window_blend", mode)
            want = check_kernel(lab, c, u, (None, prev), groups, plan=(O, mode), note=("windows", mode))
            for ab, m in want.values():
                assert ab.shape == (len(groups), 2) and (np.abs(ab[:, 0]) > 0.05).all()
                for lo, up in shared:
                    assert torch.equal(m[up, :O], m[lo, T - O:])
    finally:
        lab.set_option("draws", 1)
        lab.set_window_breaks(())
        lab.set_option("window_blend", 0)
        lab.set_option("window_overlap", 0)


# ---------------------------------------------------------------------------------------------- 2. the chains
def record(name, d):
    """(the lines profiles/momentum_margins.txt is made of)"""
    print(f"\ncfg_momentum {name}: max |d| {d:.3e} (bound {ATOL:.0e})")


@pytest.mark.parametrize("values", MC.VALUES, ids=[str(v[0]) for v in MC.VALUES])
@pytest.mark.parametrize("sampler", MC.GUIDING)
def test_chain_vs_restatement(sampler, values):
    hp, p, wav, x, noise = MC.setup()
    m = momentum_model(hp, p, sampler, *values)
    ref = MC.assert_active(sampler, *values)          # (the inputs carry momentum, before the engine's roll is looked at)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, use_graph=False, noise=noise)
    assert torch.equal(roll, eager), maxdiff(roll.cpu(), eager.cpu())
    ok, d = agree(roll, ref)
    record(f"{sampler} w 3 values {values} n 20", d)
    assert ok, d
    assert not agree(roll, MC.reference(sampler, 0, *values[1:])[0])[0]
    assert m.engine.cfg_momentum == values[0]
    assert m.engine.launch_state()["mode"] != "fused_stack+tail"


@pytest.mark.parametrize("values", MC.VALUES, ids=[str(v[0]) for v in MC.VALUES])
@pytest.mark.parametrize("name,kw,facade", MC.OPTION_CASES, ids=[c[0] for c in MC.OPTION_CASES])
def test_other_options_vs_restatement(name, kw, facade, values):
    hp, p, wav, x, noise = MC.setup()
    m = momentum_model(hp, p, "cfdg_ddpm_x0", *values, **facade)
    ref = MC.assert_active("cfdg_ddpm_x0", *values, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, noise=noise, use_graph=False)
    assert torch.equal(roll, eager)
    ok, d = agree(roll, ref)
    record(f"with {name}, w 3 values {values} n 20", d)
    assert ok, d


# ---------------------------------------------------------------------------------------------- 3. the captured chain
def _engine(steps=4, sampler="cfdg_ddpm_x0", w=MC.W):
    hp, p, wav, x, _ = MC.setup()
    m = make_model(hp, p, sampler=sampler, w=w)
    m.hparams.sampling.steps = steps
    eng = m.engine
    eng.frontend(wav, MC.TN)
    return eng, x.squeeze(1).to(eng.device).contiguous()


def test_a_captured_chain_restarts_its_state_at_every_launch_and_the_value_is_in_its_key():
    eng, x_T = _engine()

    def run(**kw):
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=MC.W, seed=MC.PHILOX_SEED, **kw)

    eng.set_option("cfg_project", 10000)
    eng.set_option("cfg_norm", 500)
    try:
        plain, cp = run(), eng.launch_counts()
        eng.set_option("cfg_momentum", -5000)
        first, c0 = run(), eng.launch_counts()
        assert c0 != cp and not torch.equal(first, plain)
        second = run()                                # the same captured chain on the state the first launch left: the baked start
        assert torch.equal(second, first) and eng.launch_counts() == c0
        assert torch.equal(run(use_graph=False), first)
        eng.set_option("cfg_momentum", -7500)
        other, c1 = run(), eng.launch_counts()
        assert c1 != c0 and not torch.equal(other, first)
        eng.set_option("cfg_momentum", -5000)
        back, c2 = run(), eng.launch_counts()
        assert torch.equal(back, first)
        eng.set_option("cfg_momentum", -7500)
        eng.set_option("cfg_momentum", -5000)         # back at the old value the old chain replays, no launch counted
        assert torch.equal(run(), first) and eng.launch_counts() == c2
    finally:
        for name in ("cfg_momentum", "cfg_project", "cfg_norm"):
            eng.set_option(name, 0)


# ---------------------------------------------------------------------------------------------- 4. the parent's chain
def test_value_0_is_the_parents_projected_chain_bitwise_and_replays_it():
    eng, x_T = _engine()

    def run():
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=MC.W, seed=MC.PHILOX_SEED)

    eng.set_option("cfg_project", 10000)
    eng.set_option("cfg_norm", 500)
    try:
        parent, c0 = run(), eng.launch_counts()
        eng.set_option("cfg_momentum", -5000)
        eng.set_option("cfg_momentum", 0)
        assert torch.equal(run(), parent) and eng.launch_counts() == c0      # back at 0 the parent's chain replays, no launch counted
        eng.set_option("cfg_momentum", -5000)
        on = run()
        eng.set_option("cfg_momentum", 0)
        off = run()                                   # (one chain is held: the parent's is captured again, the same bits)
        assert torch.equal(off, parent) and not torch.equal(on, parent)
    finally:
        for name in ("cfg_momentum", "cfg_project", "cfg_norm"):
            eng.set_option(name, 0)
    hp, p, wav, x, noise = MC.setup()
    m = momentum_model(hp, p, "cfdg_ddpm_x0", 0, 10000, 500)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, MC.PC.reference("cfdg_ddpm_x0", 10000, 500)[0])
    assert ok, d


@pytest.mark.parametrize("sampler,w", [("ddpm_x0", 0.0), ("ddim", 0.0), ("cfdg_ddpm_x0", 0.0)])
def test_a_chain_that_does_not_guide_is_untouched(sampler, w):
    eng, x_T = _engine(sampler=sampler, w=w)

    def run(**kw):
        t0 = eng.tail_launches
        return eng.sample(sampler, x_T.clone(), None, w=w, seed=MC.PHILOX_SEED, **kw), eng.tail_launches - t0

    (first, tails), c0 = run(), eng.launch_counts()
    eng.set_option("cfg_project", 10000)
    eng.set_option("cfg_momentum", -5000)
    try:
        (again, tails_on), c1 = run(), eng.launch_counts()
        eager, _ = run(use_graph=False)
    finally:
        eng.set_option("cfg_momentum", 0)
        eng.set_option("cfg_project", 0)
    assert torch.equal(again, first) and torch.equal(eager, first)
    assert tails_on == tails and c1 == c0, (c0, c1)


def test_steps_outside_the_interval_keep_every_bit_and_the_state_starts_inside():
    """dr_step over the visited steps under the interval [60, 140]: the rolls behind the steps above 140 hold the same bits with
    the option on and off; the first step <= 140 starts the state (there m = d: the roll equals the projected chain's), the
    second one parts the two; the whole matches the restatement."""
    hp, p, wav, x, _ = MC.setup()
    m = momentum_model(hp, p, "cfdg_ddpm_x0", *MC.MAIN, guidance_interval=[60, 140])
    kw = dict(seed=MC.PHILOX_SEED)
    on, _ = m.sample_trajectory(x, wav, **kw)
    whole, _ = m.sample(x, wav, **kw)
    assert torch.equal(whole, on[-1])                 # the dr_step sequence equals dr_sample
    m.hparams.sampling.cfg_momentum = None
    off, _ = m.sample_trajectory(x, wav, **kw)
    visited = m.visited_steps()
    above = [i for i, t in enumerate(visited) if t > 140]
    first = above[-1] + 1
    assert 60 <= visited[first] <= 140
    for i in above:
        assert torch.equal(on[i], off[i]), visited[i]
    assert not torch.equal(on[first + 1], off[first + 1])
    ref = MC.reference("cfdg_ddpm_x0", *MC.MAIN, philox=True, interval=(60, 140))[0]
    ok, d = agree(whole, ref)
    record("interval [60, 140], Philox, dr_step sequence", d)
    assert ok, d


# ---------------------------------------------------------------------------------------------- 5. dr_step
def test_dr_step_state_rule():
    from diffroll_amd.engine import EngineError
    eng, xb = _engine(steps=20)
    v = eng.visited_steps()

    def step(t, x=None):
        eng.step("cfdg_ddpm_x0", xb if x is None else x, None, t, w=MC.W, seed=MC.PHILOX_SEED)

    for bad in (-10000, 10000, 70000):
        with pytest.raises(ValueError, match=f"cfg_momentum.*-9999 .. 9999.*{bad}"):
            eng.set_option("cfg_momentum", bad)
    eng.set_option("cfg_momentum", -5000)
    try:
        with pytest.raises(ValueError, match="cfg_momentum = -5000.*cfg_project = 0.*cfg_norm = 0"):      # both partners 0: DR_EINVAL at the call
            step(v[0])
        with pytest.raises(ValueError, match="cfg_momentum = -5000.*cfg_project = 0.*cfg_norm = 0"):
            eng.sample("cfdg_ddpm_x0", xb.clone(), None, w=MC.W, seed=MC.PHILOX_SEED)
        eng.set_option("cfg_project", 10000)
        eng.set_option("cfg_norm", 500)
        whole = eng.sample("cfdg_ddpm_x0", xb.clone(), None, w=MC.W, seed=MC.PHILOX_SEED)
        x = xb.clone()
        with pytest.raises(EngineError, match=f"continues no momentum state - the step expected next is {v[0]}"):
            step(v[1], x)                             # dr_sample ended whatever was held
        for t in v:
            step(t, x)
        assert torch.equal(x, whole)                  # the sequence over the visited steps equals dr_sample
        step(v[0])
        step(v[1])
        with pytest.raises(EngineError, match=f"step {v[3]} continues no momentum state - the step expected next is {v[2]}"):
            step(v[3])
        step(v[2])                                    # (a refusal changes nothing)
        eng.set_option("cfg_momentum", -7500)         # a change of the value between steps ends the state
        with pytest.raises(EngineError, match=f"the step expected next is {v[0]}"):
            step(v[3])
        step(v[0])
        step(v[1])
        eng.set_option("cfg_momentum", -7500)         # the same value: nothing ends
        step(v[2])
        eng.set_option("x0_clip", 1)                  # an option change that ends a solver history ends the state
        with pytest.raises(EngineError, match="continues no momentum state"):
            step(v[3])
        # a refusal by one rule leaves the other's state alone: under solver order 2 an unguided first step (w = 0) starts a
        # history and no momentum state; the guided step behind it is refused by the momentum rule, and the history still stands
        eng.set_option("solver_order", 2)
        eng.step("cfdg_ddpm_x0", xb, None, v[0], w=0.0, seed=MC.PHILOX_SEED)
        with pytest.raises(EngineError, match=f"continues no momentum state - the step expected next is {v[0]}"):
            step(v[1])
        eng.step("cfdg_ddpm_x0", xb, None, v[1], w=0.0, seed=MC.PHILOX_SEED)
    finally:
        for name in ("solver_order", "x0_clip", "cfg_momentum", "cfg_project", "cfg_norm"):
            eng.set_option(name, 0)
    eng.finish()


# ---------------------------------------------------------------------------------------------- 6. windows and draws
def window_reference(recs, marks=(), draws=1, values=MC.MAIN, x_T=None, noise=None):
    """test_gpu_cfg_project.window_reference with the momentum."""
    hp, p = recs[0][0], recs[0][1]
    if x_T is None:
        x = torch.cat([BC.windows_of(r[4].reshape(r[2].T_c, 88), r[2]) for r in recs], 0)
        z = torch.cat([BC.windows_of(r[5].reshape(-1, r[2].T_c, 88), r[2]) for r in recs], 1)
    else:
        plan = recs[0][2]
        x = torch.cat([BC.windows_of(x_T[d, 0], plan) for d in range(draws)], 0)
        z = torch.cat([BC.windows_of(noise[:, d, 0], plan) for d in range(draws)], 1)
    spec = torch.cat([r[6] for r in recs], 0).repeat(draws, 1, 1)
    return MR.sample_chain(p, hp, BC.SAMPLER, x, spec, z, 0, momentum=values[0], project=values[1], norm=values[2], w=MC.W, O=BC.OPT_O,
                           marks=marks, draws=draws)


def test_windows_match_and_shared_frames_are_bit_identical():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, seen, rms = window_reference([rec])
    assert len(seen) == len(rms) == 4
    m = momentum_model(hp, p, BC.SAMPLER, *MC.MAIN, n=0)
    got = run_windows(m, one(plan), [wav], [x_T], [noise])
    for b in range(plan.n - 1):                       # the stitched roll is a plain gather
        assert torch.equal(got[b, plan.stride:], got[b + 1, :plan.overlap]), b
    d = maxdiff(got, ref[:, 0])
    record(f"windows w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    assert torch.equal(run_windows(m, one(plan), [wav], [x_T], [noise], use_graph=False), got)
    assert maxdiff(got, window_reference([rec], values=(0,) + MC.MAIN[1:])[0][:, 0]) > 100 * ATOL


def test_window_break_and_draws_match():
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = momentum_model(a[0], a[1], BC.SAMPLER, *MC.MAIN, n=0)
    got = run_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]])
    d = maxdiff(got, window_reference([a, b], marks=(2,))[0][:, 0])
    record(f"window_break w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    alone_a = run_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]])
    assert torch.equal(got[:2], alone_a)              # each recording equals its own chain
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, _, _, _ = rec
    x_T, noise = BC.option_canvases("draws")
    m = momentum_model(hp, p, BC.SAMPLER, *MC.MAIN, n=0)
    got = run_windows(m, one(plan), [wav], [x_T], [noise], D=2)
    d = maxdiff(got, window_reference([rec], draws=2, x_T=x_T, noise=noise)[0][:, 0])
    record(f"draws w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    for k in range(2):
        for bb in range(plan.n - 1):
            assert torch.equal(got[k * plan.n + bb, plan.stride:], got[k * plan.n + bb + 1, :plan.overlap])


# ---------------------------------------------------------------------------------------------- 7. the fused geometry
def test_fused_geometry_guided_steps_report_fused_stack_and_unguided_ones_come_back():
    """3 guided clips x 40 frames at C = 64, 3 layers, k = 9 - the smallest case of tests/fused_cases.py."""
    from oracle import diffroll_ref as R
    from test_gpu_respaced import hp_of, inputs
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=64, layers=3, k=9)
    p = R.synthetic_params(hp, seed=73)
    wav, x, _ = inputs(3, 40, 73)
    m = momentum_model(hp, p, "cfdg_ddpm_x0", *MC.MAIN)
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3201, 0), "tune.pw_nw": (2, 0), "tune.stack_fl": (1, 0)}
    for k, (val, _) in pins.items():
        eng.set_option(k, val)
    eng.set_option("fused_stack", 2)
    try:
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack" and eng.tail_launches == t0 and st["fallbacks"] == 0 and st["yields"] == 0, st
        e, _ = m.sample(x, wav, seed=5, use_graph=False)
        m.hparams.sampling.guidance_interval = [60, 140]
        gi, _ = m.sample(x, wav, seed=5, use_graph=False)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and 0 < eng.tail_launches - t0 <= 12 and st["fallbacks"] == 0 and st["yields"] == 0, st
        gig, _ = m.sample(x, wav, seed=5)
        eng.set_option("fused_stack", 0)              # per-phase launches: the same bits
        ppi, _ = m.sample(x, wav, seed=5)
        m.hparams.sampling.guidance_interval = None
        pp, _ = m.sample(x, wav, seed=5)
        assert eng.launch_state()["mode"] == "per_phase"
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, val) in pins.items():
            eng.set_option(k, val)
    assert torch.equal(g, e) and torch.equal(g, pp)
    assert torch.equal(gi, gig) and torch.equal(gi, ppi) and not torch.equal(gi, g)
    ref, seen, _ = MR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), MR.CR.philox_noise(5, 0, S, 3, 40), 20,
                                   momentum=MC.MAIN[0], project=MC.MAIN[1], norm=MC.MAIN[2], w=MC.W)
    assert len(seen) == 20
    ok, d = agree(g, ref)
    record(f"fused geometry w 3 values {MC.MAIN} n 20", d)
    assert ok, d


# ---------------------------------------------------------------------------------------------- 8. bf16x3 and bf16
def test_split_bf16_vs_restatement():
    hp, p, wav, x, noise = MC.setup()
    m = momentum_model(hp, p, "cfdg_ddpm_x0", *MC.MAIN, n=8, precision="bf16x3")
    ref, seen, rms = MR.sample_chain(p, hp, "cfdg_ddpm_x0", x, MC.spec_of("cfdg_ddpm_x0"), noise, 8, momentum=MC.MAIN[0], project=MC.MAIN[1],
                                     norm=MC.MAIN[2], w=MC.W)
    assert len(seen) == len(rms) == 8
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    record(f"bf16x3 w 3 values {MC.MAIN} n 8", d)
    assert ok, d


def test_bf16_chain_lies_in_the_restatements_band():
    """tests/test_gpu_bf16.py's chain (8 steps, C = 128, w = 0.5) under MAIN: the rms distance of the bf16 roll from the restated
    fp32 chain lies within 0.5 .. 1.5 x that of the restated bf16 chain, as in test_gpu_cfg_project.py."""
    import bf16_ref as Q
    from oracle import diffroll_ref as R
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    kw = dict(momentum=MC.MAIN[0], project=MC.MAIN[1], norm=MC.MAIN[2], w=0.5)
    ref, seen, _ = MR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, **kw)
    assert len(seen) == Q.CHAIN_STEPS
    with Q.patched(Q.rne, None):
        d_ref = Q.rms(MR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, **kw)[0] - ref)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16")
    m.hparams.sampling.cfg_project = 1.0
    m.hparams.sampling.cfg_norm = 0.05
    m.hparams.sampling.cfg_momentum = -0.5
    got = m.sample(x, wav, noise=nz)[0]
    d = Q.rms(got.cpu() - ref)
    print(f"\ncfg_momentum bf16 chain: rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (d, d_ref)
    assert torch.equal(m.sample(x, wav, noise=nz)[0], got)
    assert torch.equal(m.sample(x, wav, noise=nz, use_graph=False)[0], got)
    assert m.engine.cfg_momentum == -5000
