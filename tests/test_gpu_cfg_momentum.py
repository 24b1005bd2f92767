"""Option "cfg_momentum" on the MI355X (hparams.sampling.cfg_momentum): the statistics launch in its momentum form and the state
it leaves, bit for bit against the CPU restatement of tests/momentum_ref.py (dr_debug_momentum: every shape class, both launch
forms, with and without a state, zero / inf / NaN inputs and states, window canvases; twice), then the HIP chains against the
restated chain - the three guiding samplers, every row of project_cases.OPTION_CASES, eager = captured and the captured chain
launched twice (the baked start) - the identities of the option at 0 and of steps that do not guide, dr_step's state rule,
windows and draws, the fused geometry and the two bf16 precisions.  Inputs and references: tests/momentum_cases.py, which
tests/test_cfg_momentum_cpu.py shows to carry momentum.  Tolerance: agree / ATOL of tests/testlib.py; the observed
margins are recorded in profiles/momentum_margins.txt.  The scenarios every guidance stage is held to are those of
tests/stage_scenarios.py."""
import numpy as np
import pytest
import torch

from testlib import ATOL, agree, kernel_inputs, maxdiff, same_bits

import blend_cases as BC
import momentum_cases as MC
import momentum_ref as MR
import stage_scenarios as SS
import thresh_ref as TR
from stage_scenarios import one, run_batch_windows, unconditional

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

# (cfg_momentum, cfg_project, cfg_norm) of the kernel tests
TRIPLES = ((-5000, 10000, 500), (5000, 10000, 500), (-5000, 10000, 0), (5000, 10000, 0))


def mpn(momentum, project, norm):
    """The stage's values by option name."""
    return {"cfg_momentum": momentum, "cfg_project": project, "cfg_norm": norm}


MAIN = mpn(*MC.MAIN)
NOTE = f" (bound {ATOL:.0e})"


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    yield from SS.lab_engine(("cfg_momentum", "cfg_project", "cfg_norm"))


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
    with SS.window_canvases(lab, O, marks, draws) as modes:
        for mode in modes:
            want = check_kernel(lab, c, u, (None, prev), groups, plan=(O, mode), note=("windows", mode))
            for ab, m in want.values():
                assert ab.shape == (len(groups), 2) and (np.abs(ab[:, 0]) > 0.05).all()
                for lo, up in shared:
                    assert torch.equal(m[up, :O], m[lo, T - O:])


# ---------------------------------------------------------------------------------------------- 2. the chains
def record(name, d):
    """(the lines profiles/momentum_margins.txt is made of)"""
    SS.margin(f"cfg_momentum {name}", d, NOTE)


@pytest.mark.parametrize("values", MC.VALUES, ids=[str(v[0]) for v in MC.VALUES])
@pytest.mark.parametrize("sampler", MC.GUIDING)
def test_chain_vs_restatement(sampler, values):
    hp, p, wav, x, noise = MC.setup()
    m = SS.stage_model(hp, p, sampler, mpn(*values))
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
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", mpn(*values), **facade)
    ref = MC.assert_active("cfdg_ddpm_x0", *values, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, noise=noise, use_graph=False)
    assert torch.equal(roll, eager)
    ok, d = agree(roll, ref)
    record(f"with {name}, w 3 values {values} n 20", d)
    assert ok, d


# ---------------------------------------------------------------------------------------------- 3. the captured chain
def test_a_captured_chain_restarts_its_state_at_every_launch_and_the_value_is_in_its_key():
    eng, x_T = SS.chain_engine()

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
    eng, x_T = SS.chain_engine()

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
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", mpn(0, 10000, 500))
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, MC.PC.reference("cfdg_ddpm_x0", 10000, 500)[0])
    assert ok, d


@pytest.mark.parametrize("sampler,w", [("ddpm_x0", 0.0), ("ddim", 0.0), ("cfdg_ddpm_x0", 0.0)])
def test_a_chain_that_does_not_guide_is_untouched(sampler, w):
    SS.unguided_chain_is_untouched(sampler, w, {"cfg_project": 10000, "cfg_momentum": -5000}, off=("cfg_momentum", "cfg_project"))


def test_steps_outside_the_interval_keep_every_bit_and_the_state_starts_inside():
    """dr_step over the visited steps under the interval [60, 140]: the rolls behind the steps above 140 hold the same bits with
    the option on and off; the first step <= 140 starts the state (there m = d: the roll equals the projected chain's), the
    second one parts the two; the whole matches the restatement."""
    _, whole, on, off, first = SS.steps_outside_the_interval(MAIN, ("cfg_momentum",))
    assert not torch.equal(on[first + 1], off[first + 1])
    ref = MC.reference("cfdg_ddpm_x0", *MC.MAIN, philox=True, interval=(60, 140))[0]
    ok, d = agree(whole, ref)
    record("interval [60, 140], Philox, dr_step sequence", d)
    assert ok, d


# ---------------------------------------------------------------------------------------------- 5. dr_step
def test_dr_step_state_rule():
    from diffroll_amd.engine import EngineError
    eng, xb = SS.chain_engine(steps=20)
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
def window_reference(recs, values=MC.MAIN, **kw):
    return SS.window_reference(MR.sample_chain, mpn(*values), recs, **kw)


def test_windows_match_and_shared_frames_are_bit_identical():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, seen, rms = window_reference([rec])
    assert len(seen) == len(rms) == 4
    m = SS.stage_model(hp, p, BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise])
    for b in range(plan.n - 1):                       # the stitched roll is a plain gather
        assert torch.equal(got[b, plan.stride:], got[b + 1, :plan.overlap]), b
    d = maxdiff(got, ref[:, 0])
    record(f"windows w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    assert torch.equal(run_batch_windows(m, one(plan), [wav], [x_T], [noise], use_graph=False), got)
    assert maxdiff(got, window_reference([rec], values=(0,) + MC.MAIN[1:])[0][:, 0]) > 100 * ATOL


def test_window_break_and_draws_match():
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = SS.stage_model(a[0], a[1], BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]])
    d = maxdiff(got, window_reference([a, b], marks=(2,))[0][:, 0])
    record(f"window_break w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    alone_a = run_batch_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]])
    assert torch.equal(got[:2], alone_a)              # each recording equals its own chain
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, _, _, _ = rec
    x_T, noise = BC.option_canvases("draws")
    m = SS.stage_model(hp, p, BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise], D=2)
    d = maxdiff(got, window_reference([rec], draws=2, x_T=x_T, noise=noise)[0][:, 0])
    record(f"draws w 3 values {MC.MAIN}", d)
    assert d <= ATOL, d
    for k in range(2):
        for bb in range(plan.n - 1):
            assert torch.equal(got[k * plan.n + bb, plan.stride:], got[k * plan.n + bb + 1, :plan.overlap])


# ---------------------------------------------------------------------------------------------- 7. the fused geometry
def test_fused_geometry_guided_steps_report_fused_stack_and_unguided_ones_come_back():
    with SS.fused_geometry(MAIN) as (hp, p, m, wav, x):
        g = SS.fused_guided_steps_leave_the_tail_kernel(m, wav, x)
    _, seen, _ = SS.fused_roll_vs_restatement(MR.sample_chain, MAIN, hp, p, wav, x, g, f"cfg_momentum fused geometry w 3 values {MC.MAIN} n 20", NOTE)
    assert len(seen) == 20


# ---------------------------------------------------------------------------------------------- 8. bf16x3 and bf16
def test_split_bf16_vs_restatement():
    _, _, rms = SS.split_bf16_vs_restatement(MR.sample_chain, MAIN, f"cfg_momentum bf16x3 w 3 values {MC.MAIN} n 8", NOTE)
    assert len(rms) == 8


def test_bf16_chain_lies_in_the_restatements_band():
    """stage_scenarios.bf16_chain_lies_in_the_restatements_band under MAIN, as in test_gpu_cfg_project.py."""
    SS.bf16_chain_lies_in_the_restatements_band(MR.sample_chain, MAIN, "cfg_momentum")
