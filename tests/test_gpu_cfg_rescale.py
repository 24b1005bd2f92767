"""Option "cfg_rescale" on the MI355X (hparams.sampling.cfg_rescale): the statistics launch alone, bit for bit against the CPU
restatement of tests/rescale_ref.py (dr_debug_rescale: every shape class, both launch forms, tie / zero / inf / NaN inputs,
window grouping; twice, so the ticket is shown to re-arm), then the HIP chains against the restated chain - the three
guiding samplers, injected noise and the replayed Philox draws, eager = captured, with the clamp, the thresholding, the
solver, the guidance interval and a start step - the identities of the option at 0 and of steps that do not guide, windows,
the fused geometry (a guided step leaves the tail kernel, an unguided one comes back) and the two bf16 precisions.  Inputs
and references: tests/rescale_cases.py, which tests/test_cfg_rescale_cpu.py shows to rescale - by rescale_cases.assert_active's
own bound, |g - 1| >= 0.2 at every guided step and a roll at least 100 ATOL (10 ATOL under the guidance interval, whose last
six steps are unguided) from the unrescaled one; the issue's figures, |g - 1| >= 0.4 and 100 ATOL, are asserted there on the
inputs it names, clip_cases.setup().  Tolerance: agree / ATOL of tests/testlib.py; the
scenarios every guidance stage is held to are those of tests/stage_scenarios.py."""
import numpy as np
import pytest
import torch

from testlib import ATOL, agree, kernel_inputs, maxdiff, same_bits

import blend_cases as BC
import rescale_cases as RC
import rescale_ref as RR
import stage_scenarios as SS
import thresh_ref as TR
from stage_scenarios import one, run_batch_windows, unconditional

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

PHIS = (1, 5000, 7000, 10000)


def want_g(c, u, w, groups, plan=None):
    """phi -> (G,) fp32 of the restatement (the sums are formed once per input)."""
    return {phi: RR.group_g(c, u, w, phi, groups, plan) for phi in PHIS}


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    yield from SS.lab_engine(("cfg_rescale",))


def check_kernel(lab, c, u, groups, plan=None, note=()):
    """The launch on (c, u) at w = 3 under every phi, twice; returns the restatement's g at phi = 7000."""
    want = want_g(c, u, 3.0, groups, plan)
    for phi in PHIS:
        lab.set_option("cfg_rescale", phi)
        got = lab.rescale_stats(c, u, 3.0, groups=len(groups))
        again = lab.rescale_stats(c, u, 3.0, groups=len(groups))
        assert same_bits(got, torch.from_numpy(want[phi])), (note, phi, got.cpu().tolist()[:4], want[phi].tolist()[:4])
        assert same_bits(again, got), (note, phi)
    return want[7000]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 3), (2, 40), (16, 125), (1, 640)])
def test_statistics_are_bit_equal_to_the_restatement(lab, B, T):
    moved = 0
    for name, c in kernel_inputs(B, T, 17 + T).items():
        for u in (None, unconditional(name, B, T)):
            g = check_kernel(lab, c, u, TR.clip_groups(B), note=(name, u is not None))
            if u is None or name in ("equal", "only_nan"):
                assert g[0] == np.float32(1.0), (name, g)            # y is c / a constant roll / only NaN: exactly 1.0f
            if name == "one_nan":
                assert g[B - 1] == np.float32(1.0)
            if name == "specials":
                assert g[0] == np.float32(1.0)                       # (the roll with +-inf)
            moved += int((g != np.float32(1.0)).sum())
    assert moved > 0                                  # (some of these groups rescale)


@pytest.mark.parametrize("T", [744, 745])
def test_statistics_either_side_of_the_form_switch(lab, T):
    """T * 88 = 65472 / 65560 elements: the last roll of the one-workgroup form and the first of the grid form."""
    g = torch.Generator().manual_seed(T)
    c, u = 1.2 * torch.randn(2, T, 88, generator=g), torch.randn(2, T, 88, generator=g)
    got = check_kernel(lab, c, u, TR.clip_groups(2))
    assert (np.abs(got - 1.0) > 0.1).all()


@pytest.mark.parametrize("marks,draws", [((), 1), ((2,), 1), ((2,), 2)], ids=["one-recording", "mark-at-2", "mark-at-2-draws-2"])
@pytest.mark.parametrize("O", [1, 5, 16])
def test_statistics_over_window_canvases(lab, O, marks, draws):
    """32-frame windows, three per draw, under the three blend modes: one g per recording, over the blended predictions."""
    T, B = 32, 3 * draws
    groups = TR.window_groups(B, O, marks, draws)
    g = torch.Generator().manual_seed(5 + B + len(marks) + O)
    inputs = kernel_inputs(B, T, 23)
    with SS.window_canvases(lab, O, marks, draws) as modes:
        for mode in modes:
            for name in ("noise", "specials", "one_nan"):
                got = check_kernel(lab, inputs[name], torch.randn(B, T, 88, generator=g), groups, plan=(O, mode), note=(name, mode))
                assert got.shape == (len(groups),)
                if name == "noise":
                    assert (np.abs(got - 1.0) > 0.1).all()
                else:
                    assert got[0] == np.float32(1.0) or name == "one_nan"      # (the recording that holds the inf)


# ---------------------------------------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("value", RC.VALUES)
@pytest.mark.parametrize("sampler", RC.GUIDING)
def test_chain_vs_restatement(sampler, value):
    hp, p, wav, x, noise = RC.setup()
    m = SS.stage_model(hp, p, sampler, {"cfg_rescale": value})
    for philox, kw in ((False, dict(noise=noise)), (True, dict(seed=RC.PHILOX_SEED))):
        ref = RC.assert_active(sampler, value, philox)       # (the inputs rescale, before the engine's roll is looked at)
        roll, _ = m.sample(x, wav, **kw)
        eager, _ = m.sample(x, wav, use_graph=False, **kw)
        assert torch.equal(roll, eager), (philox, maxdiff(roll.cpu(), eager.cpu()))
        ok, d = agree(roll, ref)
        print(f"\ncfg_rescale {sampler} w 3 value {value} n 20 {'philox' if philox else 'injected'}: max |d| {d:.3e}")
        assert ok, (philox, d)
        assert not agree(roll, RC.reference(sampler, 0, philox)[0])[0]
    assert m.engine.cfg_rescale == value
    assert m.engine.launch_state()["mode"] != "fused_stack+tail"


@pytest.mark.parametrize("name,kw,facade", RC.OPTION_CASES, ids=[c[0] for c in RC.OPTION_CASES])
def test_other_options_vs_restatement(name, kw, facade):
    hp, p, wav, x, noise = RC.setup()
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", {"cfg_rescale": 7000}, **facade)
    ref = RC.assert_active("cfdg_ddpm_x0", 7000, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, noise=noise, use_graph=False)
    assert torch.equal(roll, eager)
    ok, d = agree(roll, ref)
    print(f"\ncfg_rescale with {name}, w 3 value 7000 n 20: max |d| {d:.3e}")
    assert ok, d
    assert not agree(roll, RC.reference("cfdg_ddpm_x0", 7000)[0])[0]      # the option beside the rescale matters on these inputs


# ---------------------------------------------------------------------------------------------- 3. identities
def test_value_0_is_the_parents_chain_bitwise():
    hp, p, wav, x, noise = RC.setup()
    never, _ = SS.stage_model(hp, p, "cfdg_ddpm_x0", {"cfg_rescale": 0}).sample(x, wav, noise=noise)
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", {"cfg_rescale": 7000})
    on, _ = m.sample(x, wav, noise=noise)
    m.hparams.sampling.cfg_rescale = None
    off, _ = m.sample(x, wav, noise=noise)
    assert m.engine.cfg_rescale == 0
    assert torch.equal(off, never) and not torch.equal(on, off)
    ok, d = agree(off, RC.reference("cfdg_ddpm_x0", 0)[0])
    assert ok, d


@pytest.mark.parametrize("sampler,w", [("ddpm_x0", 0.0), ("generation_ddpm_x0", 0.0), ("ddim_x0", 0.0), ("ddim", 0.0), ("cfdg_ddpm_x0", 0.0)])
def test_a_chain_that_does_not_guide_is_untouched(sampler, w):
    SS.unguided_chain_is_untouched(sampler, w, {"cfg_rescale": 7000})


def test_steps_outside_the_interval_are_untouched():
    """stage_scenarios.steps_outside_the_interval; the first guided step parts the two trajectories."""
    _, _, on, off, first_guided = SS.steps_outside_the_interval({"cfg_rescale": 7000}, ("cfg_rescale",))
    assert not torch.equal(on[first_guided], off[first_guided])


def test_the_value_is_part_of_the_captured_chains_key():
    """Setting the option drops nothing - back at the value it was captured under the chain replays, no launch counted - and
    a chain captured under another value is not replayed."""
    with SS.captured_under("cfg_rescale", 7000, 5000, ("cfg_rescale",)) as (eng, run, first, _):
        eng.set_option("cfg_rescale", 7000)
        assert torch.equal(run(), first)


def test_a_change_of_the_value_ends_a_dr_step_history_and_bad_values_are_refused():
    SS.bad_values_and_step_history({"cfg_rescale": (-1, 10001, 70000)}, ("cfg_rescale", 7000), ("cfg_rescale", 5000))


# ---------------------------------------------------------------------------------------------- 4. windows
def window_reference(recs, value=7000, **kw):
    return SS.window_reference(RR.sample_chain, {"cfg_rescale": value}, recs, **kw)


def test_windows_share_one_factor_per_recording():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, gs = window_reference([rec])
    assert all(g.shape == (1,) and abs(float(g[0]) - 1.0) >= 0.2 for g in gs.values()) and len(gs) == 4
    m = SS.stage_model(hp, p, BC.SAMPLER, {"cfg_rescale": 7000}, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise])
    for b in range(plan.n - 1):                       # all windows of the recording use the same g on the same mean
        assert torch.equal(got[b, plan.stride:], got[b + 1, :plan.overlap]), b
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_rescale windows w 3 value 7000: max |d| {d:.3e}")
    assert d <= ATOL, d
    assert torch.equal(run_batch_windows(m, one(plan), [wav], [x_T], [noise], use_graph=False), got)
    assert maxdiff(got, window_reference([rec], value=0)[0][:, 0]) > 100 * ATOL


def test_window_break_rescales_per_recording():
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = SS.stage_model(a[0], a[1], BC.SAMPLER, {"cfg_rescale": 7000}, n=0)
    got = run_batch_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]])
    ref, gs = window_reference([a, b], marks=(2,))
    assert all(g.shape == (2,) and g[0] != g[1] for g in gs.values())
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_rescale window_break w 3 value 7000: max |d| {d:.3e}")
    assert d <= ATOL, d
    # each recording equals its own chain, bit for bit
    alone_a = run_batch_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]])
    alone_b = run_batch_windows(m, one(b[2]), [b[3]], [b[4]], [b[5]])
    assert torch.equal(got[:2], alone_a) and torch.equal(got[2:], alone_b)


def test_draws_rescale_per_draw():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, _, _, _ = rec
    x_T, noise = BC.option_canvases("draws")
    m = SS.stage_model(hp, p, BC.SAMPLER, {"cfg_rescale": 7000}, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise], D=2)
    ref, gs = window_reference([rec], draws=2, x_T=x_T, noise=noise)
    assert all(g.shape == (2,) for g in gs.values())
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_rescale draws w 3 value 7000: max |d| {d:.3e}")
    assert d <= ATOL, d
    for k in range(2):                                # each draw equals its own chain: the tiled batch, draw by draw
        alone = run_batch_windows(m, one(plan), [wav], [x_T[k:k + 1]], [noise[:, k:k + 1]])
        assert torch.equal(got[k * plan.n:(k + 1) * plan.n], alone), k


# ---------------------------------------------------------------------------------------------- 5. the fused geometry
def test_fused_geometry_guided_steps_leave_the_tail_kernel_and_unguided_ones_come_back():
    values = {"cfg_rescale": 7000}
    with SS.fused_geometry(values) as (hp, p, m, wav, x):
        off = SS.fused_chain_with_the_options_off(m, wav, x, values)
        g = SS.fused_guided_steps_leave_the_tail_kernel(m, wav, x)
    assert not torch.equal(g, off)
    SS.fused_roll_vs_restatement(RR.sample_chain, values, hp, p, wav, x, g, "cfg_rescale fused geometry w 3 value 7000 n 20")


# ---------------------------------------------------------------------------------------------- 6. bf16x3 and bf16
def test_split_bf16_vs_restatement():
    _, gs = SS.split_bf16_vs_restatement(RR.sample_chain, {"cfg_rescale": 7000}, "cfg_rescale bf16x3 w 3 value 7000 n 8")
    assert all((np.abs(g - 1.0) >= 0.2).all() for g in gs.values())


def test_bf16_chain_lies_in_the_restatements_band():
    """stage_scenarios.bf16_chain_lies_in_the_restatements_band with the option at 0.7 - both restatements rescale."""
    (_, gs), _ = SS.bf16_chain_lies_in_the_restatements_band(RR.sample_chain, {"cfg_rescale": 7000}, "cfg_rescale")
    assert all((np.abs(g - 1.0) >= 0.05).all() for g in gs.values())
