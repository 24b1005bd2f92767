"""Options "cfg_project" / "cfg_norm" on the MI355X (hparams.sampling.cfg_project / .cfg_norm): the statistics launch alone, bit
for bit against the CPU restatement of tests/project_ref.py (dr_debug_project: every shape class, both launch forms, zero /
inf / NaN inputs, window grouping; twice, so the ticket is shown to re-arm), then the HIP chains against the restated chain -
the three guiding samplers, injected noise and for one case the replayed Philox draws, eager = captured, with the clamp, the
solver, the guidance interval and a start step - the identities of the options at 0 and of steps that do not guide, the two
refusals, windows, the fused geometry (a guided step leaves the tail kernel, an unguided one comes back) and the two bf16
precisions.  Inputs and references: tests/project_cases.py, which tests/test_cfg_project_cpu.py shows to project - rho k >=
0.2 at every guided step and roll, s <= 0.9 where r = 0.05, and a roll at least 100 ATOL (10 ATOL under the guidance
interval) from the chain with the options off.  Tolerance: agree / ATOL of tests/testlib.py; the
scenarios every guidance stage is held to are those of tests/stage_scenarios.py."""
import numpy as np
import pytest
import torch

from testlib import ATOL, agree, kernel_inputs, maxdiff, same_bits

import blend_cases as BC
import project_cases as PC
import project_ref as PR
import stage_scenarios as SS
import thresh_ref as TR
from stage_scenarios import one, run_batch_windows, unconditional

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

# (cfg_project, cfg_norm) of the kernel tests: rho alone, both, the bound alone, a bound that never binds
PAIRS = ((10000, 0), (5000, 500), (0, 500), (10000, 100000))
IDENTITY = (np.float32(0.0), np.float32(1.0))


def pn(project, norm):
    """The stage's values by option name."""
    return {"cfg_project": project, "cfg_norm": norm}


MAIN = pn(*PC.MAIN)


def is_identity(row):
    return row[0] == IDENTITY[0] and row[1] == IDENTITY[1]


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    yield from SS.lab_engine(("cfg_project", "cfg_norm"))


def check_kernel(lab, c, u, groups, plan=None, note=()):
    """The launch on (c, u) at w = 3 under every pair of PAIRS, twice; returns the restatement's (G, 2) at (10000, 0) and at
    (5000, 500)."""
    want = {}
    try:
        for project, norm in PAIRS:
            want[project, norm] = PR.group_ab(c, u, 3.0, project, norm, groups, plan)
            lab.set_option("cfg_project", project)
            lab.set_option("cfg_norm", norm)
            got = lab.project_stats(c, u, 3.0, groups=len(groups))
            again = lab.project_stats(c, u, 3.0, groups=len(groups))
            ref = torch.from_numpy(want[project, norm])
            assert got.shape == ref.shape
            assert same_bits(got, ref), (note, project, norm, got.cpu().tolist()[:4], ref.tolist()[:4])
            assert same_bits(again, got), (note, project, norm)
    finally:
        lab.set_option("cfg_project", 0)
        lab.set_option("cfg_norm", 0)
    return want[10000, 0], want[5000, 500]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 3), (2, 40), (2, 130), (16, 125), (1, 640)])
def test_statistics_are_bit_equal_to_the_restatement(lab, B, T):
    """(2, 130): three blocks, the last one partial."""
    moved = 0
    inputs = dict(kernel_inputs(B, T, 17 + T), zero=torch.zeros(B, T, 88))
    for name, c in inputs.items():
        for u in (None, unconditional(name, B, T)):
            rho, both = check_kernel(lab, c, u, TR.clip_groups(B), note=(name, u is not None))
            if u is None or name == "only_nan":
                assert is_identity(rho[0]) and is_identity(both[0]), (name, rho, both)      # y is c / only NaN: exactly (0, 1)
            if name == "zero":
                assert is_identity(rho[0]) and both[0, 1] == (np.float32(1.0) if u is None else np.float32(0.05 / 0.25))
            if name == "one_nan":
                assert is_identity(rho[B - 1]) and is_identity(both[B - 1])
            if name == "specials":
                assert is_identity(rho[0]) and is_identity(both[0])                      # (the roll with +-inf)
            moved += int((rho[:, 0] != IDENTITY[0]).sum())
    assert moved > 0                                  # (some of these groups project)


@pytest.mark.parametrize("T", [744, 745])
def test_statistics_either_side_of_the_form_switch(lab, T):
    """T * 88 = 65472 / 65560 elements: the last roll of the one-workgroup form and the first of the grid form."""
    g = torch.Generator().manual_seed(T)
    c, u = 1.2 * torch.randn(2, T, 88, generator=g) + 0.5, torch.randn(2, T, 88, generator=g)
    rho, both = check_kernel(lab, c, u, TR.clip_groups(2))
    assert (np.abs(rho[:, 0]) > 0.1).all() and (both[:, 1] < 0.9).all()


@pytest.mark.parametrize("marks,draws", [((), 1), ((2,), 1), ((2,), 2)], ids=["one-recording", "mark-at-2", "mark-at-2-draws-2"])
@pytest.mark.parametrize("O", [1, 5, 16])
def test_statistics_over_window_canvases(lab, O, marks, draws):
    """32-frame windows, three per draw, under the three blend modes: one pair per recording, over the blended predictions."""
    T, B = 32, 3 * draws
    groups = TR.window_groups(B, O, marks, draws)
    g = torch.Generator().manual_seed(5 + B + len(marks) + O)
    inputs = dict(kernel_inputs(B, T, 23), zero=torch.zeros(B, T, 88))
    with SS.window_canvases(lab, O, marks, draws) as modes:
        for mode in modes:
            for name in ("noise", "specials", "one_nan", "zero"):
                rho, both = check_kernel(lab, inputs[name] + (0.5 if name == "noise" else 0.0), torch.randn(B, T, 88, generator=g), groups,
                                         plan=(O, mode), note=(name, mode))
                assert rho.shape == (len(groups), 2)
                if name == "noise":
                    assert (np.abs(rho[:, 0]) > 0.1).all() and (both[:, 1] < 0.9).all()
                elif name == "specials":
                    assert is_identity(rho[0]) and is_identity(both[0])                  # (the recording that holds the inf)
                elif name == "zero":
                    assert all(is_identity(row) for row in rho)                          # c = 0: nothing parallel to remove


# ---------------------------------------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("project,norm", PC.VALUES, ids=[f"{p}-{n}" for p, n in PC.VALUES])
@pytest.mark.parametrize("sampler", PC.GUIDING)
def test_chain_vs_restatement(sampler, project, norm):
    hp, p, wav, x, noise = PC.setup()
    m = SS.stage_model(hp, p, sampler, pn(project, norm))          # DR_ENAME (-> ValueError) at the first sample before the options existed
    runs = [(False, dict(noise=noise))]
    if (sampler, project, norm) == ("cfdg_ddpm_x0",) + PC.MAIN:
        runs.append((True, dict(seed=PC.PHILOX_SEED)))
    for philox, kw in runs:
        ref = PC.assert_active(sampler, project, norm, philox)      # (the inputs project, before the engine's roll is looked at)
        roll, _ = m.sample(x, wav, **kw)
        eager, _ = m.sample(x, wav, use_graph=False, **kw)
        assert torch.equal(roll, eager), (philox, maxdiff(roll.cpu(), eager.cpu()))
        ok, d = agree(roll, ref)
        print(f"\ncfg_project {sampler} w 3 values {project} / {norm} n 20 {'philox' if philox else 'injected'}: max |d| {d:.3e}")
        assert ok, (philox, d)
        assert not agree(roll, PC.reference(sampler, 0, 0, philox)[0])[0]
    assert m.engine.cfg_project == project and m.engine.cfg_norm == norm
    assert m.engine.launch_state()["mode"] != "fused_stack+tail"


@pytest.mark.parametrize("name,kw,facade", PC.OPTION_CASES, ids=[c[0] for c in PC.OPTION_CASES])
def test_other_options_vs_restatement(name, kw, facade):
    hp, p, wav, x, noise = PC.setup()
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", MAIN, **facade)
    ref = PC.assert_active("cfdg_ddpm_x0", *PC.MAIN, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    eager, _ = m.sample(x, wav, noise=noise, use_graph=False)
    assert torch.equal(roll, eager)
    ok, d = agree(roll, ref)
    print(f"\ncfg_project with {name}, w 3 values {PC.MAIN} n 20: max |d| {d:.3e}")
    assert ok, d
    assert not agree(roll, PC.reference("cfdg_ddpm_x0", *PC.MAIN)[0])[0]      # the option beside the projection matters on these inputs


# ---------------------------------------------------------------------------------------------- 3. identities
def test_values_0_are_the_parents_chain_bitwise_and_so_is_a_bound_that_never_binds():
    hp, p, wav, x, noise = PC.setup()
    never, _ = SS.stage_model(hp, p, "cfdg_ddpm_x0", pn(0, 0)).sample(x, wav, noise=noise)
    m = SS.stage_model(hp, p, "cfdg_ddpm_x0", MAIN)
    on, _ = m.sample(x, wav, noise=noise)
    m.hparams.sampling.cfg_project = None
    m.hparams.sampling.cfg_norm = 10.0                # rho = 0 and r = 10: (a, b) = (0, 1) at every step, through the projecting form
    loose, _ = m.sample(x, wav, noise=noise)
    assert m.engine.cfg_project == 0 and m.engine.cfg_norm == 100000
    m.hparams.sampling.cfg_norm = None
    off, _ = m.sample(x, wav, noise=noise)
    assert m.engine.cfg_project == 0 and m.engine.cfg_norm == 0
    assert torch.equal(off, never) and torch.equal(loose, never) and not torch.equal(on, off)
    ok, d = agree(off, PC.reference("cfdg_ddpm_x0", 0, 0)[0])
    assert ok, d


@pytest.mark.parametrize("sampler,w", [("ddpm_x0", 0.0), ("generation_ddpm_x0", 0.0), ("ddim_x0", 0.0), ("ddim", 0.0), ("cfdg_ddpm_x0", 0.0)])
def test_a_chain_that_does_not_guide_is_untouched(sampler, w):
    SS.unguided_chain_is_untouched(sampler, w, MAIN)


def test_steps_outside_the_interval_are_untouched():
    """stage_scenarios.steps_outside_the_interval; the first guided step parts the two trajectories.  (That the unguided steps
    keep the tail kernel's launches moving is held at the fused geometry below.)"""
    _, _, on, off, first_guided = SS.steps_outside_the_interval(MAIN, ("cfg_project", "cfg_norm"))
    assert not torch.equal(on[first_guided], off[first_guided])


def test_the_values_are_part_of_the_captured_chains_key():
    """Setting the options drops nothing - back at the values it was captured under the chain replays, no launch counted - and
    a chain captured under other values is not replayed."""
    with SS.captured_under("cfg_project", 10000, 5000, ("cfg_project", "cfg_norm")) as (eng, run, first, c1):
        eng.set_option("cfg_project", 10000)
        eng.set_option("cfg_norm", 500)
        bound = run()
        assert eng.launch_counts() != c1 and not torch.equal(bound, first)
        eng.set_option("cfg_norm", 0)
        assert torch.equal(run(), first)


def test_a_change_of_a_value_ends_a_dr_step_history_and_bad_values_are_refused():
    SS.bad_values_and_step_history({"cfg_project": (-1, 10001, 70000), "cfg_norm": (-1, 100001, 700000)},
                                   ("cfg_project", 10000), ("cfg_norm", 500))


@pytest.mark.parametrize("mine", ["cfg_project", "cfg_norm"])
def test_both_combinations_are_refused_at_sample_time(mine):
    """Beside "x0_threshold" and beside "cfg_rescale": DR_EINVAL (-> ValueError) from the call, naming both options; with the
    other option back at 0 the same engine samples."""
    eng, x_T = SS.chain_engine()

    def run():
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=PC.W, seed=PC.PHILOX_SEED)

    eng.set_option(mine, 500)
    try:
        eng.set_option("cfg_rescale", 7000)
        with pytest.raises(ValueError, match="cfg_project = .* cfg_norm = .*cfg_rescale = 7000"):
            run()
        with pytest.raises(ValueError, match="cfg_rescale"):
            eng.step("cfdg_ddpm_x0", x_T.clone(), None, 199, w=PC.W)
        with pytest.raises(ValueError, match="cfg_rescale"):
            eng.project_stats(torch.zeros(1, 4, 88), torch.ones(1, 4, 88), 3.0)
        eng.set_option("cfg_rescale", 0)
        eng.set_option("x0_clip", 1)
        eng.set_option("x0_threshold", 9950)
        with pytest.raises(ValueError, match="cfg_project = .* cfg_norm = .*x0_threshold = 9950"):
            run()
        eng.set_option("x0_threshold", 0)
        clipped = run()
        eng.finish()
        assert torch.isfinite(clipped).all() and float(clipped.min()) >= 0.0
    finally:
        for name in ("cfg_rescale", "x0_threshold", "x0_clip", mine):
            eng.set_option(name, 0)


# ---------------------------------------------------------------------------------------------- 4. windows
def window_reference(recs, values=PC.MAIN, **kw):
    return SS.window_reference(PR.sample_chain, pn(*values), recs, **kw)


def moved(seen, groups):
    """Every guided step of the restated chain has `groups` pairs, none of them the identity."""
    return all(len(rows) == groups and all(np.float32(a) != 0 or np.float32(b) != 1 for _, _, _, a, b in rows) for rows in seen.values())


def test_windows_share_one_pair_per_recording():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, seen = window_reference([rec])
    assert len(seen) == 4 and moved(seen, 1)
    m = SS.stage_model(hp, p, BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise])
    for b in range(plan.n - 1):                       # all windows of the recording use the same (a, b) on the same blended values
        assert torch.equal(got[b, plan.stride:], got[b + 1, :plan.overlap]), b
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project windows w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    assert torch.equal(run_batch_windows(m, one(plan), [wav], [x_T], [noise], use_graph=False), got)
    assert maxdiff(got, window_reference([rec], values=(0, 0))[0][:, 0]) > 100 * ATOL


def test_window_break_projects_per_recording():
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = SS.stage_model(a[0], a[1], BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]])
    ref, seen = window_reference([a, b], marks=(2,))
    assert moved(seen, 2) and all(rows[0][3] != rows[1][3] for rows in seen.values())
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project window_break w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    # each recording equals its own chain, bit for bit
    alone_a = run_batch_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]])
    alone_b = run_batch_windows(m, one(b[2]), [b[3]], [b[4]], [b[5]])
    assert torch.equal(got[:2], alone_a) and torch.equal(got[2:], alone_b)


def test_draws_project_per_draw():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, _, _, _ = rec
    x_T, noise = BC.option_canvases("draws")
    m = SS.stage_model(hp, p, BC.SAMPLER, MAIN, n=0)
    got = run_batch_windows(m, one(plan), [wav], [x_T], [noise], D=2)
    ref, seen = window_reference([rec], draws=2, x_T=x_T, noise=noise)
    assert moved(seen, 2)
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project draws w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    for k in range(2):                                # each draw equals its own chain: the tiled batch, draw by draw
        alone = run_batch_windows(m, one(plan), [wav], [x_T[k:k + 1]], [noise[:, k:k + 1]])
        assert torch.equal(got[k * plan.n:(k + 1) * plan.n], alone), k


# ---------------------------------------------------------------------------------------------- 5. the fused geometry
def test_fused_geometry_guided_steps_leave_the_tail_kernel_and_unguided_ones_come_back():
    with SS.fused_geometry(MAIN) as (hp, p, m, wav, x):
        off = SS.fused_chain_with_the_options_off(m, wav, x, MAIN)
        g = SS.fused_guided_steps_leave_the_tail_kernel(m, wav, x)
    assert not torch.equal(g, off)
    _, seen = SS.fused_roll_vs_restatement(PR.sample_chain, MAIN, hp, p, wav, x, g, f"cfg_project fused geometry w 3 values {PC.MAIN} n 20")
    assert len(seen) == 20


# ---------------------------------------------------------------------------------------------- 6. bf16x3 and bf16
def test_split_bf16_vs_restatement():
    _, seen = SS.split_bf16_vs_restatement(PR.sample_chain, MAIN, f"cfg_project bf16x3 w 3 values {PC.MAIN} n 8")
    assert all(rho * k >= 0.2 and s <= 0.9 for rows in seen.values() for k, rho, s, _, _ in rows)


def test_bf16_chain_lies_in_the_restatements_band():
    """stage_scenarios.bf16_chain_lies_in_the_restatements_band with rho = 1 and r = 0.05 - both restatements project."""
    (_, seen), B = SS.bf16_chain_lies_in_the_restatements_band(PR.sample_chain, MAIN, "cfg_project")
    assert moved(seen, B)
