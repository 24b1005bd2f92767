"""Options "cfg_project" / "cfg_norm" on the MI355X (hparams.sampling.cfg_project / .cfg_norm): the statistics launch alone, bit
for bit against the CPU restatement of tests/project_ref.py (dr_debug_project: every shape class, both launch forms, zero /
inf / NaN inputs, window grouping; twice, so the ticket is shown to re-arm), then the HIP chains against the restated chain -
the three guiding samplers, injected noise and for one case the replayed Philox draws, eager = captured, with the clamp, the
solver, the guidance interval and a start step - the identities of the options at 0 and of steps that do not guide, the two
refusals, windows, the fused geometry (a guided step leaves the tail kernel, an unguided one comes back) and the two bf16
precisions.  Inputs and references: tests/project_cases.py, which tests/test_cfg_project_cpu.py shows to project - rho k >=
0.2 at every guided step and roll, s <= 0.9 where r = 0.05, and a roll at least 100 ATOL (10 ATOL under the guidance
interval) from the chain with the options off.  Tolerance: agree / ATOL of tests/test_gpu_respaced.py."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_model, maxdiff
from test_gpu_respaced import ATOL, S, agree
from test_gpu_x0_threshold import kernel_inputs, same_bits

import blend_cases as BC
import clip_ref as CL
import project_cases as PC
import project_ref as PR
import thresh_ref as TR

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

# (cfg_project, cfg_norm) of the kernel tests: rho alone, both, the bound alone, a bound that never binds
PAIRS = ((10000, 0), (5000, 500), (0, 500), (10000, 100000))
IDENTITY = (np.float32(0.0), np.float32(1.0))


def project_model(hp, p, sampler, project, norm, n=PC.N_STEPS, w=PC.W, code=0, **kw):
    """The facade with hparams.sampling.cfg_project / .cfg_norm = the values / 10000 and, where asked for, x0_clip over the
    range of `code` and the other sampling keys."""
    options = {k: kw.pop(k) for k in ("solver_order", "solver_noise", "guidance_interval", "strength") if k in kw}
    m = make_model(hp, p, sampler=sampler, w=w, inpainting_t=PC.mask_of(sampler), **kw)
    m.hparams.sampling.steps = n or None
    m.hparams.sampling.cfg_project = project / 10000.0 if project else None
    m.hparams.sampling.cfg_norm = norm / 10000.0 if norm else None
    if code:
        m.hparams.sampling.x0_clip = 1
        m.hparams.norm_args[0:2] = list(CL.BOUNDS[code])
    for k, val in options.items():
        setattr(m.hparams.sampling, k, val)
    return m


def is_identity(row):
    return row[0] == IDENTITY[0] and row[1] == IDENTITY[1]


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    """A committed engine whose options the kernel tests set; handed back with every one of them off."""
    hp, p, _, _, _ = PC.setup()
    eng = make_model(hp, p, sampler="cfdg_ddpm_x0").engine
    yield eng
    for name, value in (("window_overlap", 0), ("window_blend", 0), ("window_break", 0), ("draws", 1), ("cfg_project", 0), ("cfg_norm", 0)):
        eng.set_option(name, value)


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


def unconditional(name, B, T):
    """Normal noise beside the noise input, a constant beside the special ones (it keeps them all-equal / inf / NaN)."""
    return torch.randn(B, T, 88, generator=torch.Generator().manual_seed(T)) if name == "noise" else torch.full((B, T, 88), 0.25)


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
    try:
        lab.set_option("window_overlap", O)
        lab.set_window_breaks(marks)
        lab.set_option("draws", draws)
        for mode in (0, 1, 2):
            lab.set_option("window_blend", mode)
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
    finally:
        lab.set_option("draws", 1)
        lab.set_window_breaks(())
        lab.set_option("window_blend", 0)
        lab.set_option("window_overlap", 0)


# ---------------------------------------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("project,norm", PC.VALUES, ids=[f"{p}-{n}" for p, n in PC.VALUES])
@pytest.mark.parametrize("sampler", PC.GUIDING)
def test_chain_vs_restatement(sampler, project, norm):
    hp, p, wav, x, noise = PC.setup()
    m = project_model(hp, p, sampler, project, norm)          # DR_ENAME (-> ValueError) at the first sample before the options existed
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
    m = project_model(hp, p, "cfdg_ddpm_x0", *PC.MAIN, **facade)
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
    never, _ = project_model(hp, p, "cfdg_ddpm_x0", 0, 0).sample(x, wav, noise=noise)
    m = project_model(hp, p, "cfdg_ddpm_x0", *PC.MAIN)
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
    """The engine ignores the values for a sampler that does not guide and for a w = 0 chain: the same bits, the captured chain
    replayed (no launch counted), the tail kernel's launches moving as without them."""
    hp, p, wav, x, _ = PC.setup()
    m = make_model(hp, p, sampler=sampler, w=w)
    m.hparams.sampling.steps = 4
    eng = m.engine
    eng.frontend(wav, PC.TN)
    x_T = x.squeeze(1).to(eng.device).contiguous()

    def run():
        t0 = eng.tail_launches
        return eng.sample(sampler, x_T.clone(), None, w=w, seed=PC.PHILOX_SEED), eng.tail_launches - t0

    (first, tails), c0 = run(), eng.launch_counts()
    eng.set_option("cfg_project", 10000)
    eng.set_option("cfg_norm", 500)
    try:
        (again, tails_on), c1 = run(), eng.launch_counts()
        eager = eng.sample(sampler, x_T.clone(), None, w=w, seed=PC.PHILOX_SEED, use_graph=False)
    finally:
        eng.set_option("cfg_project", 0)
        eng.set_option("cfg_norm", 0)
    assert torch.equal(again, first) and torch.equal(eager, first)
    assert tails_on == tails
    assert c1 == c0, (c0, c1)                         # (the values are not part of such a chain's key: replayed)


def test_steps_outside_the_interval_are_untouched():
    """dr_step over the visited steps under the interval [60, 140]: the rolls behind the steps above 140 hold the same bits
    with the options on and off; the first guided step parts them.  (That the unguided steps keep the tail kernel's launches
    moving is held at the fused geometry below.)"""
    hp, p, wav, x, _ = PC.setup()
    m = project_model(hp, p, "cfdg_ddpm_x0", *PC.MAIN, guidance_interval=[60, 140])
    kw = dict(seed=PC.PHILOX_SEED)
    on, _ = m.sample_trajectory(x, wav, **kw)
    whole, _ = m.sample(x, wav, **kw)
    assert torch.equal(whole, on[-1])                 # dr_step follows the rule for its one step
    m.hparams.sampling.cfg_project = None
    m.hparams.sampling.cfg_norm = None
    off, _ = m.sample_trajectory(x, wav, **kw)
    visited = m.visited_steps()
    above = [i for i, t in enumerate(visited) if t > 140]
    first_guided = above[-1] + 1
    assert above and 60 <= visited[first_guided] <= 140
    for i in above:
        assert torch.equal(on[i], off[i]), visited[i]
    assert not torch.equal(on[first_guided], off[first_guided])


def test_the_values_are_part_of_the_captured_chains_key():
    """Setting the options drops nothing - back at the values it was captured under the chain replays, no launch counted - and
    a chain captured under other values is not replayed."""
    hp, p, wav, x, _ = PC.setup()
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=PC.W)
    m.hparams.sampling.steps = 4
    eng = m.engine
    eng.frontend(wav, PC.TN)
    x_T = x.squeeze(1).to(eng.device).contiguous()

    def run():
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=PC.W, seed=PC.PHILOX_SEED)

    eng.set_option("cfg_project", 10000)
    try:
        first, c0 = run(), eng.launch_counts()
        assert sum(c0) > 0
        eng.set_option("cfg_project", 5000)
        eng.set_option("cfg_project", 10000)
        assert torch.equal(run(), first) and eng.launch_counts() == c0
        eng.set_option("cfg_project", 5000)
        other, c1 = run(), eng.launch_counts()
        assert c1 != c0 and not torch.equal(other, first)
        eng.set_option("cfg_project", 10000)
        eng.set_option("cfg_norm", 500)
        bound = run()
        assert eng.launch_counts() != c1 and not torch.equal(bound, first)
        eng.set_option("cfg_norm", 0)
        assert torch.equal(run(), first)
    finally:
        eng.set_option("cfg_project", 0)
        eng.set_option("cfg_norm", 0)


def test_a_change_of_a_value_ends_a_dr_step_history_and_bad_values_are_refused():
    from diffroll_amd.engine import EngineError
    hp, p, wav, x, _ = PC.setup()
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=PC.W)
    eng = m.engine
    for name, bads in (("cfg_project", (-1, 10001, 70000)), ("cfg_norm", (-1, 100001, 700000))):
        for bad in bads:
            with pytest.raises(ValueError, match=f"{name}.*{bad}"):
                eng.set_option(name, bad)
    assert eng.cfg_project == 0 and eng.cfg_norm == 0
    eng.frontend(wav, PC.TN)
    eng.set_option("sampling_steps", 20)
    eng.set_option("solver_order", 2)
    v = eng.visited_steps()
    xb = x.squeeze(1).to(eng.device).contiguous()

    def step(t):
        eng.step("cfdg_ddpm_x0", xb, None, t, w=PC.W)

    try:
        step(v[0])
        step(v[1])
        eng.set_option("cfg_project", 10000)
        with pytest.raises(EngineError, match="continues no history"):
            step(v[2])
        step(v[0])
        step(v[1])
        eng.set_option("cfg_project", 10000)          # the same value: nothing ends
        step(v[2])
        eng.set_option("cfg_norm", 500)
        with pytest.raises(EngineError, match="continues no history"):
            step(v[3])
    finally:
        eng.set_option("cfg_project", 0)
        eng.set_option("cfg_norm", 0)
    eng.finish()


@pytest.mark.parametrize("mine", ["cfg_project", "cfg_norm"])
def test_both_combinations_are_refused_at_sample_time(mine):
    """Beside "x0_threshold" and beside "cfg_rescale": DR_EINVAL (-> ValueError) from the call, naming both options; with the
    other option back at 0 the same engine samples."""
    hp, p, wav, x, _ = PC.setup()
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=PC.W)
    m.hparams.sampling.steps = 4
    eng = m.engine
    eng.frontend(wav, PC.TN)
    x_T = x.squeeze(1).to(eng.device).contiguous()

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
def one(plan):
    return longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)


def run_windows(m, batch, wavs, x_T, noise, D=1, use_graph=True):
    return m._sample_windows(batch, wavs, x_T, noise, D, 0, 0, use_graph, True).cpu()


def window_reference(recs, marks=(), draws=1, values=PC.MAIN, x_T=None, noise=None):
    """The restated chain over the windows of the recordings `recs` (blend_cases.recording tuples) in one batch."""
    hp, p = recs[0][0], recs[0][1]
    if x_T is None:
        x = torch.cat([BC.windows_of(r[4].reshape(r[2].T_c, 88), r[2]) for r in recs], 0)
        z = torch.cat([BC.windows_of(r[5].reshape(-1, r[2].T_c, 88), r[2]) for r in recs], 1)
    else:
        plan = recs[0][2]
        x = torch.cat([BC.windows_of(x_T[d, 0], plan) for d in range(draws)], 0)
        z = torch.cat([BC.windows_of(noise[:, d, 0], plan) for d in range(draws)], 1)
    spec = torch.cat([r[6] for r in recs], 0).repeat(draws, 1, 1)
    return PR.sample_chain(p, hp, BC.SAMPLER, x, spec, z, 0, project=values[0], norm=values[1], w=PC.W, O=BC.OPT_O, marks=marks, draws=draws)


def moved(seen, groups):
    """Every guided step of the restated chain has `groups` pairs, none of them the identity."""
    return all(len(rows) == groups and all(np.float32(a) != 0 or np.float32(b) != 1 for _, _, _, a, b in rows) for rows in seen.values())


def test_windows_share_one_pair_per_recording():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, x_T, noise, _ = rec
    ref, seen = window_reference([rec])
    assert len(seen) == 4 and moved(seen, 1)
    m = project_model(hp, p, BC.SAMPLER, *PC.MAIN, n=0)
    got = run_windows(m, one(plan), [wav], [x_T], [noise])
    for b in range(plan.n - 1):                       # all windows of the recording use the same (a, b) on the same blended values
        assert torch.equal(got[b, plan.stride:], got[b + 1, :plan.overlap]), b
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project windows w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    assert torch.equal(run_windows(m, one(plan), [wav], [x_T], [noise], use_graph=False), got)
    assert maxdiff(got, window_reference([rec], values=(0, 0))[0][:, 0]) > 100 * ATOL


def test_window_break_projects_per_recording():
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = project_model(a[0], a[1], BC.SAMPLER, *PC.MAIN, n=0)
    got = run_windows(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]])
    ref, seen = window_reference([a, b], marks=(2,))
    assert moved(seen, 2) and all(rows[0][3] != rows[1][3] for rows in seen.values())
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project window_break w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    # each recording equals its own chain, bit for bit
    alone_a = run_windows(m, one(a[2]), [a[3]], [a[4]], [a[5]])
    alone_b = run_windows(m, one(b[2]), [b[3]], [b[4]], [b[5]])
    assert torch.equal(got[:2], alone_a) and torch.equal(got[2:], alone_b)


def test_draws_project_per_draw():
    rec = BC.recording(BC.OPT_O, 3300)
    hp, p, plan, wav, _, _, _ = rec
    x_T, noise = BC.option_canvases("draws")
    m = project_model(hp, p, BC.SAMPLER, *PC.MAIN, n=0)
    got = run_windows(m, one(plan), [wav], [x_T], [noise], D=2)
    ref, seen = window_reference([rec], draws=2, x_T=x_T, noise=noise)
    assert moved(seen, 2)
    d = maxdiff(got, ref[:, 0])
    print(f"\ncfg_project draws w 3 values {PC.MAIN}: max |d| {d:.3e}")
    assert d <= ATOL, d
    for k in range(2):                                # each draw equals its own chain: the tiled batch, draw by draw
        alone = run_windows(m, one(plan), [wav], [x_T[k:k + 1]], [noise[:, k:k + 1]])
        assert torch.equal(got[k * plan.n:(k + 1) * plan.n], alone), k


# ---------------------------------------------------------------------------------------------- 5. the fused geometry
def test_fused_geometry_guided_steps_leave_the_tail_kernel_and_unguided_ones_come_back():
    """3 guided clips x 40 frames at C = 64, 3 layers, k = 9 - the smallest case of tests/fused_cases.py, which runs
    fused_stack+tail under "fused_stack" 2: under the options a guided step keeps its fused stack launch and runs head
    projections, statistics and update as ordinary launches; under an interval the unguided steps go through the tail
    kernel again."""
    from oracle import diffroll_ref as R
    from test_gpu_respaced import hp_of, inputs
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=64, layers=3, k=9)
    p = R.synthetic_params(hp, seed=73)
    wav, x, _ = inputs(3, 40, 73)
    m = project_model(hp, p, "cfdg_ddpm_x0", *PC.MAIN)
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3201, 0), "tune.pw_nw": (2, 0), "tune.stack_fl": (1, 0)}
    for k, (val, _) in pins.items():
        eng.set_option(k, val)
    eng.set_option("fused_stack", 2)                  # (fused regardless: the planner's own choice at this size is per-phase)
    try:
        m.hparams.sampling.cfg_project = None
        m.hparams.sampling.cfg_norm = None
        t0 = eng.tail_launches
        off, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st      # the geometry takes the tail kernel
        m.hparams.sampling.cfg_project = 1.0
        m.hparams.sampling.cfg_norm = 0.05
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack" and eng.tail_launches == t0 and st["fallbacks"] == 0 and st["yields"] == 0, st
        e, _ = m.sample(x, wav, seed=5, use_graph=False)
        assert eng.launch_state()["mode"] == "fused_stack" and eng.tail_launches == t0
        m.hparams.sampling.guidance_interval = [60, 140]
        gi, _ = m.sample(x, wav, seed=5, use_graph=False)
        st = eng.launch_state()
        # 20 visited steps, 8 of them inside [60, 140]: the last steps are unguided and end in the tail kernel
        assert st["mode"] == "fused_stack+tail" and 0 < eng.tail_launches - t0 <= 12 and st["fallbacks"] == 0 and st["yields"] == 0, st
        gig, _ = m.sample(x, wav, seed=5)
        eng.set_option("fused_stack", 0)              # per-phase launches of the pinned flavours: the same bits
        ppi, _ = m.sample(x, wav, seed=5)
        m.hparams.sampling.guidance_interval = None
        pp, _ = m.sample(x, wav, seed=5)
        assert eng.launch_state()["mode"] == "per_phase"
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, val) in pins.items():
            eng.set_option(k, val)
    assert torch.equal(g, e) and torch.equal(g, pp) and not torch.equal(g, off)
    assert torch.equal(gi, gig) and torch.equal(gi, ppi) and not torch.equal(gi, g)
    ref, seen = PR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), PR.CR.philox_noise(5, 0, S, 3, 40), 20,
                                project=PC.MAIN[0], norm=PC.MAIN[1], w=PC.W)
    assert len(seen) == 20
    ok, d = agree(g, ref)
    print(f"\ncfg_project fused geometry w 3 values {PC.MAIN} n 20: max |d| {d:.3e}")
    assert ok, d


# ---------------------------------------------------------------------------------------------- 6. bf16x3 and bf16
def test_split_bf16_vs_restatement():
    hp, p, wav, x, noise = PC.setup()
    m = project_model(hp, p, "cfdg_ddpm_x0", *PC.MAIN, n=8, precision="bf16x3")
    ref, seen = PR.sample_chain(p, hp, "cfdg_ddpm_x0", x, PC.spec_of("cfdg_ddpm_x0"), noise, 8, project=PC.MAIN[0], norm=PC.MAIN[1], w=PC.W)
    assert len(seen) == 8 and all(rho * k >= 0.2 and s <= 0.9 for rows in seen.values() for k, rho, s, _, _ in rows)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\ncfg_project bf16x3 w 3 values {PC.MAIN} n 8: max |d| {d:.3e}")
    assert ok, d


def test_bf16_chain_lies_in_the_restatements_band():
    """tests/test_gpu_bf16.py's chain (8 steps, C = 128, w = 0.5) with rho = 1 and r = 0.05: the rms distance of the bf16 roll
    from the restated fp32 chain lies within 0.5 .. 1.5 x that of the restated bf16 chain - both restatements project."""
    import bf16_ref as Q
    from oracle import diffroll_ref as R
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    kw = dict(project=PC.MAIN[0], norm=PC.MAIN[1], w=0.5)
    ref, seen = PR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, **kw)
    assert len(seen) == Q.CHAIN_STEPS and moved(seen, B)
    with Q.patched(Q.rne, None):
        d_ref = Q.rms(PR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, **kw)[0] - ref)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16")
    m.hparams.sampling.cfg_project = 1.0
    m.hparams.sampling.cfg_norm = 0.05
    got = m.sample(x, wav, noise=nz)[0]
    d = Q.rms(got.cpu() - ref)
    print(f"\ncfg_project bf16 chain: rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (d, d_ref)
    assert torch.equal(m.sample(x, wav, noise=nz)[0], got)
    assert torch.equal(m.sample(x, wav, noise=nz, use_graph=False)[0], got)
    assert m.engine.cfg_project == 10000 and m.engine.cfg_norm == 500
