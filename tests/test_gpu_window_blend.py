"""Option "window_blend" on the MI355X (sample_long(..., blend=)): the HIP chains of jointly sampled windows under the linear
cross-fade (1) and the hand-over (2) against the CPU restatement of tests/blend_ref.py - per-phase at three overlaps, with
the other options of the window path, and on the fused path of the shipping geometry (stack kernel + tail kernel) - the byte
identity of mode 0, and the refusals.  Inputs and references: tests/blend_cases.py, which tests/test_window_blend_cpu.py
shows to move with the mode.  Tolerance: ATOL = 1e-5 of the long-form tests."""
import pytest
import torch

from testlib import ATOL, assert_shared_frames_agree, make_model, maxdiff

import blend_cases as BC
import blend_ref as BR
import thresh_ref as TR

from diffroll_amd import longform

pytestmark = pytest.mark.gpu


def one(plan):
    return longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)


def run(m, batch, wavs, x_T, noise, mode, D=1, use_graph=True):
    """sample_long_batch's chain, keeping the windows: (D * n, T, 88) on the host."""
    return m._sample_windows(batch, wavs, x_T, noise, D, 0, 0, use_graph, True, blend=mode).cpu()


# ---------------------------------------------------------------------------------------------- 1. per-phase parity
@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("O", BC.OS)
def test_per_phase_vs_restatement(O, mode):
    hp, p, plan, wav, x_T, noise, _ = BC.case(O)
    ref = BC.reference(O, mode)[:, 0]
    assert float((ref - 0.5).abs().min()) > 10 * ATOL        # (no element of the reference sits at the threshold)
    m = make_model(hp, p, sampler=BC.SAMPLER, w=BC.W)
    eng = m.engine
    eng.set_option("fused_stack", 0)
    graph = run(m, one(plan), [wav], [x_T], [noise], mode)
    eager = run(m, one(plan), [wav], [x_T], [noise], mode, use_graph=False)
    d = maxdiff(graph, ref)
    print(f"\nO {O} mode {mode}: max |d| {d:.3e}")
    assert d <= ATOL, d
    assert torch.equal(graph > 0.5, ref > 0.5)
    assert_shared_frames_agree(graph, plan)
    assert torch.equal(graph, eager), maxdiff(graph, eager)
    assert eng.window_blend == 0 and eng.window_overlap == 0          # held for the call only


# ---------------------------------------------------------------------------------------------- 2. mode 0
def test_mode_0_is_byte_identical_and_replays_the_captured_chain():
    """Mode 0 set explicitly: the bits of an engine that never set the option, from the chain that engine captured.  A mode
    that changes the arithmetic is part of the key (control), and is inert - replays - while "window_overlap" is 0."""
    O = 5
    hp, p, plan, wav, x_T, noise, _ = BC.case(O)
    S = int(hp["timesteps"])
    never = run(make_model(hp, p, sampler=BC.SAMPLER, w=BC.W), one(plan), [wav], [x_T], [noise], 0)
    m = make_model(hp, p, sampler=BC.SAMPLER, w=BC.W)
    eng = m.engine
    eng.frontend(longform.window_audio(wav, plan, BC.HOP), plan.T)
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).to(eng.device)
    z = longform.gather_windows(noise.reshape(S, plan.T_c, 88), plan).to(eng.device).contiguous()

    def chain(x=xw, zz=z):
        xb = x.clone()
        eng.sample(BC.SAMPLER, xb, zz, BC.W, 0, 0, True, True)
        st = eng.launch_state()
        return xb.cpu(), (eng.cold_times()[3], eng.launch_counts(), st["stack_launches"], st["tail_launches"])

    eng.set_option("window_overlap", O)
    try:
        first, c0 = chain()
        assert torch.equal(first, never)
        eng.set_option("window_blend", 0)
        again, c1 = chain()
        assert torch.equal(again, first) and c1 == c0, (c0, c1)      # replayed: no capture, no launch counted
        eng.set_option("window_blend", 1)
        moved, c2 = chain()
        assert c2 != c0 and maxdiff(moved, first) > 100 * ATOL       # part of the key, and it blends
        eng.set_option("window_blend", 0)
        assert torch.equal(chain()[0], first)
    finally:
        eng.set_option("window_blend", 0)
        eng.set_option("window_overlap", 0)
    # independent clips: the value is inert
    clips, k0 = chain()
    eng.set_option("window_blend", 2)
    try:
        same, k1 = chain()
    finally:
        eng.set_option("window_blend", 0)
    assert torch.equal(same, clips) and k1 == k0, (k0, k1)
    assert not torch.equal(clips, first)


# ---------------------------------------------------------------------------------------------- 3. with the other options
@pytest.mark.parametrize("mode", BC.MODES)
def test_window_break_blends_per_recording(mode):
    a, b = BC.break_case()
    batch = longform.BatchPlan(plans=[a[2], b[2]], first=[0, 2], marks=[2], n=3)
    m = make_model(a[0], a[1], sampler=BC.SAMPLER, w=BC.W)
    m.engine.set_option("fused_stack", 0)
    got = run(m, batch, [a[3], b[3]], [a[4], b[4]], [a[5], b[5]], mode)
    ref = BC.break_reference(mode)[:, 0]
    d = maxdiff(got, ref)
    print(f"\nwindow_break mode {mode}: max |d| {d:.3e}")
    assert d <= ATOL, d
    H = a[2].stride
    assert torch.equal(got[0, H:], got[1, :BC.OPT_O]) and not torch.equal(got[1, H:], got[2, :BC.OPT_O])


@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("name", list(BC.OPTION_CASES))
def test_option_cases_vs_restatement(name, mode):
    kw = BC.OPTION_CASES[name]
    S, D = kw.get("timesteps", 4), kw.get("draws", 1)
    hp, p, plan, wav, _, _, _ = BC.recording(BC.OPT_O, 3300, S)
    x_T, noise = BC.option_canvases(name)
    m = make_model(hp, p, sampler=BC.SAMPLER, w=kw.get("w", BC.W))
    samp = m.hparams.sampling
    if "order" in kw:
        samp.solver_order, samp.steps = kw["order"], kw["steps"]
        if kw.get("solver_noise"):
            samp.solver_noise = 1
    if "code" in kw:
        samp.x0_clip = kw["code"]
    m.engine.set_option("fused_stack", 0)
    got = run(m, one(plan), [wav], [x_T], [noise], mode, D=D)
    ref = BC.option_reference(name, mode)[:, 0]
    d = maxdiff(got, ref)
    print(f"\n{name} mode {mode}: max |d| {d:.3e}")
    assert d <= ATOL, d
    for k in range(D):                                # "draws" blends per draw
        assert_shared_frames_agree(got[k * plan.n:(k + 1) * plan.n], plan)
    assert maxdiff(got, BC.option_reference(name, 0)[:, 0]) > 100 * ATOL      # the mode matters beside the option


@pytest.mark.parametrize("mode", BC.MODES)
def test_threshold_ranks_and_updates_the_blended_prediction(mode):
    w, code, v = BC.THRESH["w"], BC.THRESH["code"], BC.THRESH["v"]
    hp, p, plan, wav, x_T, noise, _ = BC.recording(BC.OPT_O, 3300)
    ref, stats, r = BC.thresh_reference(mode)
    assert all(TR.active(stats, r))                   # the inputs threshold at every step
    m = make_model(hp, p, sampler=BC.SAMPLER, w=w)
    m.hparams.sampling.x0_clip = 1
    m.hparams.norm_args[0:2] = [-1.0, 1.0]            # the range of code 2
    m.hparams.sampling.x0_threshold = v / 10000.0
    got = run(m, one(plan), [wav], [x_T], [noise], mode)
    assert m.engine.x0_clip == code and m.engine.x0_threshold == v
    d = maxdiff(got, ref[:, 0])
    print(f"\nx0_threshold mode {mode}: max |d| {d:.3e}")
    assert d <= ATOL, d
    assert_shared_frames_agree(got, plan)
    # the selection of one step, bit for bit: q and s of the recording's canvas over the BLENDED prediction
    eng = m._engine
    O, T = BC.OPT_O, plan.T
    groups = TR.window_groups(plan.n, O)
    g = torch.Generator().manual_seed(11 + mode)
    c, u = 1.2 * torch.randn(plan.n, T, 88, generator=g), torch.randn(plan.n, T, 88, generator=g)
    y = BR.blend_groups((1 + w) * c - w * u, groups, T - O, O, mode)
    want = TR.group_stats(y, code, v, groups)
    mean = TR.group_stats(BR.blend_groups((1 + w) * c - w * u, groups, T - O, O, 0), code, v, groups)
    assert not torch.equal(want, mean)                # (the mean's q is another number: the check below tells them apart)
    for name, value in (("x0_clip", code), ("x0_threshold", v), ("window_overlap", O), ("window_blend", mode)):
        eng.set_option(name, value)
    try:
        stat = eng.threshold_stats(c, u, w, groups=len(groups)).cpu()
    finally:
        for name in ("window_blend", "window_overlap", "x0_threshold", "x0_clip"):
            eng.set_option(name, 0)
    assert torch.equal(stat.view(torch.int32), want.view(torch.int32)), (stat.tolist(), want.tolist())


def test_a_change_of_the_value_ends_a_dr_step_history():
    from diffroll_amd.engine import EngineError
    hp, p, plan, _, _, _, _ = BC.recording(BC.OPT_O, 3300, 8)
    eng = make_model(hp, p, sampler="generation_ddpm_x0").engine
    eng.set_option("solver_order", 2)
    eng.set_option("window_overlap", BC.OPT_O)
    x = torch.randn(plan.n, plan.T, 88, device=eng.device)
    try:
        eng.step("generation_ddpm_x0", x, None, 7)
        eng.step("generation_ddpm_x0", x, None, 6)
        eng.set_option("window_blend", 1)
        with pytest.raises(EngineError, match="continues no history"):
            eng.step("generation_ddpm_x0", x, None, 5)
        eng.step("generation_ddpm_x0", x, None, 7)
        eng.step("generation_ddpm_x0", x, None, 6)
        eng.set_option("window_blend", 1)             # the same value: nothing ends
        eng.step("generation_ddpm_x0", x, None, 5)
    finally:
        eng.set_option("window_blend", 0)
        eng.set_option("window_overlap", 0)
        eng.set_option("solver_order", 0)
    eng.finish()


# ---------------------------------------------------------------------------------------------- 4. the fused path
def test_fused_path_equals_per_phase_and_keeps_the_tail_kernel():
    """T = 640, O = 160, three windows: the 160-frame stack flavour and the tail kernel, whose part T3 blends."""
    hp, p, plan, wav, x_T, noise, _ = BC.fused_case()
    m = make_model(hp, p, sampler=BC.SAMPLER, w=BC.W)
    eng = m.engine
    # (the pins of tests/test_gpu_longform.py: only then are the two launch modes the same arithmetic; process-wide: restored)
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3205, 0), "tune.pw_nw": (5, 0), "tune.stack_fl": (5, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        for mode in BC.MODES:
            ref = BC.fused_reference(mode)[:, 0]
            eng.set_option("fused_stack", 0)
            pp = run(m, one(plan), [wav], [x_T], [noise], mode)
            eng.set_option("fused_stack", 2)
            t0 = eng.tail_launches
            fe = run(m, one(plan), [wav], [x_T], [noise], mode, use_graph=False)
            st = eng.launch_state()
            assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
            fg = run(m, one(plan), [wav], [x_T], [noise], mode)
            st = eng.launch_state()
            assert st["mode"] == "fused_stack+tail" and st["fallbacks"] == 0 and st["yields"] == 0, st
            d = maxdiff(fe, ref)
            print(f"\nfused mode {mode}: max |d| {d:.3e}")
            assert d <= ATOL, d
            assert torch.equal(fe, pp), maxdiff(fe, pp)               # fused == per-phase, bit for bit
            assert torch.equal(fg, fe), maxdiff(fg, fe)               # graph == eager
            assert_shared_frames_agree(fg, plan)
            roll = m.sample_long(wav, overlap=plan.overlap, x_T=x_T, noise=noise, blend={1: "linear", 2: "nearest"}[mode]).cpu()
            assert torch.equal(roll[0, 0], longform.stitch(fg, plan))     # the façade's names reach the same chain
    finally:
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
        eng.set_option("fused_stack", 1)
    assert eng.window_blend == 0 and eng.window_overlap == 0


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    hp, p, plan, wav, x_T, _, _ = BC.case(5)
    m = make_model(hp, p, sampler=BC.SAMPLER, w=BC.W)
    eng = m.engine
    for bad in (3, -1):
        with pytest.raises(ValueError, match=f"window_blend.*{bad}"):
            eng.set_option("window_blend", bad)
    assert eng.window_blend == 0
    eng.set_option("window_blend", 2)                 # DR_ENAME (-> ValueError) before the option existed
    eng.set_option("window_blend", 0)
    for bad in ("cosine", 3, True):
        with pytest.raises(ValueError, match="window blend"):
            m.sample_long(wav, overlap=5, blend=bad)
        with pytest.raises(ValueError, match="window blend"):
            m.sample_long_batch([wav], overlap=5, blend=bad)
