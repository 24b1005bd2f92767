"""Option "x0_threshold" on the MI355X (hparams.sampling.x0_threshold): the selection kernels alone, bit for bit against the
CPU restatement of tests/thresh_ref.py (dr_debug_threshold: every shape class, percentile, range, tie / zero / inf / NaN
input, window grouping; twice, so the work words are shown to re-arm), then the HIP chains against the restated chain -
samplers x weights x lengths, injected noise and the replayed Philox draws, eager = captured - the inert identity with the
"x0_clip" chain, the other options, the fused geometry (the step leaves the tail kernel and comes back), long-form windows
(one q per recording's canvas) and the refusals.  The inputs and references are those of tests/thresh_cases.py, which
tests/test_x0_threshold_cpu.py shows to be active or inert as claimed.  Tolerance: agree / ATOL of the "x0_clip" tests."""
import pytest
import torch

from testlib import ATOL, S, agree, assert_shared_frames_agree, kernel_inputs, make_model, maxdiff, run_plan_windows, same_bits

import chain_ref as CR
import clip_cases as CC
import clip_ref as CL
import thresh_cases as TC
import thresh_ref as TR

pytestmark = pytest.mark.gpu

VS = (5000, 9000, 9950, 9999, 10000)


def thresh_model(hp, p, sampler, w, code, v, n=20, **kw):
    """The facade with hparams.sampling.x0_clip and .x0_threshold on and hparams.norm_args naming the range of `code`."""
    options = {k: kw.pop(k) for k in ("solver_order", "solver_noise", "guidance_interval", "strength") if k in kw}
    m = make_model(hp, p, sampler=sampler, w=w, **kw)
    m.hparams.sampling.steps = n or None
    m.hparams.sampling.x0_clip = 1
    m.hparams.norm_args[0:2] = list(CL.BOUNDS[code])
    m.hparams.sampling.x0_threshold = v / 10000.0 if v else None
    for k, val in options.items():
        setattr(m.hparams.sampling, k, val)
    return m


def guided(n=20, **kw):
    """The guided active case of thresh_cases: cfdg_ddpm_x0 at w = 3, code 2, v = 9950 on the shared inputs."""
    hp, p, wav, x, noise, _ = CC.setup()
    s, w, code, v = TC.GUIDED
    return thresh_model(hp, p, s, w, code, v, n, **kw), wav, x, noise


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def lab():
    """A committed engine whose options the kernel tests set; handed back with every one of them off."""
    hp, p, _, _, _, _ = CC.setup()
    eng = make_model(hp, p, sampler="generation_ddpm_x0").engine
    yield eng
    for name, value in (("window_overlap", 0), ("window_break", 0), ("draws", 1), ("x0_threshold", 0), ("x0_clip", 0)):
        eng.set_option(name, value)


def guided_y(c, u, w):
    return c if u is None else (1 + w) * c - w * u


@pytest.mark.parametrize("B,T", [(1, 1), (3, 3), (2, 40), (16, 125), (1, 640)])
def test_selection_is_bit_equal_to_the_restatement(lab, B, T):
    worst = 0
    for name, c in kernel_inputs(B, T, 17 + T).items():
        # guided at w = 3: normal noise as the unconditional prediction, a constant beside the special inputs (it keeps
        # them all-equal / two-valued / inf / NaN through (1 + w) c - w u)
        for u in (None, torch.randn(B, T, 88, generator=torch.Generator().manual_seed(T)) if name == "noise" else torch.full((B, T, 88), 0.25)):
            y = guided_y(c, u, 3.0)
            for code in (1, 2):
                lab.set_option("x0_clip", code)
                for v in VS:
                    lab.set_option("x0_threshold", v)
                    want = TR.group_stats(y, code, v, TR.clip_groups(B))
                    got = lab.threshold_stats(c, u, 3.0)
                    again = lab.threshold_stats(c, u, 3.0)
                    assert same_bits(got, want), (name, u is not None, code, v, got.cpu().tolist()[:3], want.tolist()[:3])
                    assert same_bits(again, got), (name, code, v)
                    worst += int((want[:, 1] > TR.centre(code)[1]).sum())
    assert worst > 0                                  # (some of these groups threshold: s > r)


@pytest.mark.parametrize("T", [744, 745])
def test_selection_either_side_of_the_form_switch(lab, T):
    """T * 88 = 65472 / 65560 elements: the last roll of the one-workgroup form and the first of the multi-launch form."""
    g = torch.Generator().manual_seed(T)
    c, u = 1.2 * torch.randn(2, T, 88, generator=g), torch.randn(2, T, 88, generator=g)
    lab.set_option("x0_clip", 2)
    for v in (9000, 9950, 10000):
        lab.set_option("x0_threshold", v)
        want = TR.group_stats(guided_y(c, u, 3.0), 2, v, TR.clip_groups(2))
        got = lab.threshold_stats(c, u, 3.0)
        assert same_bits(got, want) and same_bits(lab.threshold_stats(c, u, 3.0), want), (v, got.cpu().tolist(), want.tolist())


@pytest.mark.parametrize("marks,draws", [((), 1), ((2,), 1), ((2,), 2)], ids=["one-recording", "mark-at-2", "mark-at-2-draws-2"])
def test_selection_over_window_canvases(lab, marks, draws):
    """(B, T, O) = (3, 8, 2): one recording; a mark at 2 - two recordings, G = 2; the same with draws = 2 on B = 6, G = 4."""
    T, O = 8, 2
    B = 3 * draws
    groups = TR.window_groups(B, O, marks, draws)
    g = torch.Generator().manual_seed(5 + B + len(marks))
    inputs = kernel_inputs(B, T, 23)
    try:
        lab.set_option("window_overlap", O)
        lab.set_window_breaks(marks)
        lab.set_option("draws", draws)
        for name in ("noise", "two", "specials", "one_nan"):
            c = inputs[name]
            for u in (None, torch.randn(B, T, 88, generator=g)):
                y = TR.shared_mean(guided_y(c, u, 3.0), groups, T - O, O)
                for code in (1, 2):
                    lab.set_option("x0_clip", code)
                    for v in VS:
                        lab.set_option("x0_threshold", v)
                        want = TR.group_stats(y, code, v, groups)
                        got = lab.threshold_stats(c, u, 3.0, groups=len(groups))
                        assert same_bits(got, want), (name, u is not None, code, v, got.cpu().tolist(), want.tolist())
                        assert same_bits(lab.threshold_stats(c, u, 3.0, groups=len(groups)), got), (name, code, v)
    finally:
        lab.set_option("draws", 1)
        lab.set_window_breaks(())
        lab.set_option("window_overlap", 0)


# ---------------------------------------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("sampler,w,code,v,n", TC.CASES, ids=TC.CASE_IDS)
def test_chain_vs_restatement(sampler, w, code, v, n):
    hp, p, wav, x, noise, _ = CC.setup()
    m = thresh_model(hp, p, sampler, w, code, v, n)
    for philox, kw in ((False, dict(noise=noise)), (True, dict(seed=CC.PHILOX_SEED))):
        ref = TC.assert_active(sampler, w, code, v, n, philox)       # (the inputs threshold, before the engine's roll is looked at)
        roll, _ = m.sample(x, wav, **kw)
        eager, _ = m.sample(x, wav, use_graph=False, **kw)
        assert torch.equal(roll, eager), (philox, maxdiff(roll.cpu(), eager.cpu()))
        ok, d = agree(roll, ref)
        print(f"\n{sampler} w {w} code {code} v {v} n {n or S} {'philox' if philox else 'injected'}: max |d| {d:.3e}")
        assert ok, (philox, d)
    assert m.engine.x0_threshold == v and m.engine.x0_clip == code
    assert m.engine.launch_state()["mode"] != "fused_stack+tail"


# ---------------------------------------------------------------------------------------------- 3. inert identity
@pytest.mark.parametrize("w,v", [(0.5, 9950), (3.0, 9000)])
def test_an_inert_chain_is_the_clipped_chain_bitwise(w, v):
    hp, p, wav, x, noise, _ = CC.setup()
    TC.assert_inert("cfdg_ddpm_x0", w, 2, v, 20)
    m = thresh_model(hp, p, "cfdg_ddpm_x0", w, 2, v, 20)
    for kw in (dict(noise=noise), dict(seed=CC.PHILOX_SEED)):
        on, _ = m.sample(x, wav, **kw)
        assert m.engine.x0_threshold == v
        m.hparams.sampling.x0_threshold = None
        clipped, _ = m.sample(x, wav, **kw)
        assert m.engine.x0_threshold == 0 and m.engine.x0_clip == 2
        m.hparams.sampling.x0_threshold = v / 10000.0
        assert torch.equal(on, clipped), maxdiff(on.cpu(), clipped.cpu())
    if w == 3.0:                                      # ... while the active percentile moves the roll
        m.hparams.sampling.x0_threshold = 0.995
        active, _ = m.sample(x, wav, noise=noise)
        m.hparams.sampling.x0_threshold = None
        clipped, _ = m.sample(x, wav, noise=noise)
        assert maxdiff(active.cpu(), clipped.cpu()) >= 100 * ATOL


# ---------------------------------------------------------------------------------------------- 4. with the other options
@pytest.mark.parametrize("name,kw", TC.OPTION_CASES, ids=[c[0] for c in TC.OPTION_CASES])
def test_solver_orders_and_interval_vs_restatement(name, kw):
    facade = dict(kw)
    if "order" in facade:
        facade["solver_order"] = facade.pop("order")
    if "interval" in facade:
        facade["guidance_interval"] = list(facade.pop("interval"))
    m, wav, x, noise = guided(**facade)
    ref = TC.assert_active(*TC.GUIDED, 20, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\n{name} w 3 code 2 v 9950 n 20: max |d| {d:.3e}")
    assert ok, d
    assert not agree(roll, TC.reference(*TC.GUIDED, 20)[0])[0]       # the option beside the threshold matters on these inputs


def test_split_bf16_vs_restatement():
    m, wav, x, noise = guided(precision="bf16x3")
    ref = TC.assert_active(*TC.GUIDED, 20)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\nbf16x3 w 3 code 2 v 9950 n 20: max |d| {d:.3e}")
    assert ok, d


@pytest.mark.parametrize("order", [0, 2])
def test_resume_draws_and_dr_step_bitwise(order):
    m, wav, x, noise = guided(solver_order=order)
    kw = dict(seed=0x1234567890AB, first_sample=3)
    traj, _ = m.sample_trajectory(x, wav, **kw)       # dr_step over the visited steps
    whole, _ = m.sample(x, wav, **kw)
    assert traj.shape == (20,) + tuple(whole.shape) and torch.equal(whole, traj[-1])
    if order == 0:                                    # (a resumed order-2 chain starts a new history: another chain)
        visited = m.visited_steps()
        for i in (0, 9, 18):
            m.hparams.sampling.start_step = visited[i + 1]
            roll, _ = m.sample(traj[i], wav, **kw)
            assert m.engine.start_step == visited[i + 1] and m.engine.x0_threshold == 9950
            assert torch.equal(roll, traj[-1]), (i, maxdiff(roll.cpu(), traj[-1].cpu()))
        m.hparams.sampling.start_step = None
    x2 = x.repeat(2, 1, 1, 1)                         # 2 draws of 2 clips: every draw is a roll - a group - of its own
    got, _ = m.sample(x2, wav, seed=7, draws=2)
    ref, _ = m.sample(x2, wav.repeat(2, 1), seed=7)
    assert torch.equal(got, ref)
    assert torch.equal(got[:2], got[2:]) == (order == 2)             # (the deterministic solver draws nothing: its draws are one roll)


def test_a_change_of_the_value_ends_a_dr_step_history():
    from diffroll_amd.engine import EngineError
    hp, p, _, _, _, _ = CC.setup()
    eng = make_model(hp, p, sampler="generation_ddpm_x0").engine
    eng.set_option("sampling_steps", 20)
    eng.set_option("solver_order", 2)
    eng.set_option("x0_clip", 1)
    v = eng.visited_steps()
    x = torch.randn(CC.B, CC.TN, 88, device=eng.device)

    def step(t):
        eng.step("generation_ddpm_x0", x, None, t)

    step(v[0])
    step(v[1])
    eng.set_option("x0_threshold", 9950)
    with pytest.raises(EngineError, match="continues no history"):
        step(v[2])
    step(v[0])
    step(v[1])
    eng.set_option("x0_threshold", 9950)              # the same value: nothing ends
    step(v[2])
    eng.set_option("x0_threshold", 9000)
    with pytest.raises(EngineError, match="continues no history"):
        step(v[3])
    eng.finish()


# ---------------------------------------------------------------------------------------------- 5. the fused geometry
def test_fused_geometry_leaves_the_tail_kernel_and_comes_back():
    """16 guided clips x 125 frames at C = 512: with the option on a step keeps its fused stack launch and runs the head
    projections, the selection and the update as ordinary launches; set back to 0, the next chain is the parent's."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp, p, wav, x = CC.fused_case()
    m = thresh_model(hp, p, "cfdg_ddpm_x0", 3.0, 2, 9950, 20, solver_order=2, solver_noise=1)
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3202, 0), "tune.pw_nw": (4, 0), "tune.stack_fl": (2, 0)}
    for k, (val, _) in pins.items():
        eng.set_option(k, val)
    try:
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack" and eng.tail_launches == t0, st
        e, _ = m.sample(x, wav, seed=5, use_graph=False)
        assert eng.launch_state()["mode"] == "fused_stack" and eng.tail_launches == t0
        m.hparams.sampling.x0_threshold = None        # back to 0: the clipped chain, through the tail kernel
        off, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert eng.x0_threshold == 0 and st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
        m.hparams.sampling.x0_threshold = 0.995
        again, _ = m.sample(x, wav, seed=5)
        m2 = thresh_model(hp, p, "cfdg_ddpm_x0", 3.0, 2, 0, 20, solver_order=2, solver_noise=1)      # never set the option
        for k, (val, _) in pins.items():
            m2.engine.set_option(k, val)
        never, _ = m2.sample(x, wav, seed=5)
        assert m2.engine.launch_state()["mode"] == "fused_stack+tail" and m2.engine.x0_threshold == 0
    finally:
        for k, (_, val) in pins.items():
            eng.set_option(k, val)
    assert torch.equal(g, e) and torch.equal(g, again)
    assert torch.equal(off, never) and not torch.equal(off, g)
    ref, stats, r = TC.fused_reference()
    assert all(TR.active(stats, r))
    ok, d = agree(g[CC.FUSED_SEL], ref)
    print(f"\nfused geometry w 3 code 2 v 9950 stochastic order 2 n 20: max |d| {d:.3e}")
    assert ok, d


# ---------------------------------------------------------------------------------------------- 6. long form
def test_sample_long_vs_the_per_canvas_restatement():
    from diffroll_amd import longform
    hp, p, plan, wav, x_T = CC.long_case()
    ref, stats, r = TC.long_reference()
    assert all(TR.active(stats, r))
    m = thresh_model(hp, p, "cfdg_ddpm_x0", 3.0, 2, 9950, 20)
    win = run_plan_windows(m, plan, wav, x_T, None, seed=CC.LONG_SEED, recording=CC.LONG_REC)
    assert_shared_frames_agree(win, plan)             # all windows of the recording use the same s on the same mean
    ok, d = agree(win, ref[:, 0])
    print(f"\nlong-form w 3 code 2 v 9950 n 20: max |d| {d:.3e}")
    assert ok, d
    eager = run_plan_windows(m, plan, wav, x_T, None, seed=CC.LONG_SEED, recording=CC.LONG_REC, use_graph=False)
    assert torch.equal(win, eager)
    roll = m.sample_long(wav, overlap=160, seed=CC.LONG_SEED, recording=CC.LONG_REC, x_T=x_T).cpu()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.x0_threshold == 9950


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    hp, p, wav, x, _, _ = CC.setup()
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    assert eng.x0_threshold == 0
    for bad in (4999, 10001, -1):
        with pytest.raises(ValueError, match=f"x0_threshold.*{bad}"):
            eng.set_option("x0_threshold", bad)
    assert eng.x0_threshold == 0
    eng.set_option("x0_threshold", 9950)              # DR_ENAME (-> ValueError) before the option existed
    xb = x.squeeze(1).to(eng.device).contiguous()
    try:
        for call in (lambda: eng.sample("generation_ddpm_x0", xb, None), lambda: eng.sample("generation_ddpm_x0", xb, None, use_graph=False),
                     lambda: eng.step("generation_ddpm_x0", xb, None, S - 1), lambda: eng.threshold_stats(xb)):
            with pytest.raises(ValueError, match=r"x0_threshold = 9950 needs x0_clip"):
                call()
        eng.set_option("x0_clip", 1)
        eng.step("generation_ddpm_x0", xb, None, S - 1)          # ... and runs with both
    finally:
        eng.set_option("x0_threshold", 0)
        eng.set_option("x0_clip", 0)
    eng.finish()
    me = make_model(hp, p, sampler="ddim")
    ee = me.engine                                    # (the property puts the hparams' values back at every use)
    ee.set_option("x0_clip", 1)
    ee.set_option("x0_threshold", 9000)
    try:
        me._engine.frontend(wav, CC.TN)
        for call in (lambda: me._engine.sample("ddim", xb, None), lambda: me._engine.step("ddim", xb, None, S - 1)):
            with pytest.raises(ValueError, match=r"sampler 7 .*x0_clip = 1.*x0_threshold = 9000"):
                call()
    finally:
        me._engine.set_option("x0_threshold", 0)
        me._engine.set_option("x0_clip", 0)
    me.hparams.sampling.x0_clip = 1
    me.hparams.sampling.x0_threshold = 0.995
    with pytest.raises(ValueError, match="epsilon"):
        me.sample(x, wav)
