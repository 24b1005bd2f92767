"""Option "solver_order" on the MI355X (hparams.sampling.solver_order): the HIP chain under the first-order exponential
integrator and DPM-Solver++ (2M) against the CPU restatement of tests/chain_ref.py - four x0 samplers, n in {2, 4, 20},
both precisions - order 1 against the ddim_x0 respaced chain, the fused path at the geometry where the tail kernel's row
tiles recompute the update (graph = eager = per-phase, no history across replays), dr_step over the visited steps, long-form
windows, draws, a guidance interval, and order 0 as the engine that never set the option."""
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import HOP, S, agree, assert_shared_frames_agree, hp_of, inputs, make_model, maxdiff, run_plan_windows

import chain_ref as CR

pytestmark = pytest.mark.gpu


def solver_model(hp, p, sampler, n, order, w=0.5, **kw):
    m = make_model(hp, p, sampler=sampler, w=w, **kw)
    m.hparams.sampling.steps = n
    m.hparams.sampling.solver_order = order
    return m


def test_option_is_public_and_validated():
    hp = hp_of(layers=2)
    p = R.synthetic_params(hp, seed=1)
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    eng.set_option("solver_order", 2)                # DR_ENAME (-> ValueError) before the option existed
    assert eng.solver_order == 2
    for bad in (3, -1):
        with pytest.raises(ValueError, match="solver_order"):
            eng.set_option("solver_order", bad)
    assert eng.solver_order == 2
    eng.set_option("solver_order", 0)
    # an epsilon sampler refuses a non-zero order at the call, naming both
    me = make_model(hp, p, sampler="ddim")
    wav, x, _ = inputs(2, 40, 2)
    me.engine.set_option("solver_order", 2)
    try:
        me._engine.frontend(wav, 40)
        xb = x.squeeze(1).to(me._engine.device).contiguous()
        with pytest.raises(ValueError, match=r"sampler 7 .*solver_order = 2"):
            me._engine.sample("ddim", xb, None)
        with pytest.raises(ValueError, match=r"sampler 7 .*solver_order = 2"):
            me._engine.step("ddim", xb, None, S - 1)
    finally:
        me._engine.set_option("solver_order", 0)
    # ... and the facade refuses it before anything reaches the engine
    me.hparams.sampling.solver_order = 2
    with pytest.raises(ValueError, match="epsilon"):
        me.sample(x, wav)


@pytest.mark.parametrize("sampler", ["ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "cfdg_ddim_x0"])
def test_chain_vs_restatement(sampler):
    """Orders 1 and 2 at n in {2, 4, 20}: n = 4 is the smallest chain with a second-order step."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=70)
    B, Tn = 2, 40
    wav, x, _ = inputs(B, Tn, 71)
    spec = R.frontend(wav, hp, Tn)
    w = 0.5 if sampler.startswith("cfdg") else 0.0
    m = make_model(hp, p, sampler=sampler, w=0.5)
    for order in (1, 2):
        for n in (2, 4, 20):
            m.hparams.sampling.steps, m.hparams.sampling.solver_order = n, order
            ref = CR.sample_chain(p, hp, sampler, x, spec, None, n, order=order, w=w)
            roll, _ = m.sample(x, wav, seed=3)
            ok, d = agree(roll, ref)
            print(f"\n{sampler} order {order} n {n}: max |d| {d:.3e}")
            assert ok, (order, n, d)
            assert m.engine.solver_order == order


def test_split_bf16_vs_restatement():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=72)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2, precision="bf16x3")
    wav, x, _ = inputs(2, 40, 73)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), None, 20, order=2, w=0.5)
    roll, _ = m.sample(x, wav)
    ok, d = agree(roll, ref)
    print(f"\nbf16x3 order 2 n 20: max |d| {d:.3e}")
    assert ok, d


def test_order_1_is_the_ddim_x0_respaced_chain():
    """Two arithmetic routes to the same update: Ap y + sqrt(1 - Ap^2) (x - A y) / Sm and (Smp / Sm) x - Ap expm1(-h) y."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=74)
    wav, x, _ = inputs(2, 40, 75)
    m = make_model(hp, p, sampler="ddim_x0")
    m.hparams.sampling.steps = 20
    ddim, _ = m.sample(x, wav)
    m.hparams.sampling.solver_order = 1
    first, _ = m.sample(x, wav)
    ok, d = agree(first, ddim.cpu())
    print(f"\norder 1 vs ddim_x0 at n = 20: max |d| {d:.3e}")
    assert ok, d
    assert not torch.equal(first, ddim)               # (it IS another route)


def test_fused_path_graph_eager_per_phase_and_no_history_across_replays():
    """16 guided clips x 125 frames at C = 512: four row tiles of the tail kernel's part T3 recompute every update in
    different blocks, and one of them stores the history - the geometry in which an in-place history would race."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=512, layers=3)
    p = R.synthetic_params(hp, seed=11)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, _ = inputs(16, 125, 76)
    x2 = torch.randn(16, 1, 125, 88, generator=torch.Generator().manual_seed(77))
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3202, 0), "tune.pw_nw": (4, 0), "tune.stack_fl": (2, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
        g2, _ = m.sample(x2, wav)                     # the same captured chain, another x_T
        e, _ = m.sample(x, wav, use_graph=False)
        eng.set_option("fused_stack", 0)
        pp, _ = m.sample(x, wav)
        st = eng.launch_state()
        assert st["mode"] == "per_phase" and st["fallbacks"] == 0 and st["yields"] == 0, st
        eng.set_option("fused_stack", 1)
        # a fresh engine's first chain from x2: what g2 must be if nothing of the chain before it leaked into it
        m2 = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
        fresh, _ = m2.sample(x2, wav)
        assert m2.engine.launch_state()["mode"] == "fused_stack+tail"
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
    assert torch.equal(g, e) and torch.equal(g, pp)
    assert torch.equal(g2, fresh) and not torch.equal(g2, g)
    # the restatement of the first and the last clip (clips are independent: the others add CPU time, not coverage)
    sel = [0, 15]
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x[sel], R.frontend(wav[sel], hp, 125), None, 20, order=2, w=0.5)
    ok, d = agree(g[sel], ref)
    print(f"\nfused path order 2 n 20: max |d| {d:.3e}")
    assert ok, d


def test_dr_step_over_the_visited_steps_and_out_of_sequence():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=78)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, _ = inputs(2, 40, 79)
    traj, _ = m.sample_trajectory(x, wav)
    roll, _ = m.sample(x, wav)
    assert traj.shape == (20,) + tuple(roll.shape) and torch.equal(traj[-1], roll)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), None, 20, order=2, w=0.5, trajectory=True)
    d = maxdiff(traj.cpu(), ref)
    print(f"\ntrajectory order 2 n 20: max |d| {d:.3e}")
    assert d <= 1e-5
    # out of sequence: a step that is not the first needs its predecessor's history
    eng = m.engine
    steps = eng.visited_steps()
    xb = x.squeeze(1).to(eng.device).contiguous()
    from diffroll_amd.engine import EngineError
    with pytest.raises(EngineError, match=f"expected next is {steps[0]}"):     # DR_ESTATE (the chain above ended the history)
        eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[3], 0.5)
    eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[0], 0.5)
    eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[1], 0.5)
    with pytest.raises(EngineError, match=f"expected next is {steps[2]}"):
        eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[3], 0.5)
    with pytest.raises(EngineError, match="expected next"):                   # ... of the same sampler
        eng.step("ddpm_x0", xb.clone(), None, steps[2], 0.0)
    eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[0], 0.5)                  # the first step always starts anew
    eng.finish()
    eng.set_option("solver_order", 1)                                          # order 1 keeps no history: any visited step
    eng.step("cfdg_ddpm_x0", xb.clone(), None, steps[3], 0.5)
    eng.finish()
    # the reference's single-step methods keep their own meaning
    m.hparams.sampling.solver_order = 0
    m.hparams.sampling.steps = None
    z = torch.randn(2, 1, 40, 88, generator=torch.Generator().manual_seed(80))
    plain, _ = m.cfdg_ddpm_x0(x, wav, 198, noise=z)
    m.hparams.sampling.solver_order, m.hparams.sampling.steps = 2, 20
    same, _ = m.cfdg_ddpm_x0(x, wav, 198, noise=z)
    assert torch.equal(same, plain)


def test_sample_long_vs_restatement():
    from diffroll_amd import longform
    hp = hp_of(channels=128, layers=3)
    p = R.synthetic_params(hp, seed=81)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    g = torch.Generator().manual_seed(81)
    L = 1400 * HOP - 100
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, None, 20, order=2, w=0.5, plan=plan)
    win = run_plan_windows(m, plan, wav, x_T, None, seed=4, recording=1)
    assert_shared_frames_agree(win, plan)
    ok, d = agree(win, ref[:, 0])
    print(f"\nlong-form order 2 n 20: max |d| {d:.3e}")
    assert ok, d
    roll = m.sample_long(wav, overlap=160, seed=4, recording=1, x_T=x_T).cpu()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.solver_order == 2


def test_draws_equal_the_tiled_batch_bitwise():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=82)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, _, _ = inputs(2, 40, 83)
    x = torch.randn(4, 1, 40, 88, generator=torch.Generator().manual_seed(84))      # 2 draws of 2 clips, draw-major
    got, _ = m.sample(x, wav, draws=2)
    ref, _ = m.sample(x, wav.repeat(2, 1))
    assert torch.equal(got, ref)
    assert not torch.equal(got[:2], got[2:])          # the draws differ - through x_T only


def test_guidance_interval_vs_restatement():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=85)
    m = solver_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    m.hparams.sampling.guidance_interval = [60, 140]
    wav, x, _ = inputs(2, 40, 86)
    spec = R.frontend(wav, hp, 40)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, None, 20, order=2, w=0.5, interval=(60, 140))
    roll, _ = m.sample(x, wav)
    ok, d = agree(roll, ref)
    print(f"\nguidance [60, 140] order 2 n 20: max |d| {d:.3e}")
    assert ok, d
    whole = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, None, 20, order=2, w=0.5)
    assert not agree(roll, whole)[0]                  # (the interval matters at this weight)


def test_order_0_is_the_engine_that_never_set_the_option():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=87)
    wav, x, noise = inputs(2, 40, 88)
    never = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    base, _ = never.sample(x, wav, noise=noise)
    base_p, _ = never.sample(x, wav, seed=6)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.engine.set_option("solver_order", 2)            # ... and back: explicitly 0
    m.engine.set_option("solver_order", 0)
    m.hparams.sampling.solver_order = 0
    got, _ = m.sample(x, wav, noise=noise)
    got_p, _ = m.sample(x, wav, seed=6)
    assert torch.equal(got, base) and torch.equal(got_p, base_p)
    # a chain captured under another order is never replayed, and setting the option back replays the first one
    m.hparams.sampling.solver_order = 2
    second, _ = m.sample(x, wav, noise=noise)
    assert not torch.equal(second, base)
    m.hparams.sampling.solver_order = 0
    again, _ = m.sample(x, wav, noise=noise)
    assert torch.equal(again, base)
