"""Option "solver_noise" on the MI355X (hparams.sampling.solver_noise): the HIP chain under the stochastic first-order
solver and stochastic DPM-Solver++ (2M) against the CPU restatement of tests/chain_ref.py - four x0 samplers,
n in {2, 4, 20}, injected noise and the replayed Philox draws, both precisions - order 1 against the ddpm_x0 respaced chain,
the fused path at the geometry where the tail kernel's row tiles recompute the update (graph = eager = per-phase, neither
seed nor history across replays), seeds, long-form windows, draws, a guidance interval, a resumed chain, dr_step over the
visited steps, sharding, and the option at 0 as the engine that never set it."""
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import HOP, S, agree, assert_shared_frames_agree, hp_of, inputs, make_model, maxdiff, run_plan_windows

import chain_ref as CR

pytestmark = pytest.mark.gpu


def noisy_model(hp, p, sampler, n, order, w=0.5, **kw):
    m = make_model(hp, p, sampler=sampler, w=w, **kw)
    m.hparams.sampling.steps = n
    m.hparams.sampling.solver_order = order
    m.hparams.sampling.solver_noise = 1
    return m


def test_option_is_public_and_validated():
    hp = hp_of(layers=2)
    p = R.synthetic_params(hp, seed=1)
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    assert eng.solver_noise == 0
    eng.set_option("solver_noise", 1)                # DR_ENAME (-> ValueError) before the option existed
    assert eng.solver_noise == 1
    for bad in (2, -1):
        with pytest.raises(ValueError, match="solver_noise"):
            eng.set_option("solver_noise", bad)
    assert eng.solver_noise == 1
    # stored always, inert while "solver_order" is 0: the sampler's own chain, bit for bit (the engine, not the facade,
    # which refuses the key without an order)
    x = torch.randn(2, 40, 88, device=eng.device)
    on = eng.sample("generation_ddpm_x0", x.clone(), None, seed=3)
    eng.set_option("solver_noise", 0)
    off = eng.sample("generation_ddpm_x0", x.clone(), None, seed=3)
    assert torch.equal(on, off)
    # the facade refuses a value without an order, and an epsilon sampler, before anything reaches the engine
    m.hparams.sampling.solver_noise = 1
    with pytest.raises(ValueError, match="solver_order"):
        m.sample(x.unsqueeze(1).cpu())
    me = make_model(hp, p, sampler="ddim")
    me.hparams.sampling.solver_noise = 1
    wav, xe, _ = inputs(2, 40, 2)
    with pytest.raises(ValueError, match="epsilon"):
        me.sample(xe, wav)


@pytest.mark.parametrize("sampler", ["ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "cfdg_ddim_x0"])
def test_chain_vs_restatement(sampler):
    """Orders 1 and 2 at n in {2, 4, 20} (n = 4 is the smallest chain with a second-order step), with injected noise and
    with Philox replayed on the CPU."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=70)
    B, Tn = 2, 40
    wav, x, noise = inputs(B, Tn, 71)
    spec = R.frontend(wav, hp, Tn)
    w = 0.5 if sampler.startswith("cfdg") else 0.0
    m = noisy_model(hp, p, sampler, 2, 1)
    zp = CR.philox_noise(9, 0, S, B, Tn)
    for order in (1, 2):
        for n in (2, 4, 20):
            m.hparams.sampling.steps, m.hparams.sampling.solver_order = n, order
            for z, kw in ((noise, dict(noise=noise)), (zp, dict(seed=9))):
                ref = CR.sample_chain(p, hp, sampler, x, spec, z, n, order=order, solver_noise=1, w=w)
                roll, _ = m.sample(x, wav, **kw)
                ok, d = agree(roll, ref)
                print(f"\n{sampler} order {order} n {n} {'injected' if 'noise' in kw else 'philox'}: max |d| {d:.3e}")
                assert ok, (order, n, kw.keys(), d)
            assert m.engine.solver_noise == 1 and m.engine.solver_order == order


def test_split_bf16_vs_restatement():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=72)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2, precision="bf16x3")
    wav, x, noise = inputs(2, 40, 73)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), noise, 20, order=2, solver_noise=1, w=0.5)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\nbf16x3 order 2 n 20: max |d| {d:.3e}")
    assert ok, d


def test_order_1_is_the_ddpm_x0_respaced_chain():
    """Two arithmetic routes to the same update: (Ap y + (dir (x - A y)) / Sm) + sigma z and ((Smp / Sm) exp(-h) x +
    Ap (1 - exp(-2h)) y) + Smp sqrt(1 - exp(-2h)) z.  Their fp32 restatements, evaluated on the CPU for these very inputs
    before any GPU run, differ by max |d| = 4.3e-07 (ddpm_x0; 7.7e-07 under cfdg_ddpm_x0, w = 0.5) on rolls of |x| <= 0.26 -
    well inside ATOL / 2 = 5e-06 - so the two GPU chains are held to each other directly."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=74)
    wav, x, noise = inputs(2, 40, 75)
    m = make_model(hp, p, sampler="ddpm_x0")
    m.hparams.sampling.steps = 20
    ddpm, _ = m.sample(x, wav, noise=noise)
    m.hparams.sampling.solver_order, m.hparams.sampling.solver_noise = 1, 1
    first, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(first, ddpm.cpu())
    print(f"\nstochastic order 1 vs ddpm_x0 at n = 20: max |d| {d:.3e}")
    assert ok, d
    assert not torch.equal(first, ddpm)               # (it IS another route)


def test_fused_path_graph_eager_per_phase_and_nothing_across_replays():
    """16 guided clips x 125 frames at C = 512: four row tiles of the tail kernel's part T3 recompute every update - and now
    every Philox draw - in different blocks, and one of them stores the history."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=512, layers=3)
    p = R.synthetic_params(hp, seed=11)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, _ = inputs(16, 125, 76)
    x2 = torch.randn(16, 1, 125, 88, generator=torch.Generator().manual_seed(77))
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3202, 0), "tune.pw_nw": (4, 0), "tune.stack_fl": (2, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
        g2, _ = m.sample(x2, wav, seed=6)             # the same captured chain, another seed and x_T
        e, _ = m.sample(x, wav, seed=5, use_graph=False)
        eng.set_option("fused_stack", 0)
        pp, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "per_phase" and st["fallbacks"] == 0 and st["yields"] == 0, st
        eng.set_option("fused_stack", 1)
        # a fresh engine's first chain from x2 and seed 6: what g2 must be if neither seed nor history leaked into it
        m2 = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
        fresh, _ = m2.sample(x2, wav, seed=6)
        assert m2.engine.launch_state()["mode"] == "fused_stack+tail"
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
    assert torch.equal(g, e) and torch.equal(g, pp)
    assert torch.equal(g2, fresh) and not torch.equal(g2, g)
    # the restatement of the first and the last clip (clips are independent: the others add CPU time, not coverage)
    sel = [0, 15]
    z = CR.philox_rows(5, sel, S, 20, 125)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x[sel], R.frontend(wav[sel], hp, 125), z, 20, order=2, solver_noise=1, w=0.5)
    ok, d = agree(g[sel], ref)
    print(f"\nfused path stochastic order 2 n 20: max |d| {d:.3e}")
    assert ok, d


def test_seeds():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=78)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, _ = inputs(2, 40, 79)
    a, _ = m.sample(x, wav, seed=11)
    b, _ = m.sample(x, wav, seed=12)
    a2, _ = m.sample(x, wav, seed=11)
    assert torch.equal(a, a2) and not torch.equal(a, b)            # the same x_T: the draws alone tell the rolls apart
    a3, _ = m.sample(x, wav, seed=11, first_sample=1)
    assert not torch.equal(a, a3)                                  # ... and so does the batch offset
    e, _ = m.sample(x, wav, seed=11, use_graph=False)
    assert torch.equal(e, a)


def test_option_at_0_is_the_engine_that_never_set_it():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=87)
    wav, x, noise = inputs(2, 40, 88)
    for order in (0, 1, 2):
        never = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
        never.hparams.sampling.steps, never.hparams.sampling.solver_order = 20, order
        base, _ = never.sample(x, wav, noise=noise)
        base_p, _ = never.sample(x, wav, seed=6)
        m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
        m.hparams.sampling.steps, m.hparams.sampling.solver_order = 20, order
        m.engine.set_option("solver_noise", 1)        # ... and back: explicitly 0
        m.engine.set_option("solver_noise", 0)
        m.hparams.sampling.solver_noise = 0
        got, _ = m.sample(x, wav, noise=noise)
        got_p, _ = m.sample(x, wav, seed=6)
        assert torch.equal(got, base) and torch.equal(got_p, base_p), order
        if order == 0:
            continue
        # a chain captured under the other value is never replayed, and setting the option back replays the first one
        m.hparams.sampling.solver_noise = 1
        second, _ = m.sample(x, wav, noise=noise)
        assert not torch.equal(second, base)
        m.hparams.sampling.solver_noise = 0
        again, _ = m.sample(x, wav, noise=noise)
        assert torch.equal(again, base)


def test_sample_long_vs_restatement():
    from diffroll_amd import longform
    from oracle import philox
    hp = hp_of(channels=128, layers=3)
    p = R.synthetic_params(hp, seed=81)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    g = torch.Generator().manual_seed(81)
    L = 1400 * HOP - 100
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    seed, rec = 21, 2
    z = {t: longform.gather_windows(torch.from_numpy(philox.step_noise(seed, rec, 1, plan.T_c * 88, t)).reshape(plan.T_c, 88),
                                    plan).unsqueeze(1)
         for t in CR.visited(S, 20) if t > 0}
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 20, order=2, solver_noise=1, w=0.5, plan=plan)
    win = run_plan_windows(m, plan, wav, x_T, None, seed=seed, recording=rec)
    assert_shared_frames_agree(win, plan)
    ok, d = agree(win, ref[:, 0])
    print(f"\nlong-form stochastic order 2 n 20: max |d| {d:.3e}")
    assert ok, d
    roll = m.sample_long(wav, overlap=160, seed=seed, recording=rec, x_T=x_T).cpu()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.solver_order == 2 and m.engine.solver_noise == 1


def test_draws_equal_the_tiled_batch_bitwise():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=82)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, _, _ = inputs(2, 40, 83)
    x = torch.randn(2, 1, 40, 88, generator=torch.Generator().manual_seed(84)).repeat(3, 1, 1, 1)      # 3 draws of 2 clips, one x_T per clip
    got, _ = m.sample(x, wav, seed=7, draws=3)
    ref, _ = m.sample(x, wav.repeat(3, 1), seed=7)
    assert torch.equal(got, ref)
    assert not torch.equal(got[:2], got[2:4]) and not torch.equal(got[2:4], got[4:])      # the draws differ - through the noise alone


def test_guidance_interval_vs_restatement():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=85)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    m.hparams.sampling.guidance_interval = [60, 140]
    wav, x, noise = inputs(2, 40, 86)
    spec = R.frontend(wav, hp, 40)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, 20, order=2, solver_noise=1, w=0.5, interval=(60, 140))
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\nguidance [60, 140] stochastic order 2 n 20: max |d| {d:.3e}")
    assert ok, d
    whole = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, 20, order=2, solver_noise=1, w=0.5)
    assert not agree(roll, whole)[0]                  # (the interval matters at this weight)


@pytest.mark.parametrize("injected", [True, False], ids=["z", "philox"])
def test_order_1_resumed_chain_ends_in_the_whole_chains_roll_bitwise(injected):
    """traj[i] is x AT visited[i + 1]: the chain started there draws the z's the whole chain draws from there on."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=90)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 1)
    wav, x, noise = inputs(2, 40, 91)
    kw = dict(noise=noise) if injected else dict(seed=0x1234567890AB, first_sample=3)
    traj, _ = m.sample_trajectory(x, wav, **kw)
    whole, _ = m.sample(x, wav, **kw)
    assert torch.equal(whole, traj[-1])
    visited = m.visited_steps()
    for i in (0, 9, 18):
        m.hparams.sampling.start_step = visited[i + 1]
        roll, _ = m.sample(traj[i], wav, **kw)
        assert m.engine.start_step == visited[i + 1]
        assert torch.equal(roll, traj[-1]), (i, maxdiff(roll.cpu(), traj[-1].cpu()))


def test_dr_step_over_the_visited_steps_ends_where_sample_ends():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=92)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, noise = inputs(2, 40, 93)
    traj, _ = m.sample_trajectory(x, wav, noise=noise)
    roll, _ = m.sample(x, wav, noise=noise)
    assert traj.shape == (20,) + tuple(roll.shape) and torch.equal(traj[-1], roll)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), noise, 20, order=2, solver_noise=1, w=0.5, trajectory=True)
    d = maxdiff(traj.cpu(), ref)
    print(f"\ntrajectory stochastic order 2 n 20: max |d| {d:.3e}")
    assert d <= 1e-5
    traj, _ = m.sample_trajectory(x, wav, seed=4, first_sample=1)
    roll, _ = m.sample(x, wav, seed=4, first_sample=1)
    assert torch.equal(traj[-1], roll)


def test_two_half_batches_equal_the_whole_batch():
    from diffroll_amd.distributed import sample_sharded_sequential
    hp = hp_of()
    p = R.synthetic_params(hp, seed=94)
    m = noisy_model(hp, p, "cfdg_ddpm_x0", 20, 2)
    wav, x, _ = inputs(4, 40, 95)
    whole, _ = m.sample(x, wav, seed=13)
    halves = sample_sharded_sequential(m, x, wav, None, seed=13, world_size=2)
    ok, d = agree(halves, whole.cpu())
    print(f"\ntwo half-batches vs the whole batch: max |d| {d:.3e}")
    assert ok, d
    assert not torch.equal(whole[0], whole[2])        # (rows 0 and 2 - the two shards' first - drew different noise)
