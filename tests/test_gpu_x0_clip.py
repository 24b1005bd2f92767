"""Option "x0_clip" on the MI355X (hparams.sampling.x0_clip): the HIP chain with the clamp of the x0 prediction against the
CPU restatement of tests/clip_ref.py - five x0 sampler / weight cases, n in {all S, 4, 20}, both ranges, injected noise
and the replayed Philox draws, both precisions - under the solver orders with and without noise, a guidance interval, a
resumed chain, strength with init=, long-form windows, draws, sharding, the fused path (graph = eager = per-phase, nothing
stale replayed when the option is toggled), dr_step over the visited steps, the option at 0 as the engine that never set
it, and the range [lo / c2, hi / c2] of every clipped roll.  The inputs and their references are those of
tests/clip_cases.py, which tests/test_x0_clip_cpu.py shows to exercise the bounds; tolerance: agree / ATOL of the existing
parity tests - a clamp is 1-Lipschitz, so the established margin carries over."""
import pytest
import torch

from testlib import S, agree, assert_shared_frames_agree, make_model, maxdiff, run_plan_windows

import chain_ref as CR
import clip_cases as CC
import clip_ref as CL

pytestmark = pytest.mark.gpu


def clipped_model(hp, p, sampler, w, code, n=20, **kw):
    """The facade with hparams.sampling.x0_clip on and hparams.norm_args naming the range of `code` (0: the key absent)."""
    options = {k: kw.pop(k) for k in ("solver_order", "solver_noise", "guidance_interval", "strength") if k in kw}
    m = make_model(hp, p, sampler=sampler, w=w, **kw)
    m.hparams.sampling.steps = n or None
    if code:
        m.hparams.sampling.x0_clip = 1
        m.hparams.norm_args[0:2] = list(CL.BOUNDS[code])
    for k, v in options.items():
        setattr(m.hparams.sampling, k, v)
    return m


def guided(code=1, n=20, **kw):
    """The guided case of clip_cases: cfdg_ddpm_x0 at w = 3 on the shared inputs."""
    hp, p, wav, x, noise, _ = CC.setup()
    return clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, code, n, **kw), wav, x, noise


# ---------------------------------------------------------------------------------------------- 1. the option
def test_option_is_public_and_validated():
    hp, p, wav, x, _, _ = CC.setup()
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    assert eng.x0_clip == 0
    eng.set_option("x0_clip", 1)                     # DR_ENAME (-> ValueError) before the option existed
    assert eng.x0_clip == 1
    eng.set_option("x0_clip", 2)
    for bad in (3, -1):
        with pytest.raises(ValueError, match=f"x0_clip.*{bad}"):
            eng.set_option("x0_clip", bad)
    assert eng.x0_clip == 2
    eng.set_option("x0_clip", 0)
    # an epsilon sampler has no x0 prediction: refused at the call, naming both, by sample and by step
    me = make_model(hp, p, sampler="ddim")
    me.engine.set_option("x0_clip", 1)
    try:
        me._engine.frontend(wav, CC.TN)
        xb = x.squeeze(1).to(me._engine.device).contiguous()
        with pytest.raises(ValueError, match=r"sampler 7 .*x0_clip = 1"):
            me._engine.sample("ddim", xb, None)
        with pytest.raises(ValueError, match=r"sampler 7 .*x0_clip = 1"):
            me._engine.sample("ddim", xb, None, use_graph=False)
        with pytest.raises(ValueError, match=r"sampler 7 .*x0_clip = 1"):
            me._engine.step("ddim", xb, None, S - 1)
    finally:
        me._engine.set_option("x0_clip", 0)
    me._engine.step("ddim", xb, None, S - 1)          # ... and runs with the option off
    me._engine.finish()
    # the facade refuses it before anything reaches the engine
    me.hparams.sampling.x0_clip = 1
    with pytest.raises(ValueError, match="epsilon"):
        me.sample(x, wav)


# ---------------------------------------------------------------------------------------------- 2. the chains
@pytest.mark.parametrize("sampler,w,code,n", CC.CASES, ids=CC.CASE_IDS)
def test_chain_vs_restatement(sampler, w, code, n):
    hp, p, wav, x, noise, _ = CC.setup()
    m = clipped_model(hp, p, sampler, w, code, n)
    for philox, kw in ((False, dict(noise=noise)), (True, dict(seed=CC.PHILOX_SEED))):
        ref = CC.assert_exercised(sampler, w, code, n, philox)       # (the inputs clamp, before the engine's roll is looked at)
        roll, _ = m.sample(x, wav, **kw)
        ok, d = agree(roll, ref)
        print(f"\n{sampler} w {w} code {code} n {n or S} {'philox' if philox else 'injected'}: max |d| {d:.3e}")
        assert ok, (philox, d)
        assert CC.in_range(roll, hp, code)
    assert m.engine.x0_clip == code


# ---------------------------------------------------------------------------------------------- 3. split bf16
def test_split_bf16_vs_restatement():
    m, wav, x, noise = guided(precision="bf16x3")
    ref = CC.assert_exercised("cfdg_ddpm_x0", 3.0, 1, 20)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\nbf16x3 w 3 code 1 n 20: max |d| {d:.3e}")
    assert ok, d
    assert CC.in_range(roll, CC.setup()[0], 1)


# ---------------------------------------------------------------------------------------------- 4. with the other options
@pytest.mark.parametrize("name,kw", CC.OPTION_CASES, ids=[c[0] for c in CC.OPTION_CASES])
def test_solver_orders_and_interval_vs_restatement(name, kw):
    facade = dict(kw)
    if "order" in facade:
        facade["solver_order"] = facade.pop("order")
    if "interval" in facade:
        facade["guidance_interval"] = list(facade.pop("interval"))
    m, wav, x, noise = guided(**facade)
    ref = CC.assert_exercised("cfdg_ddpm_x0", 3.0, 1, 20, **kw)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\n{name} w 3 code 1 n 20: max |d| {d:.3e}")
    assert ok, d
    assert CC.in_range(roll, CC.setup()[0], 1)
    if name != "order1-noise":                        # (stochastic order 1 IS the ddpm_x0 update by another arithmetic route)
        plain = CC.reference("cfdg_ddpm_x0", 3.0, 1, 20)[0]
        assert not agree(roll, plain)[0]              # the option beside the clamp matters on these inputs


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("injected", [True, False], ids=["z", "philox"])
def test_resumed_clipped_chain_ends_in_the_whole_clipped_chains_roll_bitwise(injected, order):
    """traj[i] is x AT visited[i + 1]: the chain started there clamps and draws what the whole chain does from there on."""
    m, wav, x, noise = guided(solver_order=order, solver_noise=1 if order else 0)
    kw = dict(noise=noise) if injected else dict(seed=0x1234567890AB, first_sample=3)
    traj, _ = m.sample_trajectory(x, wav, **kw)
    whole, _ = m.sample(x, wav, **kw)
    assert torch.equal(whole, traj[-1]) and CC.in_range(whole, CC.setup()[0], 1)
    visited = m.visited_steps()
    for i in (0, 9, 18):
        m.hparams.sampling.start_step = visited[i + 1]
        roll, _ = m.sample(traj[i], wav, **kw)
        assert m.engine.start_step == visited[i + 1] and m.engine.x0_clip == 1
        assert torch.equal(roll, traj[-1]), (i, maxdiff(roll.cpu(), traj[-1].cpu()))
        assert CC.in_range(roll, CC.setup()[0], 1)
    if injected and order == 0:
        ok, d = agree(whole, CC.reference("cfdg_ddpm_x0", 3.0, 1, 20)[0])
        assert ok, d


def test_strength_with_init_vs_restatement():
    """The diffusion of "start_noise" is not clamped (a clean roll in [0, 1] times A plus Sm z is what it is); the steps are."""
    hp, p, wav, _, noise, spec = CC.setup()
    m, _, _, _ = guided(strength=0.5)
    x0 = torch.rand(CC.B, 1, CC.TN, 88, generator=torch.Generator().manual_seed(94))
    t0 = CR.visited(S, 20)[10]                        # strength 0.5 of 20 steps: the last 10
    x = CR.diffuse(hp, x0, t0, noise[0])
    ref, moved = CL.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, 20, code=1, w=3.0, start=t0)
    unclipped = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, 20, w=3.0, start=t0)
    CC.exercised(moved, ("lo", "hi"), ref, unclipped)
    got, _ = m.sample(None, wav, noise=noise, init=x0)
    assert m.engine.start_step == t0 and m.engine.start_noise == 0
    ok, d = agree(got, ref)
    print(f"\nstrength 0.5 with init, w 3 code 1 n 20: max |d| {d:.3e}")
    assert ok, d
    want, _ = m.sample(x, wav, noise=noise)           # the same chain from the host's diffusion: bit for bit
    assert torch.equal(got, want)
    assert CC.in_range(got, hp, 1)


# ---------------------------------------------------------------------------------------------- 5. windows, draws, shards
def test_sample_long_vs_restatement():
    from diffroll_amd import longform
    hp, p, plan, wav, x_T = CC.long_case()
    ref, moved = CC.long_reference()
    CC.exercised(moved, ("lo", "hi"), ref, CC.long_reference(0)[0])
    m = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 1, 20)
    win = run_plan_windows(m, plan, wav, x_T, None, seed=CC.LONG_SEED, recording=CC.LONG_REC)
    assert_shared_frames_agree(win, plan)             # two windows clamp the same mean: torch.equal on the frames they share
    ok, d = agree(win, ref[:, 0])
    print(f"\nlong-form w 3 code 1 n 20: max |d| {d:.3e}")
    assert ok, d
    roll = m.sample_long(wav, overlap=160, seed=CC.LONG_SEED, recording=CC.LONG_REC, x_T=x_T).cpu()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.x0_clip == 1
    assert CC.in_range(roll, hp, 1)


def test_draws_equal_the_tiled_batch_bitwise():
    m, wav, x, _ = guided()
    x = x.repeat(2, 1, 1, 1)                          # 2 draws of 2 clips, one x_T per clip
    got, _ = m.sample(x, wav, seed=7, draws=2)
    ref, _ = m.sample(x, wav.repeat(2, 1), seed=7)
    assert torch.equal(got, ref)
    assert not torch.equal(got[:2], got[2:])          # the draws differ - through the noise alone
    assert CC.in_range(got, CC.setup()[0], 1)


def test_sample_sharded_on_one_rank_is_the_unsharded_chain():
    from diffroll_amd.distributed import sample_sharded, sample_sharded_sequential
    m, wav, x, noise = guided()
    for kw in (dict(noise=noise), dict(noise=None)):
        whole, _ = m.sample(x, wav, seed=13, **kw)
        one = sample_sharded(m, x, wav, kw["noise"], seed=13)         # no process group: world = 1
        assert torch.equal(one.cpu(), whole.cpu())
        assert CC.in_range(whole, CC.setup()[0], 1) and CC.in_range(one, CC.setup()[0], 1)
    halves = sample_sharded_sequential(m, x, wav, None, seed=13, world_size=2)
    ok, d = agree(halves, whole.cpu())
    print(f"\ntwo half-batches vs the whole batch: max |d| {d:.3e}")
    assert ok, d
    assert CC.in_range(halves, CC.setup()[0], 1) and m.engine.x0_clip == 1


# ---------------------------------------------------------------------------------------------- 6. the fused path
def test_fused_path_graph_eager_per_phase_and_nothing_stale_is_replayed():
    """16 guided clips x 125 frames at C = 512: four row tiles of the tail kernel's part T3 recompute every update - and every
    clamp and every Philox draw (stochastic order 2: the seed is read) - in different blocks, and one of them stores the clamped
    prediction as the order-2 history."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp, p, wav, x = CC.fused_case()
    m = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 1, 20, solver_order=2, solver_noise=1)
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
        # 1 -> 0 -> 1: each value replays (or captures) its own chain
        m.hparams.sampling.x0_clip = 0
        off, _ = m.sample(x, wav, seed=5)
        assert eng.x0_clip == 0
        m.hparams.sampling.x0_clip = 1
        again, _ = m.sample(x, wav, seed=5)
        e, _ = m.sample(x, wav, seed=5, use_graph=False)
        eng.set_option("fused_stack", 0)
        pp, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "per_phase" and st["fallbacks"] == 0 and st["yields"] == 0, st
        eng.set_option("fused_stack", 1)
        # fresh engines: what g2 and `off` must be if neither seed, history nor the other value's chain leaked into them
        m2 = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 1, 20, solver_order=2, solver_noise=1)
        for k, (v, _) in pins.items():
            m2.engine.set_option(k, v)
        fresh, _ = m2.sample(x2, wav, seed=6)
        other, _ = m2.sample(x2, wav, seed=5)
        assert m2.engine.launch_state()["mode"] == "fused_stack+tail"
        m3 = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 0, 20, solver_order=2, solver_noise=1)      # never set the option
        for k, (v, _) in pins.items():
            m3.engine.set_option(k, v)
        never, _ = m3.sample(x, wav, seed=5)
        assert m3.engine.launch_state()["mode"] == "fused_stack+tail" and m3.engine.x0_clip == 0
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
    assert torch.equal(g, e) and torch.equal(g, pp) and torch.equal(g, again)
    assert torch.equal(g2, fresh) and not torch.equal(g2, g)
    assert not torch.equal(other, fresh)              # (the seed is read: the same x_T under the first seed is another roll)
    assert torch.equal(off, never) and not torch.equal(off, g)
    ref, moved = CC.fused_reference()
    CC.exercised(moved, ("lo", "hi"), ref, CC.fused_reference(0)[0])
    ok, d = agree(g[CC.FUSED_SEL], ref)
    print(f"\nfused path w 3 code 1 stochastic order 2 n 20: max |d| {d:.3e}")
    assert ok, d
    assert CC.in_range(g, hp, 1) and CC.in_range(g2, hp, 1) and not CC.in_range(off, hp, 1)


@pytest.mark.parametrize("sampler,w,inert", [
    ("cfdg_ddpm_x0", 3.0, {"solver_noise": 1}),                      # ... while solver_order is 0
    ("cfdg_ddpm_x0", 3.0, {"draw_stride": 7}),                       # ... while draws is 1
    ("ddpm_x0", 0.0, {"guidance_t_min": 1, "guidance_t_max": 2}),    # ... on a sampler that does not guide
], ids=["solver_noise-without-order", "draw_stride-without-draws", "interval-without-guidance"])
def test_inert_option_values_replay_the_captured_chain(sampler, w, inert):
    """A value that is inert under the other options is not part of a captured chain's key: setting it replays the chain -
    the same roll bit for bit, and no launch counted (captured launches count once, at capture).  Control: "x0_clip" 0 -> 1
    is part of the key and captures again; back at 0 the first roll comes back.  Four steps: the shortest chain with a
    second-order step and a step into 0."""
    hp, p, wav, x, _, _ = CC.setup()
    m = make_model(hp, p, sampler=sampler, w=w)
    m.hparams.sampling.steps = 4
    eng = m.engine
    eng.frontend(wav, CC.TN)
    x_T = x.squeeze(1).to(eng.device).contiguous()

    def run():
        return eng.sample(sampler, x_T.clone(), None, w=w, seed=CC.PHILOX_SEED)

    first, c0 = run(), eng.launch_counts()
    assert sum(c0) > 0                                # (the capture was counted: the counter sees this chain)
    for name, value in inert.items():
        eng.set_option(name, value)
    again = run()
    assert torch.equal(again, first)
    assert eng.launch_counts() == c0, (c0, eng.launch_counts())
    eng.set_option("x0_clip", 1)
    run()
    assert eng.launch_counts() != c0
    eng.set_option("x0_clip", 0)
    assert torch.equal(run(), first)


# ---------------------------------------------------------------------------------------------- 7. dr_step
def test_dr_step_over_the_visited_steps_ends_where_sample_ends():
    """Order 2: the history the steps hand on is the clamped prediction."""
    m, wav, x, noise = guided(solver_order=2)
    traj, _ = m.sample_trajectory(x, wav, noise=noise)
    roll, _ = m.sample(x, wav, noise=noise)
    assert traj.shape == (20,) + tuple(roll.shape) and torch.equal(traj[-1], roll)
    hp, p, _, _, _, spec = CC.setup()
    assert CC.in_range(roll, hp, 1) and CC.in_range(traj[-1], hp, 1)
    ref, _ = CL.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, 20, code=1, w=3.0, order=2, trajectory=True)
    assert torch.equal(ref[-1], CC.reference("cfdg_ddpm_x0", 3.0, 1, 20, order=2)[0])
    d = maxdiff(traj.cpu(), ref)
    print(f"\ntrajectory w 3 code 1 order 2 n 20: max |d| {d:.3e}")
    assert d <= 1e-5
    m.hparams.sampling.solver_order = 0               # ... and the sampler's own update, with Philox
    traj, _ = m.sample_trajectory(x, wav, seed=4, first_sample=1)
    roll, _ = m.sample(x, wav, seed=4, first_sample=1)
    assert torch.equal(traj[-1], roll) and CC.in_range(roll, hp, 1)


def test_a_change_of_the_option_ends_a_dr_step_history():
    """Order 2: p is the prediction as the previous step clamped it, so a dr_step sequence does not continue across a change of
    the value - the next step that is not a chain's first is refused, as after a change of "solver_noise"."""
    from diffroll_amd.engine import EngineError
    hp, p, _, _, _, _ = CC.setup()
    eng = make_model(hp, p, sampler="generation_ddpm_x0").engine
    eng.set_option("sampling_steps", 20)
    eng.set_option("solver_order", 2)
    v = eng.visited_steps()
    x = torch.randn(CC.B, CC.TN, 88, device=eng.device)

    def step(t):
        eng.step("generation_ddpm_x0", x, None, t)

    step(v[0])
    step(v[1])
    eng.set_option("x0_clip", 1)
    with pytest.raises(EngineError, match="continues no history"):
        step(v[2])
    step(v[0])                                        # a chain's first step starts a new history under the new value
    step(v[1])
    eng.set_option("x0_clip", 1)                      # the same value: nothing ends
    step(v[2])
    eng.set_option("x0_clip", 0)
    with pytest.raises(EngineError, match="continues no history"):
        step(v[3])
    eng.finish()


# ---------------------------------------------------------------------------------------------- 8. off
def test_code_0_after_code_1_is_the_engine_that_never_set_it():
    hp, p, wav, x, noise, _ = CC.setup()
    for order in (0, 2):
        never = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 0, 20, solver_order=order)
        base, _ = never.sample(x, wav, noise=noise)
        base_p, _ = never.sample(x, wav, seed=6)
        m = clipped_model(hp, p, "cfdg_ddpm_x0", 3.0, 1, 20, solver_order=order)
        on, _ = m.sample(x, wav, noise=noise)
        on_p, _ = m.sample(x, wav, seed=6)
        assert m.engine.x0_clip == 1 and not torch.equal(on, base) and not torch.equal(on_p, base_p)
        assert CC.in_range(on, hp, 1) and CC.in_range(on_p, hp, 1) and not CC.in_range(base, hp, 1)
        m.hparams.sampling.x0_clip = 0
        got, _ = m.sample(x, wav, noise=noise)
        got_p, _ = m.sample(x, wav, seed=6)
        assert m.engine.x0_clip == 0
        assert torch.equal(got, base) and torch.equal(got_p, base_p), order
        e, _ = m.sample(x, wav, noise=noise, use_graph=False)
        assert torch.equal(e, base), order
        m.hparams.sampling.x0_clip = 1                # ... and back: the first chain, not the one in between
        back, _ = m.sample(x, wav, noise=noise)
        assert torch.equal(back, on) and CC.in_range(back, hp, 1), order
        ok, d = agree(base, CC.reference("cfdg_ddpm_x0", 3.0, 0, 20, order=order)[0])
        assert ok, d
