"""Options "start_step" / "start_noise" on the MI355X (hparams.sampling.start_step / .strength, sample(init=...)): a chain
resumed from a row of the whole chain's trajectory ends in the whole chain's roll bit for bit; the diffusion node against
the host's (A * x0) + (Sm * z) with injected noise (bitwise) and with the replayed Philox draws; the fused path (graph =
eager = per-phase, no state across replays); long-form windows, draws, solver order 2 and dr_step; and off as the engine
that never set the options."""
import math

import pytest
import torch

from oracle import diffroll_ref as R
from testlib import ATOL, HOP, S, agree, assert_shared_frames_agree, hp_of, inputs, make_model, maxdiff

import chain_ref as CR

pytestmark = pytest.mark.gpu

B, TN = 2, 40            # 2 * 40 * 88 / 4 = 1760 quads: seven blocks of diffuse_kernel, the last one partial


def rolls(B_, Tn, seed):
    """A clean roll in the model's roll space: (B, 1, Tn, 88) in [0, 1]."""
    return torch.rand(B_, 1, Tn, 88, generator=torch.Generator().manual_seed(seed))


def started(m, t_s, n=None):
    if n is not None:
        m.hparams.sampling.steps = n
    m.hparams.sampling.start_step = t_s
    return m


# ---------------------------------------------------------------------------------------------- 1. the options
def test_options_are_public_and_validated():
    hp = hp_of(layers=2)
    p = R.synthetic_params(hp, seed=1)
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    eng.set_option("start_step", 57)                  # DR_ENAME (-> ValueError) before the options existed
    eng.set_option("start_noise", 1)
    assert (eng.start_step, eng.start_noise) == (57, 1)
    for name, bads in (("start_step", (-2, S, S + 5)), ("start_noise", (-1, 2))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                eng.set_option(name, bad)
    assert (eng.start_step, eng.start_noise) == (57, 1)
    eng.set_option("start_noise", 0)
    # a start the respaced chain does not visit is refused at the call, with both neighbours named
    eng.set_option("sampling_steps", 20)
    visited = eng.visited_steps()
    assert 57 not in visited and 63 in visited and 52 in visited
    x = torch.randn(B, TN, 88, device=eng.device)
    with pytest.raises(ValueError, match=r"start_step 57 .*63 and 52"):
        eng.sample("generation_ddpm_x0", x.clone(), None)
    with pytest.raises(ValueError, match=r"start_step 57 .*63 and 52"):
        eng.sample("generation_ddpm_x0", x.clone(), None, use_graph=False)
    # ... and the chain's first visited step is the chain with -1, bit for bit (Philox and injected noise)
    noise = torch.randn(S, B, TN, 88, device=eng.device)
    got = {}
    for start in (-1, visited[0]):
        eng.set_option("start_step", start)
        got[start] = (eng.sample("generation_ddpm_x0", x.clone(), None, seed=3), eng.sample("generation_ddpm_x0", x.clone(), noise))
    assert torch.equal(got[-1][0], got[visited[0]][0]) and torch.equal(got[-1][1], got[visited[0]][1])
    eng.set_option("start_step", -1)
    # the facade refuses a start that is not visited before anything reaches the engine
    m.hparams.sampling.steps, m.hparams.sampling.start_step = 20, 57
    with pytest.raises(ValueError, match="63 and 52"):
        m.sample(x.unsqueeze(1).cpu())


# ---------------------------------------------------------------------------------------------- 2. resume identity
RESUME = [
    # sampler, n, injected noise, graph, extra
    ("cfdg_ddpm_x0", 20, True, True, {}),
    ("cfdg_ddpm_x0", 0, False, False, {}),
    ("ddim2ddpm", 20, False, True, {}),
    ("ddim2ddpm", 0, True, False, {}),
    ("generation_ddpm_x0", 20, True, False, {}),
    ("generation_ddpm_x0", 0, False, True, {}),
    ("cfdg_ddpm_x0", 20, False, True, {"guidance_interval": [60, 140]}),
    ("cfdg_ddpm_x0", 20, True, True, {"precision": "bf16x3"}),
]


@pytest.mark.parametrize("sampler,n,injected,graph,extra", RESUME,
                         ids=[f"{c[0]}-n{c[1] or S}-{'z' if c[2] else 'philox'}-{'graph' if c[3] else 'eager'}" +
                              "".join(f"-{k}" for k in c[4]) for c in RESUME])
def test_resumed_chain_ends_in_the_whole_chains_roll_bitwise(sampler, n, injected, graph, extra):
    """traj[i] is x after visited[i], i.e. x AT visited[i + 1]: the chain started there must end in traj[-1]."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=90)
    m = make_model(hp, p, sampler=sampler, w=0.5, precision=extra.get("precision", "f32"))
    if "guidance_interval" in extra:
        m.hparams.sampling.guidance_interval = extra["guidance_interval"]
    m.hparams.sampling.steps = n or None
    wav, x, noise = inputs(B, TN, 91)
    kw = dict(noise=noise) if injected else dict(seed=0x1234567890AB, first_sample=3)
    traj, _ = m.sample_trajectory(x, wav, **kw)
    visited = m.visited_steps()
    count = len(visited)
    assert traj.shape[0] == count == (n or S)
    for i in (0, count // 2, count - 2):
        m.hparams.sampling.start_step = visited[i + 1]
        roll, _ = m.sample(traj[i], wav, use_graph=graph, **kw)
        assert m.engine.start_step == visited[i + 1]
        assert torch.equal(roll, traj[-1]), (i, maxdiff(roll.cpu(), traj[-1].cpu()))
    m.hparams.sampling.start_step = None
    whole, _ = m.sample(x, wav, use_graph=graph, **kw)
    assert torch.equal(whole, traj[-1]) and m.engine.start_step == -1


# ---------------------------------------------------------------------------------------------- 3. start_noise, injected
def test_start_noise_with_injected_noise_is_the_hosts_q_sample_bitwise():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=92)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    wav, _, noise = inputs(B, TN, 93)
    x0 = rolls(B, TN, 94)
    for n, t_s in ((20, 105), (20, None), (0, 77)):
        m.hparams.sampling.steps, m.hparams.sampling.start_step = n or None, t_s
        t_eff = m.visited_steps()[0] if t_s is None else t_s
        A, Sm = m.sqrt_alphas_cumprod[t_eff], m.sqrt_one_minus_alphas_cumprod[t_eff]
        x = (A * x0) + (Sm * noise[0])                # fp32 torch on the host: each product once, then the sum
        for graph in (True, False):
            got, _ = m.sample(None, wav, noise=noise, init=x0, use_graph=graph)
            want, _ = m.sample(x, wav, noise=noise, use_graph=graph)
            assert torch.equal(got, want), (n, t_s, graph, maxdiff(got.cpu(), want.cpu()))
            assert m.engine.start_noise == 0          # held for the call only
    with pytest.raises(ValueError, match="either x_T"):
        m.sample(x, wav, init=x0)


# ---------------------------------------------------------------------------------------------- 4. start_noise, Philox
@pytest.mark.parametrize("seed,first", [(0, 0), (0xFEDCBA9876543210, 5)])
def test_start_noise_with_philox_vs_the_replayed_draws(seed, first):
    hp = hp_of()
    p = R.synthetic_params(hp, seed=95)
    m = started(make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5), 105, 20)
    wav, _, _ = inputs(B, TN, 96)
    x0 = rolls(B, TN, 97)
    z = CR.diffusion_noise(seed, first, S, B, TN, 105)
    assert abs(float(z.std()) - 1.0) < 0.05 and abs(float(z.mean())) < 0.05
    assert not torch.equal(z, torch.from_numpy(CR.philox.step_noise(seed, first, B, TN * 88, 105).reshape(B, 1, TN, 88)))
    x = CR.diffuse(hp, x0, 105, z)
    for graph in (True, False):
        got, _ = m.sample(None, wav, seed=seed, first_sample=first, init=x0, use_graph=graph)
        want, _ = m.sample(x, wav, seed=seed, first_sample=first, use_graph=graph)
        ok, d = agree(got, want.cpu())
        print(f"\nstart_noise Philox seed {seed:#x} first {first} graph {graph}: max |d| {d:.3e}")
        assert ok, d
    assert not torch.equal(got, m.sample(None, wav, seed=seed + 1, first_sample=first, init=x0)[0])


def test_start_noise_keys_are_global():
    """Rows 2..3 of a B = 4 batch are a B = 2 call at first_sample = 2."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=98)
    m = started(make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5), 105, 20)
    wav, _, _ = inputs(4, TN, 99)
    x0 = rolls(4, TN, 100)
    whole, _ = m.sample(None, wav, seed=11, init=x0)
    part, _ = m.sample(None, wav[2:], seed=11, first_sample=2, init=x0[2:])
    ok, d = agree(whole[2:], part.cpu())
    print(f"\nrows 2..3 of B = 4 vs B = 2 at first_sample 2: max |d| {d:.3e}")
    assert ok, d
    assert not agree(whole[:2], part.cpu())[0]


# ---------------------------------------------------------------------------------------------- 5. fused path
def test_fused_path_graph_eager_per_phase_and_nothing_across_replays():
    """16 guided clips x 125 frames at C = 512, started at visited[10] of n = 20 from a clean roll."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=512, layers=3)
    p = R.synthetic_params(hp, seed=11)

    def model():
        m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
        m.hparams.sampling.steps = 20
        m.hparams.sampling.start_step = m.visited_steps()[10]
        return m
    m = model()
    wav, _, _ = inputs(16, 125, 76)
    x0, x02 = rolls(16, 125, 77), rolls(16, 125, 78)
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3202, 0), "tune.pw_nw": (4, 0), "tune.stack_fl": (2, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        t0 = eng.tail_launches
        g, _ = m.sample(None, wav, seed=5, init=x0)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
        g2, _ = m.sample(None, wav, seed=5, init=x02)     # the same captured chain, another init
        e, _ = m.sample(None, wav, seed=5, init=x0, use_graph=False)
        eng.set_option("fused_stack", 0)
        pp, _ = m.sample(None, wav, seed=5, init=x0)
        st = eng.launch_state()
        assert st["mode"] == "per_phase" and st["fallbacks"] == 0 and st["yields"] == 0, st
        eng.set_option("fused_stack", 1)
        m2 = model()
        fresh, _ = m2.sample(None, wav, seed=5, init=x02)
        assert m2.engine.launch_state()["mode"] == "fused_stack+tail"
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
    assert torch.equal(g, e) and torch.equal(g, pp)
    assert torch.equal(g2, fresh) and not torch.equal(g2, g)


# ---------------------------------------------------------------------------------------------- 6. long form
def test_long_form_refinement():
    from diffroll_amd import longform
    hp = hp_of(channels=128, layers=3)
    p = R.synthetic_params(hp, seed=81)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.hparams.sampling.steps, m.hparams.sampling.strength = 20, 0.5
    visited = m.visited_steps()
    t_s = visited[10]
    assert m.start_step() == t_s
    g = torch.Generator().manual_seed(82)
    L = 1400 * HOP - 100
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    init = torch.rand(1, 1, plan.T_out, 88, generator=g)
    seed, rec = 4, 1
    canvas = m._init_canvases([init], None, longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n), 1)[0]
    assert canvas.shape == (1, 1, plan.T_c, 88) and torch.equal(canvas[:, :, :plan.T_out], init) and not canvas[:, :, plan.T_out:].any()
    batch = longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)
    win = m._sample_windows(batch, [wav], [canvas], None, 1, seed, rec, True, True, start_noise=1).cpu()
    assert_shared_frames_agree(win, plan)
    roll = m.sample_long(wav, overlap=160, seed=seed, recording=rec, init=init).cpu()
    assert roll.shape == (1, 1, plan.T_out, 88) and torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.start_noise == 0 and m.engine.start_step == t_s
    # the restatement: one canvas draw per recording for the diffusion and for each step run
    x0w = longform.gather_windows(canvas.reshape(plan.T_c, 88), plan).unsqueeze(1)
    x = CR.diffuse(hp, x0w, t_s, CR.window_noise(seed, rec, S, plan, t_s))
    zs = {t: CR.window_noise(seed, rec, 0, plan, t) for t in visited[10:] if t > 0}
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, zs, 20, start=t_s, w=0.5, plan=plan)
    ok, d = agree(win, ref[:, 0])
    print(f"\nlong-form strength 0.5 n 20: max |d| {d:.3e}")
    assert ok, d
    # feeding a returned roll back works, and two recordings in one chain are their solo chains
    again = m.sample_long(wav, overlap=160, seed=seed, recording=rec, init=roll)
    assert again.shape == roll.shape
    L1 = 300 * HOP + 17
    wav1 = 0.1 * torch.randn(L1, generator=g)
    init1 = torch.rand(1, 1, math.ceil(L1 / HOP), 88, generator=g)
    both = m.sample_long_batch([wav1, wav], overlap=160, seed=seed, first_recording=7, init=[init1, init])
    solo = [m.sample_long(wv, overlap=160, seed=seed, recording=7 + i, init=ini) for i, (wv, ini) in enumerate(((wav1, init1), (wav, init)))]
    for i, (a, b) in enumerate(zip(both, solo)):
        d = maxdiff(a.cpu(), b.cpu())
        print(f"recording {i}: batch vs solo max |delta| = {d:.3e}")
        assert a.shape == b.shape and d <= ATOL and torch.equal(a > 0.5, b > 0.5), (i, d)


# ---------------------------------------------------------------------------------------------- 7. draws
def test_draws_equal_the_tiled_batch_bitwise():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=82)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.hparams.sampling.steps, m.hparams.sampling.strength = 20, 0.5
    wav, _, _ = inputs(B, TN, 83)
    init = rolls(B, TN, 84).repeat(2, 1, 1, 1)        # 2 draws of 2 clips, draw-major: the same roll for both draws
    got, _ = m.sample(None, wav, seed=9, draws=2, init=init)
    ref, _ = m.sample(None, wav.repeat(2, 1), seed=9, init=init)
    assert torch.equal(got, ref)
    assert not torch.equal(got[:B], got[B:])          # the draws differ: through the diffusion's z and the steps'


# ---------------------------------------------------------------------------------------------- 8. solver order 2
def test_solver_order_2_started_chain_and_dr_step():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=85)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.hparams.sampling.steps, m.hparams.sampling.solver_order = 20, 2
    visited = m.visited_steps()
    t_s = visited[5]
    m.hparams.sampling.start_step = t_s
    wav, x, _ = inputs(B, TN, 86)
    spec = R.frontend(wav, hp, TN)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, None, 20, start=t_s, w=0.5, order=2, trajectory=True)
    assert CR.chain_rows(hp, "cfdg_ddpm_x0", 20, order=2, start=t_s)[t_s][3] == 0
    assert CR.chain_rows(hp, "cfdg_ddpm_x0", 20, order=2)[t_s][3] != 0
    for graph in (True, False):
        roll, _ = m.sample(x, wav, use_graph=graph)
        ok, d = agree(roll, ref[-1])
        print(f"\norder 2 started at {t_s} graph {graph}: max |d| {d:.3e}")
        assert ok, d
    traj, _ = m.sample_trajectory(x, wav)             # dr_step from t_s on: the first one starts a history
    assert traj.shape[0] == 15 and torch.equal(traj[-1], roll)
    d = maxdiff(traj.cpu(), ref)
    print(f"trajectory order 2 from {t_s}: max |d| {d:.3e}")
    assert d <= ATOL
    # the whole chain's step at t_s is second order: the started one is another number
    whole = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, None, 20, start=t_s, w=0.5, order=1, trajectory=True)
    assert torch.equal(whole[0], ref[0]) and not torch.equal(whole[1], ref[1])
    eng = m.engine
    xb = x.squeeze(1).to(eng.device).contiguous()
    from diffroll_amd.engine import EngineError
    with pytest.raises(EngineError, match="expected next"):                    # (the chain above ended the history)
        eng.step("cfdg_ddpm_x0", xb.clone(), None, visited[7], 0.5)
    first = eng.step("cfdg_ddpm_x0", xb.clone(), None, t_s, 0.5)               # t_s starts a history ...
    second = eng.step("cfdg_ddpm_x0", first.clone(), None, visited[6], 0.5)    # ... and the step after it continues it
    with pytest.raises(EngineError, match=f"expected next is {visited[7]}"):
        eng.step("cfdg_ddpm_x0", xb.clone(), None, visited[8], 0.5)
    eng.finish()
    assert torch.equal(first, traj[0, :, 0]) and torch.equal(second, traj[1, :, 0])


# ---------------------------------------------------------------------------------------------- 9. off is off
def test_off_is_the_engine_that_never_set_the_options():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=87)
    wav, x, noise = inputs(B, TN, 88)
    never = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    base, _ = never.sample(x, wav, noise=noise)
    base_p, _ = never.sample(x, wav, seed=6)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    for name, v, off in (("start_step", 120, -1), ("start_noise", 1, 0)):
        m.engine.set_option(name, v)
        m.engine.set_option(name, off)
    got, _ = m.sample(x, wav, noise=noise)
    got_p, _ = m.sample(x, wav, seed=6)
    assert torch.equal(got, base) and torch.equal(got_p, base_p)
    # a chain captured under another start is never replayed, and setting the option back replays the first one
    m.hparams.sampling.start_step = 120
    second, _ = m.sample(x, wav, noise=noise)
    assert not torch.equal(second, base)
    third, _ = m.sample(None, wav, noise=noise, init=x)           # ... nor one captured without the diffusion node
    assert not torch.equal(third, second)
    m.hparams.sampling.start_step = None
    again, _ = m.sample(x, wav, noise=noise)
    assert torch.equal(again, base)
    short = never.sample_trajectory(x, wav, noise=noise)[0]
    m.hparams.sampling.start_step = 120
    resumed, _ = m.sample(short[S - 1 - 121], wav, noise=noise)   # (row i is x at step S - 2 - i)
    assert torch.equal(resumed, base)
