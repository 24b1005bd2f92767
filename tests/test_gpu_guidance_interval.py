"""Guidance interval on the MI355X (options "guidance_t_min" / "guidance_t_max", hparams.sampling.guidance_interval):
the HIP chain that runs the unconditional evaluation only at the steps lo <= t <= hi, against the CPU restatement of
tests/chain_ref.py (which evaluates both branches at every step) - the three guiding samplers, intervals with both
transitions inside the chain / ending guided / starting guided, injected and Philox noise, split-bf16 once - and the bit
identities the options promise: defaults = [0, S - 1] = an engine that never heard of them; fused stack + tail kernel across
both transitions = per-phase launches = a dr_step loop that passes w or 0 itself; captured = eager under changing intervals;
and the compositions with respacing, windows, draws, sharding and dr_sample_checked's re-run.

Shapes: S = 12 steps, B = 2 rolls of T = 125 frames (a partial 128-frame tile, not a multiple of 32), w = 0.5, on a reduced
network (C = 64, 3 layers, k = 3); one full-depth case (C = 512, L = 15, k = 9) at the end."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import diffroll_ref as R
from testlib import HOP, agree, assert_shared_frames_agree, make_model, maxdiff, run_plan_windows
from tuning_pins import pinned

import chain_ref as CR

pytestmark = pytest.mark.gpu

S, B, T, W = 12, 2, 125, 0.5
GUIDING = ["cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0"]
MASK = [30, 60]                      # the inpainting sampler's time mask (spectrogram frames)
# per-phase kernels pinned to the flavours the 64-frame fused kernels are built from, split-K off (tests/test_gpu_fused.py)
PINS = {"tune.ksplit_max": (1, 16), "tune.tile": (3201, 0), "tune.pw_nw": (2, 0), "tune.stack_fl": (1, 0)}


def hp_of(channels=64, layers=3, k=3):
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=channels, residual_layers=layers, kernel_size=k, timesteps=S)
    return hp


def inputs(n, Tn, seed):
    g = torch.Generator().manual_seed(seed)
    wav = torch.stack([(0.05 + 0.05 * i) * torch.randn(Tn * HOP, generator=g) for i in range(n)])
    x = torch.randn(n, 1, Tn, 88, generator=g)
    noise = torch.randn(S, n, 1, Tn, 88, generator=g)
    return wav, x, noise


def model_of(sampler, hp=None, seed=70, **kw):
    hp = hp or hp_of()
    p = R.synthetic_params(hp, seed=seed)
    it = MASK if sampler == "inpainting_ddpm_x0" else None
    return hp, p, make_model(hp, p, sampler=sampler, w=W, inpainting_t=it, **kw), it


def skip_if_forced():
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation") + tuple(PINS)):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")


def engine_inputs(eng, wav, x, noise, Tn=T):
    eng.frontend(wav, Tn, return_spec=False)
    xb = x.squeeze(1).to(eng.device).contiguous()
    z = noise.squeeze(2).to(eng.device).contiguous()
    return xb, z


def chain(eng, sampler, xb, z, use_graph, seed=3):
    out = xb.clone()
    eng.sample(sampler, out, z, W, seed, 0, use_graph, True)
    return out.cpu()


# ---------------------------------------------------------------------------------------------- 0. the options
def test_options_are_public_and_validated():
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    eng = m.engine
    eng.set_option("guidance_t_min", 4)              # DR_ENAME (-> ValueError) before the options existed
    eng.set_option("guidance_t_max", 8)
    assert eng.guidance_interval == (4, 8)
    for name, bad in (("guidance_t_min", -1), ("guidance_t_min", S), ("guidance_t_max", -2), ("guidance_t_max", S)):
        with pytest.raises(ValueError, match=name):
            eng.set_option(name, bad)
    assert eng.guidance_interval == (4, 8)
    for neighbour in ("guidance_t", "guidance_t_mid", "guidance_interval"):
        with pytest.raises(ValueError, match="unknown option"):
            eng.set_option(neighbour, 1)
    # lo > hi: accepted at the set (each value is in range), refused at the call with both values named
    eng.set_option("guidance_t_min", 9)
    wav, x, noise = inputs(B, 40, 1)
    xb, z = engine_inputs(eng, wav, x, noise, 40)
    for call in (lambda: eng.step("cfdg_ddpm_x0", xb.clone(), z[5], 5, W),
                 lambda: eng.sample("cfdg_ddpm_x0", xb.clone(), z, W, check=False),
                 lambda: eng.sample("cfdg_ddpm_x0", xb.clone(), z, W, check=True)):
        with pytest.raises(ValueError, match=r"guidance_t_min = 9 .* guidance_t_max = 8"):
            call()
    # ... by the samplers that guide only: the others ignore both options
    a = eng.step("ddpm_x0", xb.clone(), z[5], 5).cpu()
    eng.set_guidance_interval()
    assert eng.guidance_interval == (0, -1)
    assert torch.equal(eng.step("ddpm_x0", xb.clone(), z[5], 5).cpu(), a)
    eng.finish()
    for bad in ((9, 8), (0, S), (-1, 3), (2.0, 3)):
        with pytest.raises(ValueError):
            eng.set_guidance_interval(*bad)
    assert eng.guidance_interval == (0, -1)


# ---------------------------------------------------------------------------------------------- 1. versus the restatement
@pytest.mark.parametrize("interval", [(4, 8), (0, 5), (6, 11)], ids=["4-8", "0-5", "6-11"])
@pytest.mark.parametrize("sampler", GUIDING)
def test_chain_vs_restatement(sampler, interval):
    """[4, 8]: both transitions inside the chain; [0, 5]: the last step guided; [6, 11]: the first step guided."""
    hp, p, m, it = model_of(sampler)
    m.hparams.sampling.guidance_interval = list(interval)
    wav, x, noise = inputs(B, T, 71)
    spec = R.frontend(wav, hp, T, inpainting_t=it)
    zp = CR.philox_noise(9, 0, S, B, T)
    for z, kw in ((noise, dict(noise=noise)), (zp, dict(seed=9))):
        ref = CR.sample_chain(p, hp, sampler, x, spec, z, 0, w=W, interval=interval)
        roll, _ = m.sample(x, wav, **kw)
        assert m.engine.guidance_interval == interval
        ok, d = agree(roll, ref)
        print(f"\n{sampler} {interval} {'injected' if 'noise' in kw else 'philox'}: max |d| = {d:.3g}")
        assert ok, (sampler, interval, "injected" if "noise" in kw else "philox", d)
    # the interval matters: the fully guided chain is a roll that this comparison tells from the interval's (with few late
    # steps unguided the two end close together - [0, 5] guides the last six steps - so the check is the rule itself)
    full = CR.sample_chain(p, hp, sampler, x, spec, zp, 0, w=W)
    assert not agree(full, ref)[0], maxdiff(full, ref)


def test_split_bf16_vs_restatement():
    hp, p, m, _ = model_of("cfdg_ddpm_x0", precision="bf16x3")
    m.hparams.sampling.guidance_interval = [4, 8]
    wav, x, noise = inputs(B, T, 72)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, T), noise, 0, w=W, interval=(4, 8))
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    print(f"\nbf16x3 [4, 8]: max |d| = {d:.3g}")
    assert ok, d


# ---------------------------------------------------------------------------------------------- 2. bit identities
@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "cfdg_ddim_x0"])
def test_bit_identities_on_the_fused_path(sampler):
    """fused_stack = 2, so that B = 2 fuses.  (a) [0, S - 1] and the defaults are the chain of an engine whose options were
    never set, eager and captured.  (b) [4, 8] with fused stack + tail = [4, 8] per phase without the tail = a dr_step loop
    at default options that passes w inside the interval and 0.0 outside - today's code path.  (c) the fused run is two
    launches per step after the first: one standalone input projection and at most one standalone first-layer conv in the
    whole eager chain, i.e. the tail kernel primed the step behind each end of the interval."""
    skip_if_forced()
    hp, p, m, _ = model_of(sampler)
    eng = m.engine
    wav, x, noise = inputs(B, T, 73)
    xb, z = engine_inputs(eng, wav, x, noise)
    with pinned(eng, PINS, restore=("fused_stack", "fused_tail")):
        eng.set_option("fused_stack", 2)
        never_e, never_g = chain(eng, sampler, xb, z, False), chain(eng, sampler, xb, z, True)       # (a) options never set
        assert torch.equal(never_e, never_g)
        for lo, hi in ((0, S - 1), (0, -1)):
            eng.set_guidance_interval(lo, hi)
            assert torch.equal(chain(eng, sampler, xb, z, False), never_e), (lo, hi)
            assert torch.equal(chain(eng, sampler, xb, z, True), never_e), (lo, hi)
        eng.set_guidance_interval(4, 8)                                                              # (b), (c)
        st0, c0 = eng.launch_state(), eng.launch_counts()
        fused = chain(eng, sampler, xb, z, False)
        st1, c1 = eng.launch_state(), eng.launch_counts()
        assert st1["mode"] == "fused_stack+tail", st1
        assert st1["tail_launches"] - st0["tail_launches"] == S and st1["stack_launches"] - st0["stack_launches"] == S, (st0, st1)
        assert c1[0] - c0[0] == 1 and c1[1] - c0[1] <= 1, (c0, c1)
        assert st1["fallbacks"] == 0 and st1["yields"] == 0, st1
        assert torch.equal(chain(eng, sampler, xb, z, True), fused)
        eng.set_option("fused_stack", 0)
        eng.set_option("fused_tail", 0)
        per_phase = chain(eng, sampler, xb, z, False)
        assert eng.launch_state()["mode"] == "per_phase"
        assert torch.equal(fused, per_phase), maxdiff(fused, per_phase)
        eng.set_guidance_interval()
        loop = xb.clone()
        for t in range(S - 1, -1, -1):
            eng.step(sampler, loop, z[t], t, W if 4 <= t <= 8 else 0.0, 3, 0)
        eng.finish()
        assert torch.equal(fused, loop.cpu()), maxdiff(fused, loop.cpu())
        assert not torch.equal(fused, never_e)


def test_first_step_guided_primes_the_unguided_successor():
    """[6, 11] and [0, 5] on the fused path: the chain starts guided (one standalone conv, then the tail leaves the
    interval) / starts unguided (no standalone conv at all: the tail enters the interval)."""
    skip_if_forced()
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    eng = m.engine
    wav, x, noise = inputs(B, T, 74)
    xb, z = engine_inputs(eng, wav, x, noise)
    with pinned(eng, PINS, restore=("fused_stack", "fused_tail")):
        for (lo, hi), convs in (((6, 11), 1), ((0, 5), 0)):
            eng.set_guidance_interval(lo, hi)
            eng.set_option("fused_stack", 2)
            eng.set_option("fused_tail", 1)
            c0, t0 = eng.launch_counts(), eng.tail_launches
            fused = chain(eng, "cfdg_ddpm_x0", xb, z, False)
            c1 = eng.launch_counts()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, convs) and eng.tail_launches - t0 == S, (lo, hi, c0, c1)
            eng.set_option("fused_stack", 0)
            eng.set_option("fused_tail", 0)
            assert torch.equal(chain(eng, "cfdg_ddpm_x0", xb, z, False), fused), (lo, hi)
        eng.set_guidance_interval()


# ---------------------------------------------------------------------------------------------- 3. captured chains
def test_captured_chain_follows_the_interval():
    """[4, 8], then [2, 9], then the defaults at the same (sampler, B, T): each captured chain equals its eager twin, so no
    graph captured under another interval was replayed; going back replays nothing stale either."""
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    eng = m.engine
    wav, x, noise = inputs(B, T, 75)
    xb, z = engine_inputs(eng, wav, x, noise)
    rolls = {}
    for lo, hi in ((4, 8), (2, 9), (0, -1), (4, 8)):
        eng.set_guidance_interval(lo, hi)
        g = chain(eng, "cfdg_ddpm_x0", xb, z, True)
        g2 = chain(eng, "cfdg_ddpm_x0", xb, None, True, seed=5)          # Philox: per-call scalars from the device block
        e = chain(eng, "cfdg_ddpm_x0", xb, z, False)
        e2 = chain(eng, "cfdg_ddpm_x0", xb, None, False, seed=5)
        assert torch.equal(g, e) and torch.equal(g2, e2), (lo, hi)
        if (lo, hi) in rolls:
            assert torch.equal(rolls[(lo, hi)], g)
        rolls[(lo, hi)] = g
    eng.set_guidance_interval()
    assert not torch.equal(rolls[(4, 8)], rolls[(2, 9)]) and not torch.equal(rolls[(2, 9)], rolls[(0, -1)])


# ---------------------------------------------------------------------------------------------- 4. compositions
def test_with_sampling_steps_vs_restatement():
    """n = 6 visits t = 11, 9, 7, 4, 2, 0: the test uses the real t, so 7 and 4 are guided."""
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    m.hparams.sampling.steps = 6
    m.hparams.sampling.guidance_interval = [4, 8]
    wav, x, noise = inputs(B, T, 76)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, T), noise, 6, w=W, interval=(4, 8))
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    assert ok, d
    traj, _ = m.sample_trajectory(x, wav, noise=noise)                   # dr_step: step t alone follows the rule
    assert traj.shape[0] == 6 and torch.equal(traj[-1], roll)


def test_with_window_overlap_vs_restatement():
    """Three windows of T = 64 frames sharing O = 16: a step is guided or not for all windows alike, and the shared-frame
    mean is taken of whichever prediction the step uses."""
    from diffroll_amd import longform
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    m.hparams.sampling.guidance_interval = [4, 8]
    g = torch.Generator().manual_seed(77)
    L = 150 * HOP
    plan = longform.plan_windows(L, HOP, T=64, overlap=16)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    noise = torch.randn(S, 1, 1, plan.T_c, 88, generator=g)
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    zw = longform.gather_windows(noise.reshape(S, plan.T_c, 88), plan).unsqueeze(2)
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, zw, 0, w=W, interval=(4, 8), plan=plan)
    for use_graph in (True, False):
        win = run_plan_windows(m, plan, wav, x_T, noise, use_graph=use_graph)
        assert_shared_frames_agree(win, plan)
        ok, d = agree(win, ref[:, 0])
        assert ok, (use_graph, d)


def test_with_draws_equals_the_tiled_batch():
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    m.hparams.sampling.guidance_interval = [4, 8]
    wav, x, noise = inputs(2 * B, T, 78)
    wav = wav[:B]
    for kw in (dict(noise=noise), dict(seed=5, first_sample=3)):
        got, _ = m.sample(x, wav, draws=2, **kw)
        ref, _ = m.sample(x, wav.repeat(2, 1), **kw)
        assert torch.equal(got, ref)
        assert not torch.equal(got[0], got[B])
    want = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav.repeat(2, 1), hp, T), noise, 0, w=W, interval=(4, 8))
    got, _ = m.sample(x, wav, draws=2, noise=noise)
    ok, d = agree(got, want)
    assert ok, d


def test_sharded_equals_unsharded():
    """sample_sharded emulated for world size 2 on one device (tests/test_gpu_sharding.py): every rank's engine gets the
    interval from the model it is handed, and the gathered rolls are the unsharded chain's."""
    from diffroll_amd.distributed import sample_sharded_sequential
    hp, p, m, _ = model_of("cfdg_ddpm_x0")
    m.hparams.sampling.guidance_interval = [4, 8]
    wav, x, noise = inputs(3, T, 79)
    for kw in (dict(noise=noise), dict(seed=6)):
        whole, _ = m.sample(x, wav, **kw)
        parts = sample_sharded_sequential(m, x, wav, kw.get("noise"), seed=kw.get("seed", 0), world_size=2)
        assert torch.equal(parts, whole)
    m.hparams.sampling.guidance_interval = None
    full, _ = m.sample(x, wav, seed=6)
    assert not torch.equal(full, whole)


# ---------------------------------------------------------------------------------------------- 5. dr_sample_checked
def test_checked_rerun_uses_the_same_interval():
    """tests/guidance_hook_cases.py in a child process on the "hook" variant of the library (the only build with the
    injected barrier time-out, tests/test_gpu_r3.py): dr_sample_checked's per-phase re-run returns the roll of the SAME
    interval."""
    from diffroll_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build(verbose=False, variant="hook")
    env = dict(os.environ, DR_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "guidance_hook_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-2000:])
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------- 6. full depth
def test_full_depth_across_both_transitions():
    """C = 512, L = 15, k = 9, B = 2, T = 125, [4, 8], fused (fused_stack = 2: two guided clips alone would run per phase):
    the real stack / tail tile shapes - 128-frame blocks, 8 blocks per group - across a transition."""
    skip_if_forced()
    hp = hp_of(channels=512, layers=15, k=9)
    hp, p, m, _ = model_of("cfdg_ddpm_x0", hp=hp, seed=3)
    m.hparams.sampling.guidance_interval = [4, 8]
    wav, x, noise = inputs(B, T, 80)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, T), noise, 0, w=W, interval=(4, 8))
    eng = m.engine
    eng.set_option("fused_stack", 2)
    try:
        c0, t0 = eng.launch_counts(), eng.tail_launches
        roll, _ = m.sample(x, wav, noise=noise, use_graph=False)
        c1, st = eng.launch_counts(), eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches - t0 == S, st
        assert c1[0] - c0[0] == 1 and c1[1] - c0[1] == 0, (c0, c1)
        captured, _ = m.sample(x, wav, noise=noise)
    finally:
        eng.set_option("fused_stack", 1)
    ok, d = agree(roll, ref)
    print(f"\nfull depth [4, 8]: max |d| = {d:.3g}")
    assert ok, d
    assert torch.equal(captured, roll)
