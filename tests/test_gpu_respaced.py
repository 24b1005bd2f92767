"""Respaced sampling on the MI355X (option "sampling_steps", hparams.sampling.steps): the HIP chain on n of the S steps
against the CPU restatement of tests/chain_ref.py - one sampler per coefficient family, injected and Philox noise,
n in {2, 20, 50}, a full-depth BASELINE config 2 guided batch, long-form windows, the trained proxy - and the bit
identities the option promises (n = S is the full chain; graph = eager; fused stack + tail = per-phase; dr_step over the
visited steps = dr_sample)."""
import json

import pytest
import torch

from oracle import diffroll_ref as R
from testlib import ATOL, HOP, S, agree, assert_shared_frames_agree, ckpt_path, hp_of, inputs, load_trained, make_model, maxdiff, run_plan_windows, trained_noise, trained_params

import chain_ref as CR

pytestmark = pytest.mark.gpu


def test_option_is_public_and_validated():
    hp = hp_of(layers=2)
    m = make_model(hp, R.synthetic_params(hp, seed=1), sampler="generation_ddpm_x0")
    eng = m.engine
    eng.set_option("sampling_steps", 50)             # DR_ENAME (-> ValueError) before the option existed
    assert eng.sampling_steps == 50 and eng.visited_steps() == CR.visited(S, 50)
    for bad in (1, -1, S + 1):
        with pytest.raises(ValueError):
            eng.set_option("sampling_steps", bad)
    assert eng.sampling_steps == 50
    # dr_step: a step the respaced chain does not visit is refused, a visited one runs
    x = torch.randn(2, 40, 88, device=eng.device)
    with pytest.raises(ValueError, match="not visited"):
        eng.step("generation_ddpm_x0", x, None, 198)
    eng.step("generation_ddpm_x0", x, None, 195)
    eng.finish()
    eng.set_option("sampling_steps", S)
    eng.step("generation_ddpm_x0", x, None, 198)
    eng.set_option("sampling_steps", 0)
    eng.finish()


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "cfdg_ddim_x0", "ddpm", "ddim", "ddim2ddpm"])
def test_respaced_chain_vs_restatement(sampler):
    """One sampler per coefficient family (DR_COEF_*), n in {2, 20, 50}, injected noise and Philox."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=60)
    m = make_model(hp, p, sampler=sampler, w=0.5)
    B, Tn = 2, 40
    wav, x, noise = inputs(B, Tn, 61)
    spec = R.frontend(wav, hp, Tn)
    w = 0.5 if sampler.startswith("cfdg") else 0.0
    zp = CR.philox_noise(9, 0, S, B, Tn)
    for n in (2, 20, 50):
        m.hparams.sampling.steps = n
        for z, kw in ((noise, dict(noise=noise)), (zp, dict(seed=9))):
            ref = CR.sample_chain(p, hp, sampler, x, spec, z, n, w=w)
            roll, _ = m.sample(x, wav, **kw)
            ok, d = agree(roll, ref)
            assert ok, (n, "injected" if "noise" in kw else "philox", d)


def test_respaced_split_bf16_vs_restatement():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=62)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    m.hparams.sampling.steps = 20
    wav, x, noise = inputs(2, 40, 63)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), noise, 20, w=0.5)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    assert ok, d


def test_full_depth_config2_guided_batch_at_50_steps():
    """The k = 9, C = 512, 15-layer network on 4-s clips (BASELINE config 2 geometry), cfdg_ddpm_x0 w = 0.5, n = 50."""
    hp = hp_of(channels=512, layers=15)
    p = R.synthetic_params(hp, seed=3)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.hparams.sampling.steps = 50
    wav, x, noise = inputs(2, 125, 64)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 125), noise, 50, w=0.5)
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, ref)
    assert ok, d


def test_bit_identities_on_the_fused_path():
    """At the bench geometry (16 guided clips x 125 frames: fused stack + tail kernel): n = S equals the option off, and
    at n = 50 the captured chain equals the eager one and the per-phase launches (pinned to the flavours the fused kernels
    are built from, as tests/test_gpu_fused.py does), with injected noise and with Philox."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=512, layers=3)
    p = R.synthetic_params(hp, seed=11)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    wav, x, noise = inputs(16, 125, 65)
    eng = m.engine
    off, _ = m.sample(x, wav, noise=noise)
    m.hparams.sampling.steps = S
    full, _ = m.sample(x, wav, noise=noise)
    assert eng.sampling_steps == S and torch.equal(full, off)
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3202, 0), "tune.pw_nw": (4, 0), "tune.stack_fl": (2, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        m.hparams.sampling.steps = 50
        t0 = eng.tail_launches
        g, _ = m.sample(x, wav, noise=noise)
        st = eng.launch_state()
        assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
        e, _ = m.sample(x, wav, noise=noise, use_graph=False)
        gp, _ = m.sample(x, wav, seed=5)
        ep, _ = m.sample(x, wav, seed=5, use_graph=False)
        eng.set_option("fused_stack", 0)
        pp, _ = m.sample(x, wav, noise=noise)
        ppp, _ = m.sample(x, wav, seed=5)
        st = eng.launch_state()
        assert st["mode"] == "per_phase" and st["fallbacks"] == 0 and st["yields"] == 0, st
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
    assert torch.equal(g, e) and torch.equal(gp, ep)
    assert torch.equal(g, pp) and torch.equal(gp, ppp)
    assert not torch.equal(g, off)


def test_dr_step_over_the_visited_steps_equals_dr_sample():
    """sample_trajectory (dr_step at every visited t) ends bit for bit where sample() ends, with n rows; the reference's
    single-step methods keep their stride-1 meaning under a respaced config."""
    hp = hp_of()
    p = R.synthetic_params(hp, seed=66)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    wav, x, noise = inputs(2, 40, 67)
    one_off, _ = m.cfdg_ddpm_x0(x, wav, 198, noise=noise[198])
    m.hparams.sampling.steps = 20
    traj, _ = m.sample_trajectory(x, wav, noise=noise)
    roll, _ = m.sample(x, wav, noise=noise)
    assert traj.shape == (20,) + tuple(roll.shape) and torch.equal(traj[-1], roll)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), noise, 20, w=0.5, trajectory=True)
    assert maxdiff(traj.cpu(), ref) <= ATOL
    traj, _ = m.sample_trajectory(x, wav, seed=4, first_sample=1)
    roll, _ = m.sample(x, wav, seed=4, first_sample=1)
    assert torch.equal(traj[-1], roll)
    one_on, _ = m.cfdg_ddpm_x0(x, wav, 198, noise=noise[198])        # 198 is not a visited step: stride 1 regardless
    assert torch.equal(one_on, one_off)
    assert m._engine.sampling_steps == 0                               # (m.engine would set it back)
    roll2, _ = m.sample(x, wav, seed=4, first_sample=1)               # ... and the chain is respaced again
    assert m.engine.sampling_steps == 20 and torch.equal(roll2, roll)


def test_sample_long_at_50_steps_vs_restatement():
    from diffroll_amd import longform
    from oracle import philox
    hp = hp_of(channels=128, layers=3)
    p = R.synthetic_params(hp, seed=68)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    m.hparams.sampling.steps = 50
    g = torch.Generator().manual_seed(68)
    L = 1400 * HOP - 100
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    seed, rec = 21, 2
    z = {t: longform.gather_windows(torch.from_numpy(philox.step_noise(seed, rec, 1, plan.T_c * 88, t)).reshape(plan.T_c, 88),
                                    plan).unsqueeze(1)
         for t in CR.visited(S, 50) if t > 0}
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 50, w=0.5, plan=plan)
    win = run_plan_windows(m, plan, wav, x_T, None, seed=seed, recording=rec)
    assert_shared_frames_agree(win, plan)
    ok, d = agree(win, ref[:, 0])
    assert ok, d
    roll = m.sample_long(wav, overlap=160, seed=seed, recording=rec, x_T=x_T).cpu()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))
    assert m.engine.window_overlap == 0 and m.engine.sampling_steps == 50


@pytest.mark.parametrize("n", [20, 50])
def test_trained_proxy_thresholded_roll(golden_dir, n):
    """tests/golden/trained_small.ckpt at n steps: the HIP thresholded roll equals the restatement's.  The F1 is
    reported, not asserted: this proxy task is too easy to show a quality cost of fewer steps."""
    from diffroll_amd import ClassifierFreeDiffRoll
    gd = load_trained(golden_dir)
    hp = json.loads(str(gd["hp"]))
    _, p = trained_params(golden_dir, gd)
    x_T, noise = trained_noise(gd)
    wav, label = torch.from_numpy(gd["wav"]), torch.from_numpy(gd["label"])
    w = float(gd["w"])
    m = ClassifierFreeDiffRoll.load_from_checkpoint(ckpt_path(golden_dir), sampling={"type": "cfdg_ddpm_x0", "w": w, "steps": n})
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x_T, R.frontend(wav, hp, x_T.shape[2]), noise, n, w=w)
    roll, _ = m.sample(x_T, wav, noise=noise)
    thr = float(gd["frame_threshold"])
    assert torch.equal(roll.cpu() > thr, ref > thr)
    assert maxdiff(roll.cpu(), ref) <= ATOL
    out = m.test_step({"frame": label, "audio": wav, "x_T": x_T, "noise": noise}, 1)
    pred, lab = ref[:, 0] > thr, label[:, :ref.shape[2]] > 0.5
    assert (out["tp"], out["fp"], out["fn"]) == (int((pred & lab).sum()), int((pred & ~lab).sum()), int((~pred & lab).sum()))
    print(f"\ntrained proxy, {n} of {S} steps: TP/FP/FN {out['tp']}/{out['fp']}/{out['fn']}, Frame-F1 {out['Test/Frame_F1']:.4f} "
          f"(200 steps: {int(gd['tp'])}/{int(gd['fp'])}/{int(gd['fn'])}, {float(gd['frame_f1']):.4f})")
