"""Long-form transcription on the MI355X: jointly sampled windows (option "window_overlap", ClassifierFreeDiffRoll.sample_long,
the CLI's max_segment_samples=null) against an oracle composed here from oracle.diffroll_ref - per-window front-end,
denoise cond / uncond, combine, the shared-frame mean, posterior_update - in the per-phase and the fused (stack_kernel +
tail kernel with its neighbour wait) launch modes, captured and eager."""
import math

import numpy as np
import pytest
import torch

from oracle import diffroll_ref as R
from oracle import philox
from testlib import ATOL, HOP, assert_shared_frames_agree, long_hp_of, make_model, maxdiff, oracle_long, run_plan_windows

from diffroll_amd import longform

pytestmark = pytest.mark.gpu


def test_joint_windows_against_the_oracle_per_phase_fused_graph_eager():
    hp = long_hp_of()
    p = R.synthetic_params(hp, seed=1400)
    g = torch.Generator().manual_seed(1400)
    L = 1400 * HOP - 100                              # ~2.2 windows: n = 3 at O = 160
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    noise = torch.randn(4, 1, 1, plan.T_c, 88, generator=g)
    ref = oracle_long(p, hp, "cfdg_ddpm_x0", plan, wav, x_T, noise, 0.5)
    ref_roll = longform.stitch(ref[:, 0], plan)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    # the per-phase launches pinned to the flavours the fused 160-frame kernels are built from (no split-K), as
    # tests/test_gpu_fused.py does: only then are the two launch modes the same arithmetic (process-wide knobs: restored)
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3205, 0), "tune.pw_nw": (5, 0), "tune.stack_fl": (5, 0)}
    for k, (v, _) in pins.items():
        eng.set_option(k, v)
    try:
        _joint_windows_cases(m, eng, hp, p, plan, wav, x_T, noise, ref, ref_roll, L)
    finally:
        for k, (_, v) in pins.items():
            eng.set_option(k, v)
        eng.set_option("fused_stack", 1)
    del m
    # split-bf16, per-phase
    mb = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    mb.engine.set_option("fused_stack", 0)
    bb = run_plan_windows(mb, plan, wav, x_T, noise)
    d = maxdiff(bb, ref[:, 0])
    assert d <= ATOL, ("bf16x3", d)
    assert_shared_frames_agree(bb, plan)


def _joint_windows_cases(m, eng, hp, p, plan, wav, x_T, noise, ref, ref_roll, L):
    # per-phase
    eng.set_option("fused_stack", 0)
    pp = run_plan_windows(m, plan, wav, x_T, noise)
    d = maxdiff(pp, ref[:, 0])
    assert d <= ATOL, ("per-phase", d)
    assert torch.equal(pp > 0.5, ref[:, 0] > 0.5)
    assert_shared_frames_agree(pp, plan)
    long_roll = m.sample_long(wav, overlap=160, x_T=x_T, noise=noise)
    assert long_roll.shape == (1, 1, plan.T_out, 88) == (1, 1, math.ceil(L / HOP), 88)
    assert torch.equal(long_roll.cpu()[0, 0], longform.stitch(pp, plan))
    assert maxdiff(long_roll.cpu()[0, 0], ref_roll) <= ATOL
    # forced fused: the 160-frame stack flavour, the tail kernel with the neighbour wait
    eng.set_option("fused_stack", 2)
    eng.profile_enable(True)                           # (a profiled chain runs eager)
    fe = run_plan_windows(m, plan, wav, x_T, noise)
    _, _, _, kname = eng.profile_read_ex()
    eng.profile_enable(False)
    st = eng.launch_state()
    assert st["mode"] == "fused_stack+tail", st
    assert kname.startswith("stack_kernel<5>"), kname
    fg = run_plan_windows(m, plan, wav, x_T, noise, use_graph=True)
    st = eng.launch_state()
    assert st["fallbacks"] == 0 and st["yields"] == 0, st
    assert maxdiff(fe, ref[:, 0]) <= ATOL
    assert torch.equal(fe, pp), maxdiff(fe, pp)       # fused == per-phase, bit for bit
    assert torch.equal(fg, fe), maxdiff(fg, fe)       # graph == eager
    assert_shared_frames_agree(fg, plan)
    eng.set_option("fused_stack", 0)
    pe = run_plan_windows(m, plan, wav, x_T, noise, use_graph=False)
    assert torch.equal(pe, pp)


def test_philox_keys_by_canvas_element_and_anchor_to_sample():
    hp = long_hp_of(layers=3, steps=4, channels=128)
    p = R.synthetic_params(hp, seed=33)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    g = torch.Generator().manual_seed(33)
    L = 1100 * HOP
    plan = longform.plan_windows(L, HOP, overlap=160)
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    seed, rec = 0x0123456789AB, 7
    got = m.sample_long(wav, overlap=160, seed=seed, recording=rec, x_T=x_T).cpu()
    z = np.zeros((4, 1, 1, plan.T_c, 88), dtype=np.float32)
    for t in range(1, 4):
        z[t] = philox.step_noise(seed, rec, 1, plan.T_c * 88, t).reshape(1, 1, plan.T_c, 88)
    inj = m.sample_long(wav, overlap=160, seed=seed, recording=rec, x_T=x_T, noise=torch.from_numpy(z)).cpu()
    # (the numpy replay's Box-Muller rounds log / sincos differently from the device's in the last bits, as in
    # test_gpu_parity.py's Philox test: same keys, agreement to fp32 rounding)
    assert maxdiff(got, inj) <= ATOL and torch.equal(got > 0.5, inj > 0.5)
    # ... and the keys are the canvas's: the per-window keying (sample = recording + b) draws different noise
    zw = np.zeros((4, plan.n, 640 * 88), dtype=np.float32)
    for t in range(1, 4):
        zw[t] = philox.step_noise(seed, rec, plan.n, 640 * 88, t)
    zc = z.reshape(4, plan.T_c, 88)
    zwin = longform.gather_windows(torch.from_numpy(zc), plan).numpy().reshape(4, plan.n, 640 * 88)
    assert np.array_equal(zwin[:, 0], zw[:, 0]) and not np.allclose(zwin[1:, 1], zw[1:, 1])
    # n = 1: sample_long == sample() on crop_or_pad(recording), first_sample = recording, sliced to T_out
    from diffroll_amd.audio import crop_or_pad
    L1 = 300 * HOP + 17
    w1 = 0.1 * torch.randn(L1, generator=g)
    x1 = torch.randn(1, 1, 640, 88, generator=g)
    before, _ = m.sample(x1, crop_or_pad(w1, 640 * HOP)[None], seed=seed, first_sample=rec)
    before = before.cpu()
    one = m.sample_long(w1, overlap=160, seed=seed, recording=rec, x_T=x1).cpu()
    T_out = math.ceil(L1 / HOP)
    assert one.shape == (1, 1, T_out, 88)
    assert torch.equal(one, before[:, :, :T_out]), maxdiff(one, before[:, :, :T_out])
    # the engine is left as found: the same sample() after sample_long gives the same bits
    after, _ = m.sample(x1, crop_or_pad(w1, 640 * HOP)[None], seed=seed, first_sample=rec)
    assert torch.equal(after.cpu(), before)
    assert m.engine.window_overlap == 0
    # inpainting is refused, and so is an overlap beyond half the window
    with pytest.raises(ValueError):
        m.sample_long(w1, overlap=321)
    mi = make_model(hp, p, sampler="inpainting_ddpm_x0", w=0.5, inpainting_t=[10, 20])
    with pytest.raises(ValueError, match="inpainting"):
        mi.sample_long(w1)


def test_engine_rejects_overlap_beyond_half_the_window():
    from diffroll_amd.engine import EngineError
    hp = long_hp_of(layers=2, steps=4, channels=64)
    p = R.synthetic_params(hp, seed=5)
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    eng = m.engine
    x = torch.zeros(2, 64, 88, device=eng.device)
    eng.set_option("window_overlap", 33)
    try:
        with pytest.raises((EngineError, ValueError)):
            eng.sample("generation_ddpm_x0", x, None, 0.0, 0, 0, False, True)
    finally:
        eng.set_option("window_overlap", 0)
    eng.sample("generation_ddpm_x0", x, None, 0.0, 0, 0, False, True)


def test_long_generation_keeps_shared_frames_equal():
    hp = long_hp_of(layers=4, steps=4)
    p = R.synthetic_params(hp, seed=1500)
    m = make_model(hp, p, sampler="generation_ddpm_x0")
    plan = longform.plan_windows(1500, None, overlap=160)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=torch.Generator().manual_seed(15))
    win = run_plan_windows(m, plan, None, x_T, None, seed=3, recording=1)
    assert_shared_frames_agree(win, plan)
    roll = m.sample_long(frames=1500, overlap=160, seed=3, recording=1, x_T=x_T).cpu()
    assert roll.shape == (1, 1, 1500, 88) and torch.isfinite(roll).all()
    assert torch.equal(roll[0, 0], longform.stitch(win, plan))


def test_cli_transcribes_whole_files(tmp_path):
    from scipy.io import wavfile
    from diffroll_amd import cli, midi
    wav_dir = tmp_path / "audio"
    wav_dir.mkdir()
    rng = np.random.default_rng(9)
    lengths = {"long": 30 * 16000 + 123, "short": 8 * 16000}
    for stem, L in lengths.items():
        wavfile.write(str(wav_dir / f"{stem}.wav"), 16000, (0.1 * rng.standard_normal(L)).astype(np.float32))
    out = tmp_path / "out"
    cli.main(["task=transcription", "dataset=Custom", f"dataset.args.audio_path={wav_dir}", "dataset.args.audio_ext=wav",
              "dataset.args.max_segment_samples=null", "task.timesteps=4", "model.args.residual_layers=3",
              "model.args.residual_channels=128", f"output_dir={out}"])
    m = None
    for stem, L in lengths.items():
        roll = np.load(out / f"roll_{stem}.npy")
        assert roll.shape == (1, 1, math.ceil(L / HOP), 88) and np.isfinite(roll).all()
        assert (out / f"clean_midi_{stem}.mid").exists()
        if m is None:
            hp = long_hp_of(layers=2, steps=4, channels=64)
            m = make_model(hp, R.synthetic_params(hp, seed=0))
        pitches, iv = midi.extract_notes_wo_velocity(m.engine, torch.from_numpy(roll))[0]
        ons = sorted((int(p) + midi.MIN_MIDI, int(float(a) * (HOP / 16000.0) * midi.TICKS_PER_SECOND))
                     for p, (a, _) in zip(pitches, iv.astype(np.float64)))
        ev = midi.read_midi_notes(str(out / f"raw_midi_{stem}.mid"))
        got = sorted((e[2], e[0]) for e in ev if (e[1] & 0xF0) == 0x90 and e[3] > 0)
        assert got == ons, stem
