"""Several recordings in one long-form chain on the MI355X (option "window_break", ClassifierFreeDiffRoll.sample_long_batch,
the CLI's task.recordings_per_chain): against the joint-chain oracle of tests/test_gpu_longform.py run independently per
recording, against solo sample_long chains, and the engine-level contract of the marks (graph reuse, errors, hygiene)."""
import math

import numpy as np
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import assert_shared_frames_agree, long_hp_of, make_model, maxdiff, oracle_long
from tuning_pins import pinned

from diffroll_amd import longform

pytestmark = pytest.mark.gpu

ATOL = 1e-5            # the project's chain tolerance
HOP = 512
W = 640 * HOP
# the per-phase launches pinned to the flavours the fused 160-frame kernels are built from (no split-K), as
# tests/test_gpu_longform.py does: only then are the launch modes the same arithmetic (process-wide knobs: restored)
PINS = {"tune.ksplit_max": (1, 16), "tune.tile": (3205, 0), "tune.pw_nw": (5, 0), "tune.stack_fl": (5, 0)}


def run_batch(m, batch, wavs, x_T, noise, marks=None, seed=0, first=0, use_graph=True):
    """sample_long_batch's chain, keeping the windows: (n, T, 88) on the host.  marks: None = the batch plan's, or a list (an
    empty one = set and then cleared with "window_break" = 0).  An overlap the caller has set is the plan's: left alone."""
    if marks is not None and not marks:
        m.engine.set_option("window_break", 1)
        m.engine.set_option("window_break", 0)
    return m._sample_windows(batch, wavs, x_T, noise, 1, seed, first, use_graph, True, marks=marks).cpu()


_FULL = {}


def full_size_case():
    """The one full-size case (15 layers, C = 512, k = 9, guided, 4 steps, injected noise): recordings of 2 + 1 + 1
    windows and the oracle's windows of each, computed once for the two tests that use them."""
    if _FULL:
        return _FULL
    hp = long_hp_of()
    p = R.synthetic_params(hp, seed=1400)
    # The rolls of the synthetic network as drawn are spread evenly across the 0.5 threshold (mean 0.03, std 0.35: about
    # 11 of the 225 280 elements within 1e-4 of it whatever the input seed - 28 seeds gave margins of 2.4e-7 .. 3.2e-5), so
    # no choice of seed alone can keep every element 1e-4 away.  The output bias is a free choice of this test: 80 of
    # the 88 pitches are moved clear of the threshold (odd pitches + 2: always on, even ones - 2: always off; measured
    # margin 0.27), as a trained model's mostly-decided rolls are, and every 11th pitch (8 of them) keeps the drawn bias,
    # input-dependent with about 11 % of its frames on.  A bias adds no rounding error of its own.  Among the input seeds
    # 2114 .. 2119, searched on the CPU, 2117 and 2119 meet the precondition; 2119 has the wider margin (2.3e-4).
    pitch = torch.arange(88)
    p["output_projection.bias"] = p["output_projection.bias"] + torch.where(
        pitch % 11 == 0, torch.zeros(88), torch.where(pitch % 2 == 1, torch.full((88,), 2.0), torch.full((88,), -2.0)))
    g = torch.Generator().manual_seed(2119)
    lengths = [W + 200 * HOP - 77, W - 90 * HOP, 300 * HOP + 5]
    batch = longform.plan_batch(lengths, HOP, overlap=160)
    assert [q.n for q in batch.plans] == [2, 1, 1] and batch.marks == [2, 3]
    wavs = [0.1 * torch.randn(L, generator=g) for L in lengths]
    x_T = [torch.randn(1, 1, q.T_c, 88, generator=g) for q in batch.plans]
    noise = [torch.randn(4, 1, 1, q.T_c, 88, generator=g) for q in batch.plans]
    # every recording on its own: the oracle never sees the batch
    ref = [oracle_long(p, hp, "cfdg_ddpm_x0", q, wv, x, z, 0.5)[:, 0] for q, wv, x, z in zip(batch.plans, wavs, x_T, noise)]
    # precondition: no oracle element within 1e-4 of the threshold, so the thresholded rolls cannot differ for a rounding
    # reason (max |delta| <= 1e-5)
    margin = min(float((r - 0.5).abs().min()) for r in ref)
    print(f"full-size case: min |oracle - 0.5| = {margin:.3e}")
    assert margin > 1e-4, margin
    _FULL.update(hp=hp, p=p, batch=batch, lengths=lengths, wavs=wavs, x_T=x_T, noise=noise, ref=ref)
    return _FULL


def check_against_oracle(win, c, what):
    batch = c["batch"]
    for r, (f, q) in enumerate(zip(batch.first, batch.plans)):
        mine = win[f:f + q.n]
        d = maxdiff(mine, c["ref"][r])
        print(f"{what}, recording {r}: max |delta| = {d:.3e}")
        assert d <= ATOL, (what, r, d)
        assert torch.equal(mine > 0.5, c["ref"][r] > 0.5), (what, r)
        assert_shared_frames_agree(mine, q)


def test_three_recordings_against_the_oracle_per_phase_fused_graph():
    """The full-size case in every launch mode (its precondition is asserted where the case is built)."""
    c = full_size_case()
    batch, wavs, x_T, noise = c["batch"], c["wavs"], c["x_T"], c["noise"]
    m = make_model(c["hp"], c["p"], sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    # nothing forced: 4 windows x 2 evaluations x 32 blocks = 256 blocks, the plan fuses on its own
    eng.profile_enable(True)                               # (a profiled chain runs eager)
    de = run_batch(m, batch, wavs, x_T, noise)
    _, _, _, kname = eng.profile_read_ex()
    eng.profile_enable(False)
    st = eng.launch_state()
    assert st["mode"] == "fused_stack+tail", st
    assert kname.startswith("stack_kernel<5>"), kname
    dg = run_batch(m, batch, wavs, x_T, noise, use_graph=True)
    st = eng.launch_state()
    assert st["mode"] == "fused_stack+tail" and st["fallbacks"] == 0 and st["yields"] == 0, st
    check_against_oracle(de, c, "default plan, eager")
    check_against_oracle(dg, c, "default plan, graph")
    # the façade returns the stitched rolls of the same windows
    rolls = m.sample_long_batch(wavs, overlap=160, x_T=x_T, noise=noise)
    for r, (f, q) in enumerate(zip(batch.first, batch.plans)):
        assert rolls[r].shape == (1, 1, q.T_out, 88) == (1, 1, math.ceil(c["lengths"][r] / HOP), 88)
        assert torch.equal(rolls[r].cpu()[0, 0], longform.stitch(dg[f:f + q.n], q))
    assert eng.window_overlap == 0 and eng.window_breaks == ()
    with pinned(eng, PINS):
        eng.set_option("fused_stack", 0)
        pp = run_batch(m, batch, wavs, x_T, noise)
        check_against_oracle(pp, c, "per-phase")
        eng.set_option("fused_stack", 2)
        eng.profile_enable(True)
        fe = run_batch(m, batch, wavs, x_T, noise)
        _, _, _, kname = eng.profile_read_ex()
        eng.profile_enable(False)
        assert eng.launch_state()["mode"] == "fused_stack+tail" and kname.startswith("stack_kernel<5>"), kname
        fg = run_batch(m, batch, wavs, x_T, noise, use_graph=True)
        st = eng.launch_state()
        assert st["fallbacks"] == 0 and st["yields"] == 0, st
        check_against_oracle(fe, c, "forced fused, eager")
        check_against_oracle(fg, c, "forced fused, graph")
        assert torch.equal(fe, pp), maxdiff(fe, pp)       # fused == per-phase, bit for bit
        assert torch.equal(fg, fe), maxdiff(fg, fe)       # graph == eager


def test_the_boundary_is_real():
    """Same inputs.  With the marks, recording A's last window and recording B's window do not exchange anything on the
    frames that neighbouring windows of ONE recording would share; with the marks cleared ("window_break" = 0) the batch
    is what sample_long's engine call makes of it - four consecutive windows of one recording, every neighbouring pair
    averaged - and at t = 0 (x = y / c2) the shared frames of every pair come out equal, bit for bit."""
    c = full_size_case()
    batch, wavs, x_T, noise = c["batch"], c["wavs"], c["x_T"], c["noise"]
    m = make_model(c["hp"], c["p"], sampler="cfdg_ddpm_x0", w=0.5)
    H, O = 480, 160
    one = longform.plan_windows(3 * H + 640, None, overlap=O)          # the geometry of a 4-window recording
    assert one.n == 4
    marked = run_batch(m, batch, wavs, x_T, noise)
    a_end, b_start = marked[1, H:], marked[2, :O]
    assert not torch.equal(a_end, b_start)
    # they are the solo results (test above), not the mean: far from each other
    assert maxdiff(a_end, b_start) > 100 * ATOL
    assert maxdiff(marked[1], c["ref"][0][1]) <= ATOL and maxdiff(marked[2], c["ref"][1][0]) <= ATOL
    cleared = run_batch(m, batch, wavs, x_T, noise, marks=[])          # marks set, then "window_break" = 0
    assert_shared_frames_agree(cleared, one)
    assert maxdiff(cleared[1, H:], c["ref"][0][1][H:]) > 100 * ATOL    # A's tail now depends on B
    # ... and equals an engine that never had marks: exactly sample_long's call for a 4-window recording
    m2 = make_model(c["hp"], c["p"], sampler="cfdg_ddpm_x0", w=0.5)
    eng2 = m2.engine
    xb = longform.gather_batch([x.reshape(q.T_c, 88).to(eng2.device) for x, q in zip(x_T, batch.plans)], batch)
    z = longform.gather_batch([zr.reshape(4, q.T_c, 88).to(eng2.device) for zr, q in zip(noise, batch.plans)], batch).contiguous()
    eng2.frontend(torch.cat([longform.window_audio(wv, q, HOP) for wv, q in zip(wavs, batch.plans)]), 640)
    eng2.set_option("window_overlap", O)
    try:
        eng2.sample("cfdg_ddpm_x0", xb, z, 0.5, 0, 0, True, True)
    finally:
        eng2.set_option("window_overlap", 0)
    assert torch.equal(xb.cpu(), cleared)


def small_case(seed=33):
    hp = long_hp_of(layers=3, steps=4, channels=128)
    p = R.synthetic_params(hp, seed=seed)
    g = torch.Generator().manual_seed(seed)
    lengths = [W + 100 * HOP + 3, 300 * HOP + 17, 1400 * HOP - 100]     # 2, 1 (in the middle) and 3 windows
    wavs = [0.1 * torch.randn(L, generator=g) for L in lengths]
    return hp, p, lengths, wavs


def test_batch_equals_solo_chains_with_philox_noise():
    hp, p, lengths, wavs = small_case()
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    seed = 0x0123456789AB
    assert [q.n for q in longform.plan_batch(lengths, HOP).plans] == [2, 1, 3]

    def both():
        got = [r.cpu() for r in m.sample_long_batch(wavs, seed=seed, first_recording=7)]
        solo = [m.sample_long(wv, seed=seed, recording=7 + i).cpu() for i, wv in enumerate(wavs)]
        return got, solo

    with pinned(eng, PINS):
        for mode in (0, 2):                                   # per-phase, forced fused
            eng.set_option("fused_stack", mode)
            got, solo = both()
            for i, (a, b) in enumerate(zip(got, solo)):
                assert a.shape == b.shape == (1, 1, math.ceil(lengths[i] / HOP), 88)
                assert torch.equal(a, b), (mode, i, maxdiff(a, b))
    got, solo = both()                                        # the default plan of each chain
    for i, (a, b) in enumerate(zip(got, solo)):
        d = maxdiff(a, b)
        print(f"default plan, recording {i}: batch vs solo max |delta| = {d:.3e}")
        assert d <= ATOL and torch.equal(a > 0.5, b > 0.5), (i, d)
    # the recordings are not each other's noise: recording 7 + i, not 7
    other = m.sample_long(wavs[1], seed=seed, recording=7).cpu()
    assert not torch.equal(other, solo[1])
    # generation: frame counts instead of waveforms
    mg = make_model(hp, p, sampler="generation_ddpm_x0")
    frames = [700, 300, 1500]
    gg = mg.sample_long_batch(frames=frames, seed=5, first_recording=2)
    for i, f in enumerate(frames):
        s = mg.sample_long(frames=f, seed=5, recording=2 + i)
        assert gg[i].shape == (1, 1, f, 88)
        assert maxdiff(gg[i].cpu(), s.cpu()) <= ATOL and torch.equal(gg[i] > 0.5, s > 0.5)


def test_new_marks_replay_the_captured_chain():
    hp, p, _, _ = small_case(seed=41)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    g = torch.Generator().manual_seed(41)
    # the same four windows of audio and x_T under three segmentations: only the marks change
    batch = longform.plan_batch([W] * 4, HOP, overlap=160)
    wavs = [0.1 * torch.randn(W, generator=g) for _ in range(4)]
    x_T = [torch.randn(1, 1, 640, 88, generator=g) for _ in range(4)]
    eng.set_option("window_overlap", 160)
    try:
        captures = []
        for marks in ([2, 3], [1, 2], []):
            eager = run_batch(m, batch, wavs, x_T, None, marks=marks, seed=9, first=3, use_graph=False)
            graph = run_batch(m, batch, wavs, x_T, None, marks=marks, seed=9, first=3, use_graph=True)
            assert torch.equal(graph, eager), (marks, maxdiff(graph, eager))
            st = eng.launch_state()
            captures.append((eng.cold_times()[3], st["stack_launches"], st["tail_launches"]))
        # one capture served all three: capture time and the launch counts (a captured launch counts once, at capture;
        # the eager chains in between add the same number each round)
        assert captures[0][0] == captures[1][0] == captures[2][0], captures
        assert captures[1][1] - captures[0][1] == captures[2][1] - captures[1][1], captures
        assert captures[1][2] - captures[0][2] == captures[2][2] - captures[1][2], captures
        # the segmentations differ where they should: window 1 | 2 is a boundary under [2, 3] and [1, 2] only
        a = run_batch(m, batch, wavs, x_T, None, marks=[2, 3], seed=9, first=3)
        b = run_batch(m, batch, wavs, x_T, None, marks=[1, 2], seed=9, first=3)
        assert torch.equal(a[0, 480:], a[1, :160]) and not torch.equal(b[0, 480:], b[1, :160])
        assert torch.equal(b[2, 480:], b[3, :160]) and not torch.equal(a[2, 480:], a[3, :160])
    finally:
        eng.set_option("window_overlap", 0)


def test_errors_and_hygiene():
    from diffroll_amd.audio import crop_or_pad
    from diffroll_amd.engine import EngineError
    hp, p, lengths, wavs = small_case(seed=52)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    g = torch.Generator().manual_seed(52)
    x1 = torch.randn(2, 1, 640, 88, generator=g)
    w1 = torch.stack([crop_or_pad(wavs[0], W), crop_or_pad(wavs[1], W)])
    before, _ = m.sample(x1, w1, seed=11, first_sample=4)
    before = before.cpu()
    # a mark that is not a window of the batch
    eng.frontend(w1, 640)
    m._fe_key = None
    xw = x1[:, 0].to(eng.device).contiguous()
    eng.set_option("window_overlap", 160)
    try:
        eng.set_option("window_break", 2)
        with pytest.raises((EngineError, ValueError), match="window_break 2"):
            eng.sample("cfdg_ddpm_x0", xw, None, 0.5, 0, 0, False, True)
        eng.set_option("window_break", 0)
        eng.set_option("window_break", 1)
        eng.sample("cfdg_ddpm_x0", xw, None, 0.5, 0, 0, False, True)
        with pytest.raises((EngineError, ValueError)):
            eng.set_option("window_break", -1)
        assert eng.window_breaks == (1,)
    finally:
        eng.set_option("window_break", 0)
        eng.set_option("window_overlap", 0)
    assert eng.window_breaks == ()
    # marks are ignored while "window_overlap" is 0, even ones beyond the batch
    eng.set_option("window_break", 5)
    try:
        ignored, _ = m.sample(x1, w1, seed=11, first_sample=4)
    finally:
        eng.set_option("window_break", 0)
    assert torch.equal(ignored.cpu(), before)
    # the façade leaves the engine as it found it
    m.sample_long_batch(wavs, seed=1)
    assert eng.window_overlap == 0 and eng.window_breaks == ()
    after, _ = m.sample(x1, w1, seed=11, first_sample=4)
    assert torch.equal(after.cpu(), before)
    # too many windows for one chain; wrong argument kinds; inpainting
    with pytest.raises(ValueError, match="MAX_WINDOWS"):
        m.sample_long_batch([torch.zeros(W)] * (longform.MAX_WINDOWS + 1))
    with pytest.raises(ValueError):
        m.sample_long_batch(frames=[700])
    with pytest.raises(ValueError):
        m.sample_long_batch(wavs, x_T=[torch.zeros(1, 1, 640, 88)])
    mi = make_model(hp, p, sampler="inpainting_ddpm_x0", w=0.5, inpainting_t=[10, 20])
    with pytest.raises(ValueError, match="inpainting"):
        mi.sample_long_batch(wavs)


def test_cli_groups_recordings_into_chains(tmp_path):
    from scipy.io import wavfile
    from diffroll_amd import cli
    from diffroll_amd.audio import ingest
    wav_dir = tmp_path / "audio"
    wav_dir.mkdir()
    rng = np.random.default_rng(12)
    lengths = {"a_long": 30 * 16000 + 123, "b_short": 8 * 16000, "c_mid": 22 * 16000 + 7}
    for stem, L in lengths.items():
        wavfile.write(str(wav_dir / f"{stem}.wav"), 16000, (0.1 * rng.standard_normal(L)).astype(np.float32))
    out = tmp_path / "out"
    argv = ["task=transcription", "dataset=Custom", f"dataset.args.audio_path={wav_dir}", "dataset.args.audio_ext=wav",
            "dataset.args.max_segment_samples=null", "task.timesteps=4", "model.args.residual_layers=3",
            "model.args.residual_channels=128", f"output_dir={out}", "seed=3", "task.recordings_per_chain=3"]
    torch.manual_seed(77)                                   # (the CLI's model without a checkpoint draws its weights)
    cli.main(argv)
    cfg = cli.build_config(argv)
    torch.manual_seed(77)
    m = cli.make_model(cfg, torch.device("cuda", torch.cuda.current_device()))
    for i, (stem, L) in enumerate(sorted(lengths.items())):
        roll = np.load(out / f"roll_{stem}.npy")
        assert roll.shape == (1, 1, math.ceil(L / HOP), 88) and np.isfinite(roll).all()
        solo = m.sample_long(ingest(str(wav_dir / f"{stem}.wav"), 16000, None), seed=3, recording=i).cpu().numpy()
        d = maxdiff(roll, solo)
        print(f"{stem}: CLI chain vs sample_long max |delta| = {d:.3e}")
        assert d <= ATOL, (stem, d)
        assert (out / f"raw_midi_{stem}.mid").exists() and (out / f"clean_midi_{stem}.mid").exists()
