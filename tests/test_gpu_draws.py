"""Several draws per clip in one chain on the MI355X (options "draws" / "draw_stride" of include/diffroll_amd.h,
ClassifierFreeDiffRoll.sample(draws=), sample_long_batch(draws=)).  The feature is defined by equivalences with code that
exists without it, so every comparison here is bitwise (torch.equal):

  * D draws of n clips after frontend(n clips)  ==  the same D * n rolls after frontend(the waveform tiled D times);
  * "draw_stride" = G  ==  D plain chains of the n clips with first_sample + d * G;
  * draw d of a long-form batch  ==  today's sample_long_batch with first_recording + d * (number of recordings).

Both sides of the first equivalence launch the same batch (same NB, T), so the planner picks the same kernels for both
and nothing has to be pinned; the other two compare batches of different sizes, which only are the same arithmetic with
the kernel flavours pinned and split-K off (as tests/test_gpu_longform.py does).  The engine exposes no byte count of its
allocations (no dr_debug_* for it), so the conditioner's size is not asserted here (tools/draws_sweep.py reports it).
"""
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import make_model
from tuning_pins import pinned

from diffroll_amd import longform
from diffroll_amd.engine import EngineError

pytestmark = pytest.mark.gpu

HOP = 512


def small(sampler, precision="f32", layers=3, k=9, steps=6, channels=64, seed=7):
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=channels, residual_layers=layers, kernel_size=k, timesteps=steps)
    p = R.synthetic_params(hp, seed=seed)
    return hp, make_model(hp, p, sampler=sampler, w=0.5, precision=precision)


def clips(n, T, seed):
    """n DIFFERENT seeded waveforms: a wrong b % n or b / n changes the result."""
    g = torch.Generator().manual_seed(seed)
    wav = torch.stack([(0.05 + 0.1 * i) * torch.randn(T * HOP, generator=g) for i in range(n)])
    assert not torch.equal(wav[0], wav[-1]) or n == 1
    return wav, g


# ---------------------------------------------------------------------------------------------- 1. the defining equivalence
@pytest.mark.parametrize("fused", [False, True], ids=["per_phase", "fused"])
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("sampler", ["ddpm_x0", "cfdg_ddpm_x0", "cfdg_ddim_x0"])
def test_draws_equal_the_tiled_batch_bitwise(sampler, precision, fused):
    """n = 2 clips, D = 3 draws, T = 125, k = 9: eager and captured graph, Philox and injected noise.  (The split-bf16
    fused kernel needs a channel count that is a multiple of 128: those cases run C = 128, everything else C = 64.)"""
    n, D, T = 2, 3, 125
    hp, m = small(sampler, precision, channels=128 if precision == "bf16x3" else 64)
    S = hp["timesteps"]
    eng = m.engine
    eng.set_option("fused_stack", 2 if fused else 0)
    wav, g = clips(n, T, 11)
    x = torch.randn(D * n, 1, T, 88, generator=g)
    nz = torch.randn(S, D * n, 1, T, 88, generator=g)
    # the tail kernel exists in exact fp32 only
    want_mode = ("fused_stack+tail" if precision == "f32" else "fused_stack") if fused else "per_phase"
    tiled_wav = wav.repeat(D, 1)
    try:
        for use_graph in (False, True):
            for noise in (None, nz):
                got, spec = m.sample(x, wav, noise=noise, seed=5, first_sample=3, use_graph=use_graph, draws=D)
                assert eng.launch_state()["mode"] == want_mode, eng.launch_state()
                assert eng.draws == 1 and eng.draw_stride == 0          # restored
                ref, ref_spec = m.sample(x, tiled_wav, noise=noise, seed=5, first_sample=3, use_graph=use_graph)
                assert eng.launch_state()["mode"] == want_mode, eng.launch_state()
                assert got.shape == (D * n, 1, T, 88) and spec.shape == (n, hp["n_mels"], T)
                assert torch.equal(spec, ref_spec[:n])
                assert torch.equal(got, ref), (use_graph, noise is not None, float((got - ref).abs().max()))
                # the draws differ from each other and the clips differ inside a draw: nothing degenerate was compared
                assert not torch.equal(got[0], got[n]) and not torch.equal(got[0], got[1])
        st = eng.launch_state()
        assert st["fallbacks"] == 0 and st["yields"] == 0, st
    finally:
        eng.set_option("fused_stack", 1)


# ---------------------------------------------------------------------------------------------- 2. a chunk boundary inside a draw
def test_a_fused_chunk_that_starts_inside_a_draw_wraps_round_the_clips():
    """27 conditional evaluations (n = 3 clips, D = 9) of 640 frames on 64-frame blocks (tune.stack_fl = 1): 10 blocks per
    evaluation, so a 256-CU chip takes 25 per launch and the planner cuts the batch into balanced chunks of 14 + 13 - the
    second one starts at row 14 = draw 4, clip 2, and wraps after one row."""
    n, D, T = 3, 9, 640
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = min(cus, 1024) // 10
    chunks = -(-n * D // cap)
    first = n * D // chunks + (1 if (n * D) % chunks else 0)
    assert chunks >= 2 and first % n != 0, (cus, chunks, first)
    hp, m = small("ddpm_x0", layers=2, k=3, steps=3)
    S = hp["timesteps"]
    eng = m.engine
    wav, g = clips(n, T, 23)
    x = torch.randn(D * n, 1, T, 88, generator=g)
    with pinned(eng, {"tune.stack_fl": (1, 0)}):
        eng.set_option("fused_stack", 2)
        eng.stack_status()
        n0 = eng.stack_launches
        got, _ = m.sample(x, wav, seed=2, use_graph=False, draws=D)
        eng.stack_status()
        assert eng.stack_launches - n0 == S * chunks, (eng.stack_launches - n0, S, chunks)
        assert eng.launch_state()["mode"] == "fused_stack"
        ref, _ = m.sample(x, wav.repeat(D, 1), seed=2, use_graph=False)
        assert torch.equal(got, ref), float((got - ref).abs().max())
        got_g, _ = m.sample(x, wav, seed=2, use_graph=True, draws=D)
        assert torch.equal(got_g, ref)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


# ---------------------------------------------------------------------------------------------- 3. 640 frames, 160-frame flavour
def test_640_frames_on_the_160_frame_stack():
    """The shipping window geometry at full width (C = 512, k = 9, 2 layers, 4 steps, guided): one clip, two draws, the
    fused residual stack on 160-frame blocks followed by the tail kernel."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_layers=2, kernel_size=9, timesteps=4)
    m = make_model(hp, R.synthetic_params(hp, seed=649), sampler="cfdg_ddpm_x0", w=0.5)
    eng = m.engine
    wav, g = clips(1, 640, 641)
    x = torch.randn(2, 1, 640, 88, generator=g)
    nz = torch.randn(4, 2, 1, 640, 88, generator=g)
    with pinned(eng, {"tune.stack_fl": (5, 0)}):
        eng.set_option("fused_stack", 2)
        eng.profile_enable(True)                    # (a profiled chain runs eager)
        got_e, _ = m.sample(x, wav, noise=nz, draws=2)
        _, _, _, kname = eng.profile_read_ex()
        eng.profile_enable(False)
        assert kname.startswith("stack_kernel<5>"), kname
        assert eng.launch_state()["mode"] == "fused_stack+tail", eng.launch_state()
        got, _ = m.sample(x, wav, noise=nz, draws=2)
        assert eng.launch_state()["mode"] == "fused_stack+tail", eng.launch_state()
        ref, _ = m.sample(x, wav.repeat(2, 1), noise=nz)
        assert torch.equal(got, ref) and torch.equal(got_e, ref), float((got - ref).abs().max())
        got_p, _ = m.sample(x, wav, seed=9, draws=2)
        ref_p, _ = m.sample(x, wav.repeat(2, 1), seed=9)
        assert torch.equal(got_p, ref_p)
    assert not torch.equal(got[0], got[1])


def test_two_clips_of_640_frames_wrap_on_the_160_frame_stack_and_the_tail():
    """The case above has one clip, so every row reads tensor 0 whatever the index arithmetic does.  Here n = 2 different
    clips, D = 3, at a cheap width (C = 64, 2 layers, k = 9, guided): stack_kernel<5> and the tail kernel, whose
    next-step first-layer conv runs on 96-frame items at this geometry (one round of 7 items instead of two of 10), read
    clip b % 2."""
    n, D, T = 2, 3, 640
    hp, m = small("cfdg_ddpm_x0", layers=2, steps=4)
    eng = m.engine
    wav, g = clips(n, T, 643)
    x = torch.randn(D * n, 1, T, 88, generator=g)
    nz = torch.randn(4, D * n, 1, T, 88, generator=g)
    with pinned(eng, {"tune.stack_fl": (5, 0)}):
        eng.set_option("fused_stack", 2)
        eng.profile_enable(True)
        got_e, _ = m.sample(x, wav, noise=nz, draws=D)
        _, _, _, kname = eng.profile_read_ex()
        eng.profile_enable(False)
        assert kname.startswith("stack_kernel<5>"), kname
        assert eng.launch_state()["mode"] == "fused_stack+tail", eng.launch_state()
        t0 = eng.tail_launches
        got, _ = m.sample(x, wav, noise=nz, draws=D)
        assert eng.tail_launches > t0 and eng.launch_state()["mode"] == "fused_stack+tail"
        ref, _ = m.sample(x, wav.repeat(D, 1), noise=nz)
        assert torch.equal(got, ref) and torch.equal(got_e, ref), float((got - ref).abs().max())
        got_p, _ = m.sample(x, wav, seed=3, draws=D)
        ref_p, _ = m.sample(x, wav.repeat(D, 1), seed=3)
        assert torch.equal(got_p, ref_p)
        # the captured chain is keyed by the option, not dropped by it: the same draws call again replays, bit for bit
        again, _ = m.sample(x, wav, seed=3, draws=D)
        assert torch.equal(again, got_p)
    # same x_T and noise rows for the two clips of a draw would still differ through the conditioning
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2])


# ---------------------------------------------------------------------------------------------- 4. draw_stride
# batches of different sizes are the same arithmetic only on the same kernels: 64-frame 32x32 conv tiles, the direct 1x1,
# no split-K, one launch per phase
SAME_KERNELS = {"tune.ksplit_max": (1, 16), "tune.tile": (3201, 0), "tune.pw_nw": (2, 0)}


def test_draw_stride_keys_draw_d_like_a_chain_of_first_sample_plus_d_G():
    n, D, T, G, first = 2, 2, 125, 7, 3
    hp, m = small("cfdg_ddpm_x0")
    eng = m.engine
    wav, g = clips(n, T, 31)
    x = torch.randn(D * n, 1, T, 88, generator=g)
    with pinned(eng, SAME_KERNELS):
        eng.set_option("fused_stack", 0)
        for use_graph in (False, True):
            got, _ = m.sample(x, wav, seed=4, first_sample=first, use_graph=use_graph, draws=D, draw_stride=G)
            for d in range(D):
                ref, _ = m.sample(x[d * n:(d + 1) * n], wav, seed=4, first_sample=first + d * G, use_graph=use_graph)
                assert torch.equal(got[d * n:(d + 1) * n], ref), (use_graph, d, float((got[d * n:(d + 1) * n] - ref).abs().max()))
        # ... and G = 0 keys row b as first_sample + b: with other keys the rolls differ
        plain, _ = m.sample(x, wav, seed=4, first_sample=first, draws=D)
        assert torch.equal(plain[:n], got[:n]) and not torch.equal(plain[n:], got[n:])


# ---------------------------------------------------------------------------------------------- 5. long-form
LONG_PINS = {"tune.ksplit_max": (1, 16), "tune.tile": (3205, 0), "tune.pw_nw": (5, 0), "tune.stack_fl": (5, 0)}


def windows_of_draws(m, batch, wavs, x_T, D, seed, first, use_graph):
    """sample_long_batch(draws=D)'s chain, keeping the windows: (D, n, T, 88)."""
    return m._sample_windows(batch, wavs, x_T, None, D, seed, first, use_graph, True).reshape(D, batch.n, 640, 88)


@pytest.mark.parametrize("fused", [False, True], ids=["per_phase", "fused"])
def test_long_form_draw_d_is_the_chain_of_first_recording_plus_d_R(fused):
    """Recordings of 2 windows and 1 window, two draws in one chain of 6 windows: draw d is, bit for bit, what
    sample_long_batch returns without the option for first_recording + 2 d on draw d's canvases; inside each draw the
    frames two windows of a recording share are identical, and nothing is shared across a recording or draw boundary."""
    D, first, seed = 2, 5, 8
    hp, m = small("cfdg_ddpm_x0", layers=2, steps=4)
    eng = m.engine
    g = torch.Generator().manual_seed(77)
    lengths = [640 * HOP + 150 * HOP - 33, 400 * HOP + 9]
    batch = longform.plan_batch(lengths, HOP, overlap=160)
    assert [q.n for q in batch.plans] == [2, 1] and batch.marks == [2]
    wavs = [0.1 * torch.randn(L, generator=g) for L in lengths]
    x_T = [torch.randn(D, 1, q.T_c, 88, generator=g) for q in batch.plans]
    with pinned(eng, LONG_PINS):
        eng.set_option("fused_stack", 2 if fused else 0)
        rolls = m.sample_long_batch(wavs, overlap=160, seed=seed, first_recording=first, x_T=x_T, draws=D)
        assert eng.launch_state()["mode"] == ("fused_stack+tail" if fused else "per_phase"), eng.launch_state()
        assert eng.draws == 1 and eng.window_overlap == 0 and eng.window_breaks == ()
        assert [tuple(r.shape) for r in rolls] == [(D, 1, q.T_out, 88) for q in batch.plans]
        for d in range(D):
            ref = m.sample_long_batch(wavs, overlap=160, seed=seed, first_recording=first + 2 * d, x_T=[x[d:d + 1] for x in x_T])
            for r in range(2):
                assert torch.equal(rolls[r][d:d + 1], ref[r]), (d, r, float((rolls[r][d:d + 1] - ref[r]).abs().max()))
        assert not torch.equal(rolls[0][0], rolls[0][1])
        for use_graph in (False, True):
            win = windows_of_draws(m, batch, wavs, x_T, D, seed, first, use_graph).cpu()
            q = batch.plans[0]
            for d in range(D):
                assert torch.equal(win[d, 0, q.stride:], win[d, 1, :q.overlap]), (use_graph, d)      # shared frames of recording 0
                assert not torch.equal(win[d, 1, q.stride:], win[d, 2, :q.overlap])                  # recording boundary
                for r, (f, p) in enumerate(zip(batch.first, batch.plans)):
                    assert torch.equal(longform.stitch(win[d, f:f + p.n], p), rolls[r][d, 0].cpu()), (use_graph, d, r)
            assert not torch.equal(win[0, 2, q.stride:], win[1, 0, :q.overlap])                      # draw boundary


# ---------------------------------------------------------------------------------------------- 6. argument errors, hygiene
def test_argument_errors_and_draws_1_after_draws_3():
    n, T = 2, 125
    hp, m = small("ddpm_x0")
    eng = m.engine
    wav, g = clips(n, T, 41)
    x = torch.randn(3 * n, T, 88, generator=g).to(eng.device)
    plain, _ = m.sample(x[:n].unsqueeze(1), wav, seed=1)
    eng.frontend(wav, T)
    m._fe_key = None
    with pytest.raises(ValueError, match="draws is >= 1"):
        eng.set_option("draws", 0)
    with pytest.raises(ValueError, match="draw_stride is >= 0"):
        eng.set_option("draw_stride", -1)
    assert eng.draws == 1 and eng.draw_stride == 0
    eng.set_option("draws", 3)
    try:
        # B % D != 0: DR_EINVAL with both numbers (Engine.sample refuses it before the call; dr_step is the bare ABI)
        with pytest.raises(ValueError, match=r"B=4 .*draws = 3"):
            eng.step("ddpm_x0", x[:4].clone(), None, 2)
        with pytest.raises(ValueError, match="not a whole number of draws"):
            eng.sample("ddpm_x0", x[:4].clone(), None)
        # the front-end ran on 2 clips: 9 rolls are 3 draws of 3 clips -> DR_ESTATE with both numbers
        x9 = torch.randn(9, T, 88, generator=g).to(eng.device)
        with pytest.raises(EngineError, match=r"dr_frontend\(B=2,T=125\).*3 draws of B/draws=3 clips"):
            eng.sample("ddpm_x0", x9, None)
        # a window_break mark names a window of ONE draw
        eng.set_option("window_overlap", 40)
        eng.set_option("window_break", 2)
        with pytest.raises(ValueError, match="window_break 2 is not a window of one draw"):
            eng.sample("ddpm_x0", x.clone(), None)
        eng.set_option("window_break", 0)
        eng.set_option("window_overlap", 0)
        three = eng.sample("ddpm_x0", x.clone(), None, seed=1)              # a chain captured with draws = 3
        assert not torch.equal(three[:n], three[n:2 * n])
    finally:
        eng.set_option("window_break", 0)
        eng.set_option("window_overlap", 0)
        eng.set_option("draws", 1)
    # draws = 1 again on the same engine: the plain result, no stale chain, and 6 rolls now need 6 clips
    again = eng.sample("ddpm_x0", x[:n].clone(), None, seed=1)
    assert torch.equal(again, plain[:, 0])
    with pytest.raises(EngineError, match=r"dr_frontend\(B=2,T=125\)"):
        eng.sample("ddpm_x0", x.clone(), None)
