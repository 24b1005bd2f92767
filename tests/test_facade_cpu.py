"""What the façade (diffroll_amd/model.py) asks of the engine, without a GPU: a recording stand-in for Engine is installed
on a small ClassifierFreeDiffRoll (m._engine, device = cpu) and every entry point's conversation with it is asserted -
the calls in order, their scalars, the shapes of the tensors and the contents of those the façade builds itself - together
with the shape and value of what the façade returns.

Two things are not part of the conversation and are taken out before the comparison (talk()): a set that leaves an option
as it was, and the order inside a run of consecutive option sets.  Where "nothing is set" is the point, the raw record is
asserted.  The engine's sample() records the options in force when it is called.
"""
import inspect

import pytest
import torch

from diffroll_amd import longform
from diffroll_amd.engine import Engine
from diffroll_amd.ensemble import aggregate
from facade_fakes import DEFAULTS, HOP, L1, L2, MELS, SAMPLERS, W, RecordingEngine, clip, eq, facade, sample_call, weight


# ---------------------------------------------------------------------------------------------- single steps
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_single_step_methods(sampler):
    masks = dict(inpainting_t=[10, 20], inpainting_f=[3, 40])
    m, eng = facade(sampler, **masks)                        # (the masks reach the front-end for inpainting_ddpm_x0 only)
    wav, x, z, _ = clip(2, 125)
    roll, spec = getattr(m, sampler)(x, wav, 3, z)
    it, i_f = (masks["inpainting_t"], masks["inpainting_f"]) if sampler == "inpainting_ddpm_x0" else (None, None)
    want = [] if sampler == "generation_ddpm_x0" else [("frontend", eq(wav), 125, it, i_f)]
    want += [("step", sampler, eq(x[:, 0]), eq(z[:, 0]), 3, weight(sampler), 0, 0), ("finish",)]
    assert eng.talk() == want
    assert torch.equal(roll, x)
    fill = -1.0 if sampler == "generation_ddpm_x0" else 0.0
    assert torch.equal(spec, torch.full((2, MELS, 125), fill))
    assert m.reverse_diffusion == getattr(m, sampler)


def test_single_step_without_noise_draws_from_the_global_generator():
    m, eng = facade("ddpm_x0")
    wav, x, _, _ = clip(2, 125)
    torch.manual_seed(3)
    z = torch.randn(2, 125, 88)
    torch.manual_seed(3)
    m.ddpm_x0(x, wav, 3)
    assert eng.talk() == [("frontend", eq(wav), 125, None, None), ("step", "ddpm_x0", eq(x[:, 0]), eq(z), 3, 0.0, 0, 0), ("finish",)]
    m.ddpm_x0(x, wav, 0)                                     # t = 0: no noise at all (and the front-end is cached)
    assert eng.talk() == [("step", "ddpm_x0", eq(x[:, 0]), None, 0, 0.0, 0, 0), ("finish",)]


def test_generation_step_conditioning():
    # no waveform: the roll keeps its length
    m, eng = facade("generation_ddpm_x0")
    _, x, z, _ = clip(2, 125)
    roll, spec = m.generation_ddpm_x0(x, None, 3, z)
    assert eng.talk() == [("step", "generation_ddpm_x0", eq(x[:, 0]), eq(z[:, 0]), 3, 0.0, 0, 0), ("finish",)]
    assert torch.equal(roll, x) and torch.equal(spec, torch.full((2, MELS, 125), -1.0))
    # a waveform shorter than the roll trims it (trim_spec_roll), and no front-end runs
    wav, _, _, _ = clip(2, 125, frames=99)                   # 99 * hop samples: 100 spectrogram frames
    z100 = z[:, :, :100].contiguous()
    roll, spec = m.generation_ddpm_x0(x, wav, 3, z100)
    assert eng.talk() == [("step", "generation_ddpm_x0", eq(x[:, 0, :100].contiguous()), eq(z100[:, 0]), 3, 0.0, 0, 0), ("finish",)]
    assert torch.equal(roll, x[:, :, :100]) and torch.equal(spec, torch.full((2, MELS, 100), -1.0))
    # condition='trainable_spec': the roll is trimmed to the 641 learned frames, which are the spectrogram returned
    m, eng = facade("generation_ddpm_x0", condition="trainable_spec")
    m.trainable_parameters.copy_(torch.randn(MELS, 641, generator=torch.Generator().manual_seed(1)))
    _, x, _, _ = clip(2, 700)
    z641 = torch.randn(2, 1, 641, 88, generator=torch.Generator().manual_seed(2))
    roll, spec = m.generation_ddpm_x0(x, None, 3, z641)
    assert eng.talk() == [("step", "generation_ddpm_x0", eq(x[:, 0, :641].contiguous()), eq(z641[:, 0]), 3, 0.0, 0, 0), ("finish",)]
    assert torch.equal(roll, x[:, :, :641]) and torch.equal(spec, m.trainable_parameters.detach())
    assert m.output_frames(700, None) == 641 == m.sample(x)[0].shape[2]


# ---------------------------------------------------------------------------------------------- forward
def test_forward():
    m, eng = facade()
    wav, x, _, _ = clip(2, 125)
    x0, spec = m.forward(x, wav, torch.tensor([3, 3]))
    assert eng.talk() == [("frontend", eq(wav), 125, None, None), ("forward", eq(x[:, 0]), 3, False), ("finish",)]
    assert torch.equal(x0, x) and torch.equal(spec, torch.zeros(2, MELS, 125))
    x0, spec = m.forward(x, wav, torch.tensor([3, 1]))       # one step per sample (and the front-end is cached)
    assert eng.talk() == [("forward_steps", eq(x[:, 0]), [3, 1], False), ("finish",)]
    assert torch.equal(x0, x) and torch.equal(spec, torch.zeros(2, MELS, 125))
    x0, spec = m.forward(x, wav, torch.tensor([2, 2]), sampling=True)          # the unconditional evaluation
    assert eng.talk() == [("forward", eq(x[:, 0]), 2, True), ("finish",)]
    assert torch.equal(x0, x) and torch.equal(spec, torch.full((2, MELS, 125), -1.0))
    with pytest.raises(ValueError, match="diffusion_step has 3 entries for a batch of 2"):
        m.forward(x, wav, torch.tensor([3, 3, 3]))


# ---------------------------------------------------------------------------------------------- sample
def test_sample_draws_and_the_frontend_cache():
    m, eng = facade()
    wav, x, _, _ = clip(2, 125)
    roll, spec = m.sample(x, wav, seed=7, first_sample=3, use_graph=False, check=False)
    assert not any(c[0].startswith("set_") for c in eng.calls)              # draws = 1 holds already: nothing is set
    assert eng.talk() == [("frontend", eq(wav), 125, None, None), sample_call("cfdg_ddpm_x0", x[:, 0], None, 7, 3, False, False)]
    assert torch.equal(roll, x) and torch.equal(spec, torch.zeros(2, MELS, 125))
    assert m.output_frames(125, wav.shape[1]) == 125
    m.sample(x, wav)                                         # the same waveform again: no front-end
    assert eng.talk() == [sample_call("cfdg_ddpm_x0", x[:, 0], None)]
    # two draws of the two clips, keyed 5 apart: set before the chain, restored after it, one spectrogram per clip
    x4 = torch.randn(4, 1, 125, 88, generator=torch.Generator().manual_seed(4))
    roll, spec = m.sample(x4, wav, seed=1, draws=2, draw_stride=5)
    assert eng.talk() == [("set_option", "draw_stride", 5), ("set_option", "draws", 2),
                          sample_call("cfdg_ddpm_x0", x4[:, 0], None, 1, draws=2, draw_stride=5),
                          ("set_option", "draw_stride", 0), ("set_option", "draws", 1)]
    assert torch.equal(roll, x4) and spec.shape == (2, MELS, 125)
    # ... and nothing is set where the options hold already
    eng.set_option("draws", 2)
    eng.set_option("draw_stride", 5)
    eng.calls = []
    m.sample(x4, wav, draws=2, draw_stride=5)
    assert not any(c[0].startswith("set_") for c in eng.calls)
    assert eng.talk() == [sample_call("cfdg_ddpm_x0", x4[:, 0], None, draws=2, draw_stride=5)]
    assert (eng.draws, eng.draw_stride) == (2, 5)
    # restored also when the chain raises
    eng.fail = True
    with pytest.raises(RuntimeError, match="sample failed"):
        m.sample(x, wav)
    assert (eng.draws, eng.draw_stride) == (2, 5) and eng.talk()[-2:] == [("set_option", "draw_stride", 5), ("set_option", "draws", 2)]


def test_sample_trims_the_roll_and_the_noise_to_the_spectrogram():
    m, eng = facade()
    wav, x, _, nz = clip(2, 125, frames=99)                  # 100 spectrogram frames
    roll, spec = m.sample(x, wav, noise=nz)
    z = nz[:, :, 0, :100].contiguous()
    assert eng.talk() == [("frontend", eq(wav), 125, None, None), sample_call("cfdg_ddpm_x0", x[:, 0, :100].contiguous(), z)]
    assert torch.equal(roll, x[:, :, :100]) and spec.shape == (2, MELS, 100)
    assert m.output_frames(125, wav.shape[1]) == 100
    # generation: no front-end, no weight; the spectrogram returned is -1 per clip
    m, eng = facade("generation_ddpm_x0")
    x4 = torch.randn(4, 1, 125, 88, generator=torch.Generator().manual_seed(4))
    roll, spec = m.sample(x4, draws=2)
    assert eng.talk() == [("set_option", "draws", 2), sample_call("generation_ddpm_x0", x4[:, 0], None, draws=2), ("set_option", "draws", 1)]
    assert torch.equal(roll, x4) and torch.equal(spec, torch.full((2, MELS, 125), -1.0))
    assert m.output_frames(125, None) == 125
    roll, spec = m.sample(x, wav, noise=nz)
    assert eng.talk() == [sample_call("generation_ddpm_x0", x[:, 0, :100].contiguous(), z)]
    assert spec.shape == (2, MELS, 100) and m.output_frames(125, wav.shape[1]) == 100
    # the inpainting masks reach the front-end of the whole chain too
    m, eng = facade("inpainting_ddpm_x0", inpainting_t=[10, 20], inpainting_f=[3, 40])
    wav, x, _, _ = clip(2, 125)
    m.sample(x, wav)
    assert eng.talk() == [("frontend", eq(wav), 125, [10, 20], [3, 40]), sample_call("inpainting_ddpm_x0", x[:, 0], None)]


def test_sample_errors():
    m, eng = facade()
    wav, x, _, _ = clip(3, 125)
    with pytest.raises(ValueError, match="x_T holds 3 rolls: not a whole number of draws = 2"):
        m.sample(x, wav, draws=2)
    with pytest.raises(ValueError, match="2 draws of 4 rolls take the waveform of 2 clips, got 3"):
        m.sample(torch.zeros(4, 1, 125, 88), wav, draws=2)
    with pytest.raises(ValueError, match="waveform is required for conditional samplers"):
        m.sample(x)
    with pytest.raises(ValueError, match="draws must be"):
        m.sample(x, wav, draws=0)
    assert eng.talk() == []


# ---------------------------------------------------------------------------------------------- long form
def recordings(D=1, S=4, seed=21):
    g = torch.Generator().manual_seed(seed)
    batch = longform.plan_batch([L2, L1], HOP, overlap=160)
    assert [p.n for p in batch.plans] == [2, 1] and batch.marks == [2]
    wavs = [torch.randn(L, generator=g) for L in (L2, L1)]
    x_T = [torch.randn(D, 1, p.T_c, 88, generator=g) for p in batch.plans]
    noise = [torch.randn(S, D, 1, p.T_c, 88, generator=g) for p in batch.plans]
    return batch, wavs, x_T, noise


def set_by_hand(m, eng, overlap=32, marks=()):
    """Options a caller left set and a stale front-end key: a long-form call samples under its own and puts these back."""
    eng.set_option("window_overlap", overlap)
    for b in marks:
        eng.set_option("window_break", b)
    eng.calls = []
    m._fe_key = "stale"


def test_sample_long_conditional():
    m, eng = facade(timesteps=4)
    batch, wavs, x_T, noise = recordings()
    plan, wav, x, nz = batch.plans[0], wavs[0], x_T[0], noise[0]
    set_by_hand(m, eng)
    roll = m.sample_long(wav, overlap=160, seed=5, recording=2, x_T=x, noise=nz, use_graph=False)
    xb = longform.gather_windows(x.reshape(plan.T_c, 88), plan)
    zb = longform.gather_windows(nz.reshape(4, plan.T_c, 88), plan)
    assert xb.shape == (2, 640, 88) and zb.shape == (4, 2, 640, 88)
    assert eng.talk() == [("frontend", eq(longform.window_audio(wav, plan, HOP)), 640, None, None),
                          ("set_option", "window_overlap", 160),
                          sample_call("cfdg_ddpm_x0", xb, zb, 5, 2, False, True, window_overlap=160),
                          ("set_option", "window_overlap", 32)]
    assert m._fe_key is None
    assert roll.shape == (1, 1, 700, 88) and torch.equal(roll[0, 0], longform.stitch(xb, plan))
    assert eng.options() == dict(DEFAULTS, window_overlap=32)
    # restored also when the chain raises
    eng.fail = True
    with pytest.raises(RuntimeError, match="sample failed"):
        m.sample_long(wav, x_T=x)
    assert eng.options() == dict(DEFAULTS, window_overlap=32)
    eng.fail = False
    eng.talk()
    # two draws: the batch method's chain of one recording
    batch2, _, x2, nz2 = recordings(D=2)
    rolls = m.sample_long(wav, seed=5, recording=2, x_T=x2[0], noise=nz2[0], draws=2)
    xb = torch.cat([longform.gather_windows(x2[0][d].reshape(plan.T_c, 88), plan) for d in range(2)], 0)
    zb = torch.cat([longform.gather_windows(nz2[0][:, d].reshape(4, plan.T_c, 88), plan) for d in range(2)], 1)
    got = eng.talk()
    assert got[0] == ("frontend", eq(longform.window_audio(wav, plan, HOP)), 640, None, None)
    assert got[-3] == sample_call("cfdg_ddpm_x0", xb, zb, 5, 2, window_overlap=160, draws=2)
    assert rolls.shape == (2, 1, 700, 88) and torch.equal(rolls[:, 0], longform.stitch(xb.reshape(2, 2, 640, 88), plan))
    assert eng.options() == dict(DEFAULTS, window_overlap=32)


def test_sample_long_generation():
    m, eng = facade("generation_ddpm_x0", timesteps=4)
    plan = longform.plan_windows(700, None, overlap=160)
    set_by_hand(m, eng)
    roll = m.sample_long(frames=700, seed=5, recording=1)    # x_T: the canvas of torch.Generator().manual_seed(seed)
    xb = longform.gather_windows(torch.randn(1, 1, plan.T_c, 88, generator=torch.Generator().manual_seed(5)).reshape(plan.T_c, 88), plan)
    assert eng.talk() == [("set_option", "window_overlap", 160),
                          sample_call("generation_ddpm_x0", xb, None, 5, 1, window_overlap=160),
                          ("set_option", "window_overlap", 32)]
    assert roll.shape == (1, 1, 700, 88) and torch.equal(roll[0, 0], longform.stitch(xb, plan))
    assert m._fe_key == "stale"                              # (no front-end ran: nothing to forget)


@pytest.mark.parametrize("D", [1, 2])
def test_sample_long_batch(D):
    m, eng = facade(timesteps=4)
    batch, wavs, x_T, noise = recordings(D)
    set_by_hand(m, eng, marks=(5,))
    rolls = m.sample_long_batch(wavs, overlap=160, seed=5, first_recording=3, x_T=x_T, noise=noise, draws=D)
    # the window batch of draw 0, then that of draw 1 (draw-major), over ONE front-end of the windows' audio
    xb = torch.cat([longform.gather_batch([x[d].reshape(p.T_c, 88) for x, p in zip(x_T, batch.plans)], batch) for d in range(D)], 0)
    zb = torch.cat([longform.gather_batch([z[:, d].reshape(4, p.T_c, 88) for z, p in zip(noise, batch.plans)], batch) for d in range(D)], 1)
    assert xb.shape == (3 * D, 640, 88) and zb.shape == (4, 3 * D, 640, 88)
    audio = torch.cat([longform.window_audio(wv, p, HOP) for wv, p in zip(wavs, batch.plans)])
    held = dict(window_overlap=160, window_breaks=(2,), draws=D)
    got = eng.talk()
    assert got[0] == ("frontend", eq(audio), 640, None, None)
    at = [c[0] for c in got].index("sample")
    assert got[at] == sample_call("cfdg_ddpm_x0", xb, zb, 5, 3, **held)
    assert all(c[0].startswith("set_") for c in got[1:at] + got[at + 1:])
    assert eng.options() == dict(DEFAULTS, window_overlap=32, window_breaks=(5,))      # as the caller left them
    assert m._fe_key is None
    want = longform.stitch_batch(xb.reshape(D, 3, 640, 88), batch)
    assert [tuple(r.shape) for r in rolls] == [(D, 1, 700, 88), (D, 1, 301, 88)]
    assert all(torch.equal(r[:, 0], w) for r, w in zip(rolls, want))
    # the default canvases: the first D of the seed's generator, per recording; Philox noise
    rolls = m.sample_long_batch(wavs, seed=9, draws=D)
    x9 = [torch.randn(D, 1, p.T_c, 88, generator=torch.Generator().manual_seed(9)) for p in batch.plans]
    xb = torch.cat([longform.gather_batch([x[d].reshape(p.T_c, 88) for x, p in zip(x9, batch.plans)], batch) for d in range(D)], 0)
    got = eng.talk()
    assert got[[c[0] for c in got].index("sample")] == sample_call("cfdg_ddpm_x0", xb, None, 9, 0, **held)
    # restored also when the chain raises
    eng.fail = True
    with pytest.raises(RuntimeError, match="sample failed"):
        m.sample_long_batch(wavs, draws=D)
    assert eng.options() == dict(DEFAULTS, window_overlap=32, window_breaks=(5,))


def test_sample_long_batch_generation():
    m, eng = facade("generation_ddpm_x0", timesteps=4)
    batch = longform.plan_batch([700, 301], None, overlap=160)
    rolls = m.sample_long_batch(frames=[700, 301], seed=2, first_recording=1)
    x2 = [torch.randn(1, 1, p.T_c, 88, generator=torch.Generator().manual_seed(2)) for p in batch.plans]
    xb = longform.gather_batch([x.reshape(p.T_c, 88) for x, p in zip(x2, batch.plans)], batch)
    assert eng.talk() == [("set_option", "window_overlap", 160), ("set_window_breaks", (2,)),
                          sample_call("generation_ddpm_x0", xb, None, 2, 1, window_overlap=160, window_breaks=(2,)),
                          ("set_option", "window_overlap", 0), ("set_window_breaks", ())]
    assert [tuple(r.shape) for r in rolls] == [(1, 1, 700, 88), (1, 1, 301, 88)]


def test_long_form_errors():
    m, eng = facade(timesteps=4)
    g, _ = facade("generation_ddpm_x0", timesteps=4)
    i, _ = facade("inpainting_ddpm_x0", timesteps=4, inpainting_t=[10, 20])
    wav = torch.zeros(L2)
    with pytest.raises(ValueError, match="sample_long does not support inpainting_ddpm_x0"):
        i.sample_long(wav)
    with pytest.raises(ValueError, match="sample_long_batch does not support inpainting_ddpm_x0"):
        i.sample_long_batch([wav])
    with pytest.raises(ValueError, match=r"generation_ddpm_x0: pass frames= \(the roll length\), not a waveform"):
        g.sample_long(wav)
    with pytest.raises(ValueError, match=r"generation_ddpm_x0: pass frames= \(the roll lengths\), not waveforms"):
        g.sample_long_batch([wav])
    with pytest.raises(ValueError, match=r"cfdg_ddpm_x0: pass waveform= \(L,\), not frames"):
        m.sample_long(frames=700)
    with pytest.raises(ValueError, match=r"cfdg_ddpm_x0: pass waveforms= \(a sequence of \(L,\) recordings\), not frames"):
        m.sample_long_batch(frames=[700])
    with pytest.raises(ValueError, match=r"waveform must be one recording \(L,\), got \(2, 1000\)"):
        m.sample_long(torch.zeros(2, 1000))
    with pytest.raises(ValueError, match=r"every waveform must be one recording \(L,\), got \(2, 1000\)"):
        m.sample_long_batch([wav, torch.zeros(2, 1000)])
    with pytest.raises(ValueError, match=r"x_T must be the canvas \(1, 1, 1120, 88\), got \(1, 1, 640, 88\)"):
        m.sample_long(wav, x_T=torch.zeros(1, 1, 640, 88))
    with pytest.raises(ValueError, match=r"x_T must be one canvas \(1, 1, T_c, 88\) per recording, T_c = \[1120\]"):
        m.sample_long_batch([wav], x_T=[torch.zeros(1, 1, 640, 88)])
    with pytest.raises(ValueError, match=r"x_T must be one canvas \(2, 1, T_c, 88\) per recording, T_c = \[1120\]"):
        m.sample_long(wav, x_T=torch.zeros(1, 1, 1120, 88), draws=2)
    with pytest.raises(ValueError, match=r"noise must be the canvas \(4, 1, 1, 1120, 88\), got \(4, 1, 1, 640, 88\)"):
        m.sample_long(wav, noise=torch.zeros(4, 1, 1, 640, 88))
    with pytest.raises(ValueError, match=r"noise must be one canvas \(4, 1, 1, T_c, 88\) per recording, T_c = \[1120\]"):
        m.sample_long_batch([wav], noise=[torch.zeros(4, 1, 1, 640, 88)])
    too_long = 640 + 480 * longform.MAX_WINDOWS               # one window more than a chain holds
    with pytest.raises(ValueError, match=r"257 windows of 640 frames: one chain holds at most 256 \(longform.MAX_WINDOWS\); split"):
        g.sample_long(frames=too_long)
    with pytest.raises(ValueError, match=r"258 windows in 2 recordings \(2 draw\(s\)\): one chain holds at most 256 \(longform.MAX_WINDOWS\)"):
        g.sample_long_batch(frames=[640 + 480 * 127, 640], draws=2)
    with pytest.raises(ValueError, match="overlap 321 out of range"):
        m.sample_long(wav, overlap=321)
    assert eng.talk() == []                                  # refused before anything reached the engine


# ---------------------------------------------------------------------------------------------- trajectory
def test_sample_trajectory():
    m, eng = facade()
    wav, x, _, nz = clip(2, 125)
    traj, spec = m.sample_trajectory(x, wav, noise=nz)       # injected noise; row 0 is not used: step 0 gets zeros
    want = [("frontend", eq(wav), 125, None, None)]
    for t in (5, 4, 3, 2, 1, 0):
        z = nz[t][:, 0] if t > 0 else torch.zeros(2, 125, 88)
        want += [("step", "cfdg_ddpm_x0", eq(x[:, 0]), eq(z), t, W, 0, 0), ("finish",)]
    assert eng.talk() == want
    assert traj.shape == (6, 2, 1, 125, 88) and all(torch.equal(r, x) for r in traj) and spec.shape == (2, MELS, 125)
    traj, _ = m.sample_trajectory(x, wav, seed=7, first_sample=3)          # Philox: the engine draws, keyed as sample() does
    want = []
    for t in (5, 4, 3, 2, 1):
        want += [("step", "cfdg_ddpm_x0", eq(x[:, 0]), None, t, W, 7, 3), ("finish",)]
    want += [("step", "cfdg_ddpm_x0", eq(x[:, 0]), eq(torch.zeros(2, 125, 88)), 0, W, 0, 0), ("finish",)]
    assert eng.talk() == want
    assert traj.shape == (6, 2, 1, 125, 88)
    # generation: -1 spectrogram, no front-end
    g, geng = facade("generation_ddpm_x0")
    traj, spec = g.sample_trajectory(x, seed=7)
    assert [c[0] for c in geng.talk()] == ["step", "finish"] * 6
    assert traj.shape == (6, 2, 1, 125, 88) and torch.equal(spec, torch.full((2, MELS, 125), -1.0))


def test_respaced_trajectory_and_stride_1_single_steps():
    m, eng = facade(sampling={"steps": 3})                   # 3 of 6 steps: t = 5, 3, 0
    assert eng.sampling_steps == 3 and m.visited_steps() == [5, 3, 0]
    wav, x, z, nz = clip(2, 125)
    traj, _ = m.sample_trajectory(x, wav, noise=nz)
    got = eng.talk()
    assert [c[4] for c in got if c[0] == "step"] == [5, 3, 0]
    assert not any(c[0].startswith("set_") for c in got) and eng.sampling_steps == 3
    assert traj.shape == (3, 2, 1, 125, 88)
    # the reference's single-step methods keep their stride-1 meaning: the option is off for their call
    m.cfdg_ddpm_x0(x, wav, 3, z)
    assert eng.talk() == [("set_option", "sampling_steps", 0),
                          ("step", "cfdg_ddpm_x0", eq(x[:, 0]), eq(z[:, 0]), 3, W, 0, 0), ("finish",)]
    m.sample(x, wav)                                         # ... and on again at the next chain
    assert eng.talk() == [("set_option", "sampling_steps", 3), sample_call("cfdg_ddpm_x0", x[:, 0], None)]


# ---------------------------------------------------------------------------------------------- predict_step / sampling
@pytest.mark.parametrize("D", [1, 2])
def test_predict_step_and_sampling(D):
    m, eng = facade(sampling={"draws": D})
    wav, x, _, nz = clip(2, 125)
    roll = m.predict_step((x, wav), batch_idx=4)
    sets = ([("set_option", "draws", 2)], [("set_option", "draws", 1)]) if D == 2 else ([], [])
    if D == 2:      # draw 0 starts from the batch's x_T, draw 1 from the generator seeded with batch_idx; the mean roll
        x_all = torch.cat([x, torch.randn(2, 1, 125, 88, generator=torch.Generator().manual_seed(4))], 0)
    else:
        x_all = x
    assert eng.talk() == [("frontend", eq(wav), 125, None, None)] + sets[0] + \
        [sample_call("cfdg_ddpm_x0", x_all[:, 0], None, 4, draws=D)] + sets[1]
    assert torch.equal(roll, aggregate(x_all, D)[0]) and roll.shape == (2, 1, 125, 88) and roll.is_contiguous()
    # sampling(): x_T from the batch, or drawn - from torch's global generator, or (draws) a generator seeded with batch_idx
    batch = {"frame": torch.zeros(2, 125, 88), "audio": wav, "x_T": x_all, "noise": None}
    roll, spec = m.sampling(batch, batch_idx=6)
    assert eng.talk() == sets[0] + [sample_call("cfdg_ddpm_x0", x_all[:, 0], None, 6, draws=D)] + sets[1]
    assert torch.equal(roll, aggregate(x_all, D)[0]) and spec.shape == (2, MELS, 125)
    torch.manual_seed(8)
    drawn = torch.randn(2, 1, 125, 88) if D == 1 else torch.randn(4, 1, 125, 88, generator=torch.Generator().manual_seed(6))
    torch.manual_seed(8)
    roll, _ = m.sampling({"frame": batch["frame"], "audio": wav}, batch_idx=6)
    assert eng.talk() == sets[0] + [sample_call("cfdg_ddpm_x0", drawn[:, 0], None, 6, draws=D)] + sets[1]
    assert torch.equal(roll, aggregate(drawn, D)[0])
    if D == 2:
        votes, std = m.last_ensemble
        assert votes.shape == std.shape == (2, 1, 125, 88)


# ---------------------------------------------------------------------------------------------- the stand-in itself
def test_the_stand_in_has_the_signatures_of_the_engine():
    for name in ("load_params", "set_precision", "set_option", "set_guidance_interval", "set_window_breaks", "frontend",
                 "forward", "forward_steps", "step", "sample", "finish"):
        mine, real = (inspect.signature(getattr(cls, name)).parameters.values() for cls in (RecordingEngine, Engine))
        assert [(p.name, p.default) for p in mine] == [(p.name, p.default) for p in real], name
