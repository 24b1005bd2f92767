"""What the test modules share: tolerances, the model builder, the comparison helpers and the input builders that more than
one file uses - test infrastructure, not collected.  tests/conftest.py puts tests/ on sys.path, so every test and case
module imports these by name from here and none imports from a test_*.py (tests/test_docs_cpu.py holds that).

Tolerances of the GPU parity tests (fp32 everywhere; the kernels use the exact-fp32 MFMA, so differences come only from
summation order, the FFT implementation and the hardware exp/rcp of the gate):
  * one network evaluation:      atol 1e-5  (outputs are O(1); observed <= 2.9e-6 over the whole suite)
  * one reverse step / chain:    atol 1e-5  (observed <= 2.9e-6; SURVEY.md 8c proposes 2e-5 per kernel)
  * normalised log-mel:          atol 4e-5  (values in [0,1]; observed <= 8.5e-6: own FFT vs torch's, amplified by
                                             the log at near-silent bins)
  * same clips, other shard / batch geometry (other tile flavour or split-K order): atol 1e-5 (observed <= 2.9e-6)
i.e. 3.4-5x the observed margins (DR_PARITY_LOG=<file> records every comparison): a 5x regression fails.
(Until the front-end tables were built with the reference's fp32 filterbank arithmetic the log-mel differed by
2e-5 and every conditional evaluation by up to 3e-5 - diffroll_amd/frontend_tables.py.)
"""
import json
import os
import re
import socket

import numpy as np
import pytest
import torch

from oracle import diffroll_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATOL_FWD = 1e-5
ATOL_STEP = 1e-5
ATOL_SPEC = 4e-5
ATOL_SHARD = 1e-5

# the sampling-option suites (respaced chains and everything written after them) and the long-form windows
ATOL = 1e-5
HOP = 512
S = 200


# ---------------------------------------------------------------------------------------------- the model and the comparison
def make_model(hp, params, sampler="cfdg_ddpm_x0", w=0.5, inpainting_t=None, inpainting_f=None, precision="f32", **extra):
    from diffroll_amd import ClassifierFreeDiffRoll
    m = ClassifierFreeDiffRoll(
        residual_channels=hp["residual_channels"], unconditional=False, condition="fixed",
        n_mels=hp["n_mels"], norm_args=[0, 1, "imagewise"], residual_layers=hp["residual_layers"],
        kernel_size=hp["kernel_size"], dilation_base=hp["dilation_base"],
        dilation_bound=hp["dilation_bound"],
        spec_args=dict(sample_rate=hp["sample_rate"], n_fft=hp["n_fft"], hop_length=hp["hop_length"],
                       n_mels=hp["n_mels"], f_min=hp["f_min"], f_max=hp["f_max"], center=True,
                       normalized=True, pad_mode="reflect"),
        spec_dropout=0.1, inpainting_t=inpainting_t, inpainting_f=inpainting_f,
        timesteps=hp["timesteps"], beta_start=hp["beta_start"], beta_end=hp["beta_end"],
        training={"mode": "x_0"}, sampling={"type": sampler, "w": w}, precision=precision, **extra)
    m.load_state_dict(params)
    return m


def maxdiff(a, b):
    d = float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
    log = os.environ.get("DR_PARITY_LOG")          # observed margins, one line per comparison (tools/gpu_*.sh)
    if log:
        import inspect
        # the line names the test: the nearest caller whose function starts with test_ (a comparison made inside agree() or
        # a shared scenario is the calling test's), else the direct caller
        stack = inspect.stack()[1:]
        fr = next((f for f in stack if f.function.startswith("test_")), stack[0])
        with open(log, "a") as f:
            f.write(f"{fr.function}:{fr.lineno} {d:.3e}\n")
    return d


def agree(roll, ref):
    """|d| <= ATOL where |ref| <= 1 (the x0 families' rolls), ATOL |ref| beyond - the epsilon samplers' rolls reach
    |x| ~ 17 under a random network (x_T / sqrt_acp and worse), where fp32 itself spacing is 2e-6 - and the same
    thresholded roll except within ATOL of the threshold.  Returns (ok, max |d|)."""
    roll = roll.cpu()
    d = maxdiff(roll, ref)
    within = ((roll - ref).abs() <= ATOL * ref.abs().clamp(min=1.0)).all()
    near = (ref - 0.5).abs() < ATOL
    return bool(within) and bool((((roll > 0.5) == (ref > 0.5)) | near).all()), d


def same_bits(got, want):
    """Bit equality of two fp32 tensors, a NaN equal to a NaN (its payload is the adder's, not the option's)."""
    got, want = got.cpu(), want.cpu()
    both_nan = torch.isnan(got) & torch.isnan(want)
    return bool(((got.view(torch.int32) == want.view(torch.int32)) | both_nan).all())


# ---------------------------------------------------------------------------------------------- inputs
def hp_of(channels=64, layers=4, k=9):
    """The 200-step network of the sampling-option suites."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=channels, residual_layers=layers, kernel_size=k, timesteps=S)
    return hp


def inputs(B, Tn, seed):
    g = torch.Generator().manual_seed(seed)
    wav = 0.1 * torch.randn(B, Tn * HOP, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    noise = torch.randn(S, B, 1, Tn, 88, generator=g)
    return wav, x, noise


def cfg2_inputs(B=16, steps=200):
    """BASELINE config 2's clips (4 s, 125 frames) from torch's global generator, seeded here."""
    torch.manual_seed(0)
    L = 64000
    Tn = L // 512
    wav = 0.1 * torch.randn(B, L)
    x = torch.randn(B, 1, Tn, 88)
    noise = torch.randn(steps, B, 1, Tn, 88)
    return wav, x, noise


def kernel_inputs(B, T, seed):
    """name -> the conditional prediction (B, T, 88): normal noise, all equal, two values with the tie straddling k and k + 1
    at v = 5000, a roll with +-0 and +-inf, a roll with one NaN, a roll of only NaN."""
    g = torch.Generator().manual_seed(seed)
    n = T * 88
    noise = 1.2 * torch.randn(B, T, 88, generator=g)
    two = torch.cat([torch.full((n // 2,), -1.5), torch.full((n - n // 2,), 2.5)])
    two = two[torch.randperm(n, generator=g)].reshape(1, T, 88).repeat(B, 1, 1)
    specials = noise.clone()
    specials[0].view(-1)[:4] = torch.tensor([0.0, -0.0, float("inf"), float("-inf")])[: min(4, n)]
    one_nan = noise.clone()
    one_nan[B - 1].view(-1)[n // 2] = float("nan")
    only_nan = noise.clone()
    only_nan[0] = float("nan")
    return {"noise": noise, "equal": torch.full((B, T, 88), 0.75), "two": two, "specials": specials, "one_nan": one_nan, "only_nan": only_nan}


def shard_model(sampler="cfdg_ddpm_x0", layers=4, steps=12, k=9, C=128):
    """The model of tests/test_gpu_sharding.py and of the rank processes it starts."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=C, residual_layers=layers, kernel_size=k, timesteps=steps)
    p = R.synthetic_params(hp, seed=11)
    return hp, p, make_model(hp, p, sampler=sampler, w=0.5)


# ---------------------------------------------------------------------------------------------- long form
def long_hp_of(layers=15, k=9, steps=4, channels=None):
    """The few-step, full-depth network of the long-form suites."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_layers=layers, kernel_size=k, timesteps=steps)
    if channels:
        hp["residual_channels"] = channels
    return hp


def oracle_long(p, hp, sampler, plan, wav, x_T, noise, w):
    """The joint chain on the CPU: windows of the canvas x_T / noise, one front-end per window crop, and the chain loop of
    tests/chain_ref.py over every step - the guided prediction of each window, the mean on shared frames, the posterior
    update.  Returns windows (n, 1, T, 88)."""
    import chain_ref as CR
    from diffroll_amd import longform
    steps = int(hp["timesteps"])
    x = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    zs = longform.gather_windows(noise.reshape(steps, plan.T_c, 88), plan).unsqueeze(2)
    spec = None
    if sampler != "generation_ddpm_x0":
        spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    return CR.sample_chain(p, hp, sampler, x, spec, zs, 0, w=w, plan=plan)


def run_plan_windows(m, plan, wav, x_T, noise, seed=0, recording=0, use_graph=True):
    """sample_long's chain over the windows of one recording's plan, keeping the windows: (n, T, 88) on the host."""
    from diffroll_amd import longform
    batch = longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)
    return m._sample_windows(batch, None if wav is None else [wav], [x_T], None if noise is None else [noise], 1, seed,
                             recording, use_graph, True).cpu()


def assert_shared_frames_agree(win, plan):
    for b in range(plan.n - 1):
        assert torch.equal(win[b, plan.stride:], win[b + 1, :plan.overlap]), b


# ---------------------------------------------------------------------------------------------- the trained fixture
def load_trained(golden_dir):
    z = np.load(os.path.join(golden_dir, "trained_small.npz"))
    return {k: z[k] for k in z.files}


def trained_noise(g):
    """x_T and the injected z's, regenerated from the stored seed exactly as make_golden.seeded_noise drew them."""
    hp = json.loads(str(g["hp"]))
    steps, (B, Tn, _) = int(hp["timesteps"]), g["label"].shape
    gen = torch.Generator().manual_seed(int(g["noise_seed"]))
    x_T = torch.randn(B, 1, Tn, 88, generator=gen)
    noise = torch.randn(steps, B, 1, Tn, 88, generator=gen)

    def bits(t):
        b = t.contiguous().view(torch.int32).to(torch.int64)
        return [int(b.sum()), int((b >> 9).sum())]
    if bits(x_T) != [int(v) for v in g["x_T_bits"]] or bits(noise) != [int(v) for v in g["noise_bits"]] \
            or not np.array_equal(noise[steps - 1].numpy(), g["noise_last"]):
        pytest.fail("torch's CPU generator does not reproduce the fixture's noise on this machine "
                    "(trained_small.npz stores the seed, not the 18 MB of draws): the comparison would be meaningless")
    return x_T, noise


def ckpt_path(golden_dir):
    return os.path.join(golden_dir, "trained_small.ckpt")


def trained_params(golden_dir, g):
    ck = torch.load(ckpt_path(golden_dir), map_location="cpu", weights_only=False)
    p = {k: v for k, v in ck["state_dict"].items() if not k.startswith("mel_layer")}
    wsum = float(sum(v.double().abs().sum().item() for v in p.values()))
    assert wsum == float(g["wsum"]), "checkpoint and fixture were not generated together"
    return ck, p


# ---------------------------------------------------------------------------------------------- source text and sockets
def header_functions(name="diffroll_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dr_[a-z_0-9]+)\s*\(", text)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
