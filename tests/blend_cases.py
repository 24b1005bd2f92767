"""The inputs of the "window_blend" GPU tests (tests/test_gpu_window_blend.py) and their CPU references - test
infrastructure.  Each reference is computed once per process and shared, never modified: tests/test_window_blend_cpu.py
checks on the references alone that modes 1 and 2 move the final roll away from mode 0's by more than the parity bound, the
GPU tests hold the engine to the same tensors.

Shapes: three windows of T = 32 frames, 3 residual layers of 128 channels (k = 9), cfdg_ddpm_x0 at w = 0.5, injected noise on
the canvas; O = 1 (one shared frame: the hand-over's odd frame goes to the lower window), 5 (odd, wu = 1/6 .. 5/6) and 16
(= T / 2, the largest the engine accepts: every frame of the middle window is shared).  The option cases run at O = 5.  The
fused case is the shipping geometry: three 640-frame windows sharing 160 frames, 2 residual layers."""
import functools

import torch

from oracle import diffroll_ref as R

import blend_ref as BR
import thresh_ref as TR

from diffroll_amd import longform

HOP = 512
T, OS, W = 32, (1, 5, 16), 0.5
SAMPLER = "cfdg_ddpm_x0"
MODES = (1, 2)


def hp_of(layers=3, channels=128, steps=4, k=9):
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_layers=layers, kernel_size=k, timesteps=steps, residual_channels=channels)
    return hp


def plan_of(O, n=3, T=T):
    """n windows of T frames sharing O: a recording that just fills their canvas."""
    H = T - O
    L = ((n - 1) * H + T) * HOP - 100
    plan = longform.plan_windows(L, HOP, T, O)
    assert plan.n == n and plan.T_out == plan.T_c
    return plan, L


def windows_of(canvas, plan):
    """Canvas (..., T_c, 88) -> windows (..., n, 1, T, 88)."""
    return longform.gather_windows(canvas, plan).unsqueeze(-3)


@functools.lru_cache(maxsize=None)
def recording(O, seed, steps=4, n=3, T=T, layers=3, channels=128):
    """One recording: (hp, params, plan, wav (L,), x_T canvas (1, 1, T_c, 88), noise canvas (steps, 1, 1, T_c, 88), the windows'
    spectrograms)."""
    hp = hp_of(layers, channels, steps)
    p = R.synthetic_params(hp, seed=seed)
    g = torch.Generator().manual_seed(seed)
    plan, L = plan_of(O, n, T)
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    noise = torch.randn(steps, 1, 1, plan.T_c, 88, generator=g)
    spec = R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T)
    return hp, p, plan, wav, x_T, noise, spec


def case(O):
    return recording(O, 3200 + O)


@functools.lru_cache(maxsize=None)
def reference(O, mode):
    """The windows (3, 1, T, 88) after the chain of case(O) under `mode`."""
    hp, p, plan, _, x_T, noise, spec = case(O)
    x = windows_of(x_T.reshape(plan.T_c, 88), plan)
    z = windows_of(noise.reshape(-1, plan.T_c, 88), plan)
    return BR.sample_chain(p, hp, SAMPLER, x, spec, z, 0, mode=mode, O=O, w=W)


# ---------------------------------------------------------------------------------------------- the option cases, O = 5
OPT_O = 5
# name -> (what the chain runs under beside the blend; timesteps of the model)
OPTION_CASES = {
    "draws": dict(draws=2),
    "order2-steps": dict(order=2, steps=4, timesteps=8),
    "order2-steps-noise": dict(order=2, steps=4, timesteps=8, solver_noise=1),
    "clip": dict(code=1, w=3.0),
}


@functools.lru_cache(maxsize=None)
def option_reference(name, mode):
    """The windows after the chain of option case `name` under `mode` - (D * 3, 1, T, 88), draw-major."""
    kw = dict(OPTION_CASES[name])
    S = kw.pop("timesteps", 4)
    D = kw.pop("draws", 1)
    n = kw.pop("steps", 0)
    code = kw.pop("code", 0)
    w = kw.pop("w", W)
    hp, p, plan, _, _, _, spec = recording(OPT_O, 3300, S)
    x_T, noise = option_canvases(name)
    x = torch.cat([windows_of(x_T[d, 0], plan) for d in range(D)], 0)
    z = torch.cat([windows_of(noise[:, d, 0], plan) for d in range(D)], 1)
    after = BR.clip_hook(code) if code else None
    return BR.sample_chain(p, hp, SAMPLER, x, spec.repeat(D, 1, 1), z, n, mode=mode, O=OPT_O, draws=D, after=after, w=w, **kw)


@functools.lru_cache(maxsize=None)
def option_canvases(name):
    """(x_T (D, 1, T_c, 88), noise (S, D, 1, T_c, 88)) of an option case: draw 0 is the recording's own canvas pair."""
    kw = OPTION_CASES[name]
    S, D = kw.get("timesteps", 4), kw.get("draws", 1)
    _, _, plan, _, x_T, noise, _ = recording(OPT_O, 3300, S)
    g = torch.Generator().manual_seed(77)
    xs = [x_T] + [torch.randn(1, 1, plan.T_c, 88, generator=g) for _ in range(D - 1)]
    zs = [noise] + [torch.randn(S, 1, 1, plan.T_c, 88, generator=g) for _ in range(D - 1)]
    return torch.cat(xs, 0), torch.cat(zs, 1)


# "window_break": two recordings of 2 + 1 windows in one chain
@functools.lru_cache(maxsize=None)
def break_case():
    a = recording(OPT_O, 3400, n=2)
    b = recording(OPT_O, 3401, n=1)
    assert a[0] == b[0]
    return a, b


@functools.lru_cache(maxsize=None)
def break_reference(mode):
    a, b = break_case()
    hp, p = a[0], a[1]                                 # (one model: the first recording's parameters)
    x = torch.cat([windows_of(r[4].reshape(r[2].T_c, 88), r[2]) for r in (a, b)], 0)
    z = torch.cat([windows_of(r[5].reshape(-1, r[2].T_c, 88), r[2]) for r in (a, b)], 1)
    spec = torch.cat([a[6], b[6]], 0)
    return BR.sample_chain(p, hp, SAMPLER, x, spec, z, 0, mode=mode, O=OPT_O, marks=(2,), w=W)


# "x0_threshold": the guided active case of thresh_cases (w = 3, code 2, v = 9950) on these windows
THRESH = dict(w=3.0, code=2, v=9950)


@functools.lru_cache(maxsize=None)
def thresh_reference(mode):
    """(windows, {t: (1, 2) {q, s}}, r): one q per step over the recording's canvas, on the blended prediction."""
    hp, p, plan, _, x_T, noise, spec = recording(OPT_O, 3300)
    x = windows_of(x_T.reshape(plan.T_c, 88), plan)
    z = windows_of(noise.reshape(-1, plan.T_c, 88), plan)
    stats = {}
    groups = TR.window_groups(plan.n, OPT_O)
    after = BR.thresh_hook(THRESH["code"], THRESH["v"], groups, stats)
    roll = BR.sample_chain(p, hp, SAMPLER, x, spec, z, 0, mode=mode, O=OPT_O, after=after, w=THRESH["w"])
    return roll, stats, TR.centre(THRESH["code"])[1]


# ---------------------------------------------------------------------------------------------- the fused geometry
FUSED = dict(O=160, seed=3500, steps=4, n=3, T=640, layers=2, channels=512)


def fused_case():
    return recording(**FUSED)


@functools.lru_cache(maxsize=None)
def fused_reference(mode):
    hp, p, plan, _, x_T, noise, spec = fused_case()
    x = windows_of(x_T.reshape(plan.T_c, 88), plan)
    z = windows_of(noise.reshape(-1, plan.T_c, 88), plan)
    return BR.sample_chain(p, hp, SAMPLER, x, spec, z, 0, mode=mode, O=FUSED["O"], w=W)
