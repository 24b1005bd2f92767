"""Option "window_blend" (include/diffroll_amd.h) restated on the CPU - test infrastructure: what a frame shared by two
windows takes of their guided predictions (blend / blend_groups, torch fp32, one rounding per operation, the lower window's
value first), and the chain loop of chain_ref.sample_chain with that blend as its hook (sample_chain) - in front of the
clamp of clip_ref or the thresholding of thresh_ref where a test passes one on."""
from typing import Callable, Optional

import torch

import chain_ref as CR
import thresh_ref as TR

MEAN, LINEAR, NEAREST = 0, 1, 2


def blend_pair(lo: torch.Tensor, up: torch.Tensor, O: int, mode: int) -> torch.Tensor:
    """lo / up (..., O, 88): the lower window's frames [H, T) and the upper window's frames [0, O) -> the shared value."""
    if mode == MEAN:
        return 0.5 * (lo + up)
    out = torch.empty_like(lo)
    for j in range(O):
        if mode == LINEAR:
            wu = torch.tensor(j + 1, dtype=torch.float32) / torch.tensor(O + 1, dtype=torch.float32)
            out[..., j, :] = lo[..., j, :] + wu * (up[..., j, :] - lo[..., j, :])
        elif mode == NEAREST:
            out[..., j, :] = lo[..., j, :] if j < (O + 1) // 2 else up[..., j, :]
        else:
            raise ValueError(f"window_blend {mode}")
    return out


def blend_groups(y: torch.Tensor, groups, H: int, O: int, mode: int) -> torch.Tensor:
    """y (B, ..., T, 88), groups as thresh_ref.window_groups: consecutive windows of a recording share O frames; every
    value is formed from the UNBLENDED predictions of the two windows (O <= T / 2: a frame has at most one partner)."""
    T = y.shape[-2]
    out = y.clone()
    for g in groups:
        for (b, _), (b1, _) in zip(g[:-1], g[1:]):
            m = blend_pair(y[b, ..., H:T, :], y[b1, ..., 0:O, :], O, mode)
            out[b, ..., H:T, :] = m
            out[b1, ..., 0:O, :] = m
    return out


def blend(y: torch.Tensor, plan, mode: int) -> torch.Tensor:
    """Windows (n, 1, T, 88) of ONE recording (longform.WindowPlan): chain_ref.shared_mean with the option's mode."""
    return blend_groups(y, TR.window_groups(plan.n, plan.overlap), plan.stride, plan.overlap, mode)


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, mode: int, O: int,
                 marks=(), draws: int = 1, after: Optional[Callable] = None, **kw):
    """chain_ref.sample_chain's arguments (plan=None: the blend is the hook's) for a window batch x (B, 1, T, 88) of overlap O
    with recording marks / draws as thresh_ref.window_groups reads them - the blend per recording.  after(t, y) -> y: what
    follows the blend on the prediction (clip_hook / thresh_hook below)."""
    B, T = x.shape[0], x.shape[-2]
    groups = TR.window_groups(B, O, marks, draws)

    def hook(t, y):
        y = blend_groups(y, groups, T - O, O, mode)
        return after(t, y) if after is not None else y

    return CR.sample_chain(params, hp, sampler, x, spec_c, noise, n, plan=None, hook=hook, **kw)


def clip_hook(code: int) -> Callable:
    """Option "x0_clip" behind the blend: clip_ref's clamp."""
    import clip_ref as CL
    return lambda t, y: y.clamp(*CL.BOUNDS[code])


def thresh_hook(code: int, v: int, groups, stats: dict) -> Callable:
    """Option "x0_threshold" behind the blend: thresh_ref's seven lines over the recordings' canvases; stats[t] = (G, 2) {q, s}."""
    def hook(t, y):
        y, stats[t] = TR.threshold(y, code, v, groups)
        return y
    return hook
