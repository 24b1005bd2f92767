"""Option "cfg_rescale" (include/diffroll_amd.h) restated on the CPU - test infrastructure, in two parts: the factor g of
every group in numpy float64 with the header's order of the sums, every addition written out (group_sums / factor /
group_g), and the chain loop with the rescale between the shared-frame blend and the clamp or thresholding (sample_chain).
The groups are thresh_ref's: [(row, first counted frame)] per clip or per recording's canvas."""
from typing import Optional

import numpy as np
import torch

import blend_ref as BR
import chain_ref as CR
import clip_ref as CL
import thresh_ref as TR

BLOCK = 64      # frames per block of a row's sums


def frame_sums(a: np.ndarray):
    """a (F, 88) fp32 -> (S1, S2) (F,) float64: each frame's 88 elements in pitch order, a sequential sum from 0.0 (the
    frames side by side; a square of an fp32 value is exact in float64)."""
    a = a.astype(np.float64)
    s1, s2 = np.zeros(a.shape[0]), np.zeros(a.shape[0])
    for p in range(a.shape[1]):
        s1 = s1 + a[:, p]
        s2 = s2 + a[:, p] * a[:, p]
    return s1, s2


def group_sums(a: torch.Tensor, rows):
    """(N, S1, S2) of one group of a (B, ..., T, 88): per row the counted frames [f0, T) in blocks of BLOCK from f0, a block's
    frames in frame order; the group's blocks in row, then block order; every level a sequential sum from 0.0."""
    N, S1, S2 = 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        for b, f0 in rows:
            s1, s2 = frame_sums(a[b].reshape(-1, 88)[f0:].numpy())
            N += s1.shape[0] * 88
            for j0 in range(0, s1.shape[0], BLOCK):
                b1, b2 = 0.0, 0.0
                for j in range(j0, min(j0 + BLOCK, s1.shape[0])):
                    b1 = b1 + s1[j]
                    b2 = b2 + s2[j]
                S1 = S1 + b1
                S2 = S2 + b2
    return N, S1, S2


def factor(value: int, N: int, S1c, S2c, S1y, S2y) -> np.float32:
    """g of a group from its sums, every operation rounded once in float64; 1.0f where the header says so."""
    with np.errstate(all="ignore"):
        N = np.float64(N)
        S1c, S2c, S1y, S2y = (np.float64(s) for s in (S1c, S2c, S1y, S2y))
        mc, my = S1c / N, S1y / N
        Vc, Vy = S2c - S1c * mc, S2y - S1y * my
        if not Vy > 0.0 or not Vc >= 0.0:
            return np.float32(1.0)
        rho = np.sqrt(Vc / Vy)
        phid = np.float64(value) / np.float64(10000.0)
        g = np.float32(np.float64(1.0) + phid * (rho - np.float64(1.0)))
    return g if np.isfinite(g) else np.float32(1.0)


def guided(c: torch.Tensor, u: Optional[torch.Tensor], w: float) -> torch.Tensor:
    """(1 + w) c - w u in fp32, 1 + w formed in double and rounded once (guided_quad); c alone without u."""
    return c if u is None else (1 + w) * c - w * u


def group_g(c: torch.Tensor, u: Optional[torch.Tensor], w: float, value: int, groups, plan=None) -> np.ndarray:
    """(G,) fp32: g of the groups of the predictions c / u (B, ..., T, 88) combined with weight w.  plan = (O, mode): a window
    batch - y and c each go through the blend of the frames consecutive windows of a group share (blend_ref.blend_groups)."""
    y = guided(c, u, w)
    if plan is not None:
        O, mode = plan
        H = c.shape[-2] - O
        y, c = BR.blend_groups(y, groups, H, O, mode), BR.blend_groups(c, groups, H, O, mode)
    out = np.empty(len(groups), dtype=np.float32)
    for i, rows in enumerate(groups):
        N, S1c, S2c = group_sums(c, rows)
        _, S1y, S2y = group_sums(y, rows)
        out[i] = factor(value, N, S1c, S2c, S1y, S2y)
    return out


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, cfg_rescale: int, w: float = 0.0,
                 code: int = 0, v: int = 0, O: int = 0, mode: int = 0, marks=(), draws: int = 1, interval=None, order: int = 0,
                 solver_noise: int = 0, start: Optional[int] = None):
    """The chain of chain_ref.sample_chain with the rescale: predict y (weight w) and c (weight 0) -> blend both over the
    shared frames (O > 0: a window batch with recording marks / draws as thresh_ref.window_groups reads them) -> at a step
    that guides y = g y per group -> the clamp of code / the thresholding at v -> update.  cfg_rescale = 0: the option off.
    Returns (the final roll, {t: (G,) fp32 g} over the guided steps)."""
    S = int(hp["timesteps"])
    family, branch = CR.SAMPLERS[sampler]
    B, T = x.shape[0], x.shape[-2]
    groups = TR.window_groups(B, O, marks, draws) if O else TR.clip_groups(B)
    noisy = solver_noise if order else family in (0, 2, 4)
    lo, hi = (0, S - 1) if interval is None else interval
    table = CR.R.build_embedding(S)
    prev, gs = None, {}
    with torch.no_grad():
        for t, row in CR.chain_rows(hp, sampler, n, order, solver_noise, start).items():
            guides = branch is not None and w != 0.0 and lo <= t <= hi
            y = CR.prediction(params, hp, sampler, x, spec_c, t, w if guides else 0.0, table)
            c = CR.prediction(params, hp, sampler, x, spec_c, t, 0.0, table) if guides and cfg_rescale else None
            if O:
                y = BR.blend_groups(y, groups, T - O, O, mode)
                c = BR.blend_groups(c, groups, T - O, O, mode) if c is not None else None
            if c is not None:
                g = np.empty(len(groups), dtype=np.float32)
                y = y.clone()
                for i, rows in enumerate(groups):
                    N, S1c, S2c = group_sums(c, rows)
                    _, S1y, S2y = group_sums(y, rows)
                    g[i] = factor(cfg_rescale, N, S1c, S2c, S1y, S2y)
                for i, rows in enumerate(groups):
                    for b, _ in rows:
                        y[b] = torch.tensor(g[i]) * y[b]
                gs[t] = g
            if v:
                y, _ = TR.threshold(y, code, v, groups)
            elif code:
                y = y.clamp(*CL.BOUNDS[code])
            z = noise[t] if noisy and t > 0 else None
            x = CR.solver_update(t, row, x, y, prev, z) if order else CR.update(family, t, row, x, y, z)
            prev = y
    return x, gs
