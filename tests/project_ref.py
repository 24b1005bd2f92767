"""Options "cfg_project" / "cfg_norm" (include/diffroll_amd.h) restated on the CPU - test infrastructure, in two parts: the
coefficients (a, b) of every group in numpy float64 with the header's order of the sums, every addition written out
(group_sums / coefficients / group_ab), and the chain loop with the projected step between the shared-frame blend and the
clamp (sample_chain).  The groups are thresh_ref's: [(row, first counted frame)] per clip or per recording's canvas."""
from typing import Optional

import numpy as np
import torch

import blend_ref as BR
import chain_ref as CR
import clip_ref as CL
import thresh_ref as TR
from rescale_ref import BLOCK, guided


def frame_sums(c: np.ndarray, y: np.ndarray):
    """c, y (F, 88) fp32 -> (Scc, Scd, Sdd) (F,) float64: each frame's 88 elements in pitch order, a sequential sum from 0.0
    (the frames side by side); d = (double)y - (double)c, every difference, product and addition rounded once."""
    c, y = c.astype(np.float64), y.astype(np.float64)
    scc, scd, sdd = np.zeros(c.shape[0]), np.zeros(c.shape[0]), np.zeros(c.shape[0])
    for p in range(c.shape[1]):
        d = y[:, p] - c[:, p]
        scc = scc + c[:, p] * c[:, p]
        scd = scd + c[:, p] * d
        sdd = sdd + d * d
    return scc, scd, sdd


def group_sums(c: torch.Tensor, y: torch.Tensor, rows):
    """(N, Scc, Scd, Sdd) of one group of c, y (B, ..., T, 88): per row the counted frames [f0, T) in blocks of BLOCK from f0,
    a block's frames in frame order; the group's blocks in row, then block order; every level a sequential sum from 0.0."""
    N, S = 0, [0.0, 0.0, 0.0]
    with np.errstate(all="ignore"):
        for b, f0 in rows:
            fs = frame_sums(c[b].reshape(-1, 88)[f0:].numpy(), y[b].reshape(-1, 88)[f0:].numpy())
            F = fs[0].shape[0]
            N += F * 88
            for j0 in range(0, F, BLOCK):
                blk = [0.0, 0.0, 0.0]
                for j in range(j0, min(j0 + BLOCK, F)):
                    for k in range(3):
                        blk[k] = blk[k] + fs[k][j]
                for k in range(3):
                    S[k] = S[k] + blk[k]
    return N, S[0], S[1], S[2]


def parts(project: int, norm: int, w: float, N: int, Scc, Scd, Sdd):
    """(k, rho, s, a, b) of a group in float64, before the cast to fp32 - every operation rounded once."""
    with np.errstate(all="ignore"):
        N = np.float64(N)
        Scc, Scd, Sdd = (np.float64(v) for v in (Scc, Scd, Sdd))
        k = Scd / Scc if Scc > 0.0 else np.float64(0.0)
        rho = np.float64(project) / np.float64(10000.0)
        s = np.float64(1.0)
        if norm != 0:
            r = np.float64(norm) / np.float64(10000.0)
            q = np.sqrt(Sdd / N) / np.abs(np.float64(np.float32(w)))
            if q > r:
                s = r / q
        a = (np.float64(1.0) - s) - s * (rho * k)
    return k, rho, s, a, s


def coefficients(project: int, norm: int, w: float, N: int, Scc, Scd, Sdd):
    """(a, b) of a group from its sums as fp32; (0.0f, 1.0f) where either is not finite."""
    _, _, _, a, b = parts(project, norm, w, N, Scc, Scd, Sdd)
    with np.errstate(all="ignore"):
        a, b = np.float32(a), np.float32(b)
    if not np.isfinite(a) or not np.isfinite(b):
        return np.float32(0.0), np.float32(1.0)
    return a, b


def blended(c, u, w, groups, plan):
    """(c, y) as the statistics and the update see them: the guided prediction at weight w and the conditional one, each put
    through the blend of the frames consecutive windows of a group share (plan = (O, mode); None: clips)."""
    y = guided(c, u, w)
    if plan is not None:
        O, mode = plan
        H = c.shape[-2] - O
        y, c = BR.blend_groups(y, groups, H, O, mode), BR.blend_groups(c, groups, H, O, mode)
    return c, y


def group_ab(c: torch.Tensor, u: Optional[torch.Tensor], w: float, project: int, norm: int, groups, plan=None) -> np.ndarray:
    """(G, 2) fp32: (a, b) of the groups of the predictions c / u (B, ..., T, 88) combined with weight w."""
    c, y = blended(c, u, w, groups, plan)
    out = np.empty((len(groups), 2), dtype=np.float32)
    for i, rows in enumerate(groups):
        out[i] = coefficients(project, norm, w, *group_sums(c, y, rows))
    return out


def apply(c: torch.Tensor, y: torch.Tensor, ab: np.ndarray, groups) -> torch.Tensor:
    """y' = (a c) + (b y) in fp32 per group, each operation rounded once; y itself where a == 0.0f and b == 1.0f."""
    y = y.clone()
    for (a, b), rows in zip(ab, groups):
        if a == np.float32(0.0) and b == np.float32(1.0):
            continue
        for r, _ in rows:
            y[r] = torch.tensor(a) * c[r] + torch.tensor(b) * y[r]
    return y


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, cfg_project: int = 0,
                 cfg_norm: int = 0, w: float = 0.0, code: int = 0, O: int = 0, mode: int = 0, marks=(), draws: int = 1, interval=None,
                 order: int = 0, solver_noise: int = 0, start: Optional[int] = None):
    """The chain of chain_ref.sample_chain with the projected step: predict y (weight w) and c (weight 0) -> blend both over
    the shared frames (O > 0: a window batch with recording marks / draws as thresh_ref.window_groups reads them) -> at a step
    that guides y = (a c) + (b y) per group -> the clamp of code -> update.  cfg_project = cfg_norm = 0: the options off.
    Returns (the final roll, {t: [(k, rho, s, a, b) float64 per group]} over the guided steps)."""
    S = int(hp["timesteps"])
    family, branch = CR.SAMPLERS[sampler]
    B, T = x.shape[0], x.shape[-2]
    groups = TR.window_groups(B, O, marks, draws) if O else TR.clip_groups(B)
    noisy = solver_noise if order else family in (0, 2, 4)
    lo, hi = (0, S - 1) if interval is None else interval
    table = CR.R.build_embedding(S)
    prev, seen = None, {}
    with torch.no_grad():
        for t, row in CR.chain_rows(hp, sampler, n, order, solver_noise, start).items():
            guides = branch is not None and w != 0.0 and lo <= t <= hi
            y = CR.prediction(params, hp, sampler, x, spec_c, t, w if guides else 0.0, table)
            c = CR.prediction(params, hp, sampler, x, spec_c, t, 0.0, table) if guides and (cfg_project or cfg_norm) else None
            if O:
                y = BR.blend_groups(y, groups, T - O, O, mode)
                c = BR.blend_groups(c, groups, T - O, O, mode) if c is not None else None
            if c is not None:
                ab = np.empty((len(groups), 2), dtype=np.float32)
                seen[t] = []
                for i, rows in enumerate(groups):
                    sums = group_sums(c, y, rows)
                    ab[i] = coefficients(cfg_project, cfg_norm, w, *sums)
                    seen[t].append(parts(cfg_project, cfg_norm, w, *sums))
                y = apply(c, y, ab, groups)
            if code:
                y = y.clamp(*CL.BOUNDS[code])
            z = noise[t] if noisy and t > 0 else None
            x = CR.solver_update(t, row, x, y, prev, z) if order else CR.update(family, t, row, x, y, z)
            prev = y
    return x, seen
