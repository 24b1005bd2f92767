"""Option "x0_threshold" (include/diffroll_amd.h) restated on the CPU - test infrastructure, in two parts: the option's
seven lines with torch.sort (group_stats / threshold: per roll, or per recording's canvas through the window groups), and the
chain loop of chain_ref.sample_chain with the thresholding as its hook, in place of clip_ref's clamp (sample_chain).  Every line rounds once in fp32, as the header states it; beside the roll the chain returns, per step
and group, q and whether s > r, so that a test can tell whether its inputs threshold at all."""
from typing import List, Optional

import numpy as np
import torch

import chain_ref as CR
import clip_ref as CL


def centre(code: int):
    """(m, r) of the range the option's x0_clip code names: both exact in fp32."""
    lo, hi = CL.BOUNDS[code]
    return (lo + hi) / 2, (hi - lo) / 2


def clip_groups(B: int) -> List[List[tuple]]:
    """Every roll is a group of its own: [(row, first counted frame)]."""
    return [[(b, 0)] for b in range(B)]


def window_groups(B: int, O: int, marks=(), draws: int = 1) -> List[List[tuple]]:
    """The groups of a window batch: one per recording (marks: the windows of one draw that start a new recording; every
    draw starts new ones), each window contributing all its frames if it is its recording's first, else frames [O, T)."""
    n = B // draws
    groups = []
    for b in range(B):
        if b % n == 0 or (b % n) in marks:
            groups.append([(b, 0)])
        else:
            groups[-1].append((b, O))
    return groups


def shared_mean(y: torch.Tensor, groups, H: int, O: int) -> torch.Tensor:
    """chain_ref.shared_mean for any recordings: consecutive windows of a group share O frames, lower + upper."""
    T = y.shape[-2]
    ym = y.clone()
    for g in groups:
        for (b, _), (b1, _) in zip(g[:-1], g[1:]):
            m = 0.5 * (y[b, ..., H:T, :] + y[b1, ..., 0:O, :])
            ym[b, ..., H:T, :] = m
            ym[b1, ..., 0:O, :] = m
    return ym


def quantile(u: torch.Tensor, v: int) -> torch.Tensor:
    """Lines 2-5: a = |u| sorted ascending as bit patterns with the sign cleared, num = v (N - 1), k, rem = divmod(num,
    10000), q = a[k] or a[k] + f (a[k + 1] - a[k]) with f = fp32(rem / 10000), one fp32 rounding per operation."""
    bits = u.contiguous().reshape(-1).view(torch.int32) & 0x7FFFFFFF
    a = bits.sort().values.view(torch.float32)
    k, rem = divmod(int(v) * (a.numel() - 1), 10000)
    if rem == 0:
        return a[k].clone()
    f = torch.tensor(np.float32(rem / 10000.0))
    return a[k] + f * (a[k + 1] - a[k])


def group_stats(y: torch.Tensor, code: int, v: int, groups) -> torch.Tensor:
    """(G, 2) fp32 {q, s} of the groups of y (B, ..., T, 88)."""
    m, r = centre(code)
    out = torch.empty(len(groups), 2, dtype=torch.float32)
    for g, rows in enumerate(groups):
        u = torch.cat([(y[b, ..., f0:, :] - m).reshape(-1) for b, f0 in rows])
        q = quantile(u, v)
        out[g, 0] = q
        out[g, 1] = q if bool(q > r) else r            # (a NaN q gives s = r)
    return out


def threshold(y: torch.Tensor, code: int, v: int, groups):
    """The seven lines: (y', (G, 2) {q, s}).  A group whose s does not exceed r takes the static clamp itself."""
    m, r = centre(code)
    lo, hi = CL.BOUNDS[code]
    qs = group_stats(y, code, v, groups)
    out = y.clone()
    for g, rows in enumerate(groups):
        s = qs[g, 1]
        for b, _ in rows:
            if bool(s > r):
                out[b] = m + ((y[b] - m).clamp(-s, s) * r) / s
            else:
                out[b] = y[b].clamp(lo, hi)
    return out, qs


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, code: int, v: int,
                 plan=None, **kw):
    """clip_ref.sample_chain's arguments and v, the option's value (0: the clipped chain).  Returns (the final roll - or the
    trajectory -, {t: (G, 2) {q, s}} over the steps run, r)."""
    assert CR.SAMPLERS[sampler][0] <= 1 and code, "the threshold refines x0_clip on an x0 prediction"
    groups = clip_groups(x.shape[0]) if plan is None else window_groups(plan.n, plan.overlap)
    stats = {}

    def hook(t, y):
        if not v:
            return y.clamp(*CL.BOUNDS[code])
        y, stats[t] = threshold(y, code, v, groups)               # in place of the clamp
        return y

    return CR.sample_chain(params, hp, sampler, x, spec_c, noise, n, plan=plan, hook=hook, **kw), stats, centre(code)[1]


def active(stats, r) -> List[bool]:
    """s > r of every (step, group) visited."""
    return [bool(qs[g, 1] > r) for qs in stats.values() for g in range(qs.shape[0])]
