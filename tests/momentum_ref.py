"""Option "cfg_momentum" (include/diffroll_amd.h) restated on the CPU - test infrastructure.  The recurrence m = d + (bf *
m_prev) of d = y - c in torch fp32, every operation its own rounding; the coefficients (a, b) of the groups over yb = c + m by
project_ref's group_sums / coefficients, applied by its apply; and the chain loop of project_ref.sample_chain with the state
carried from one guided step to the next (sample_chain).  Nothing of project_ref or chain_ref is edited."""
from typing import Optional

import numpy as np
import torch

import blend_ref as BR
import chain_ref as CR
import clip_ref as CL
import project_ref as PR
import thresh_ref as TR


def factor(beta: int) -> torch.Tensor:
    """bf = (float)((double)cfg_momentum / 10000.0) as a 0-d fp32 tensor."""
    return torch.tensor(np.float32(np.float64(beta) / np.float64(10000.0)))


def recurrence(y: torch.Tensor, c: torch.Tensor, m_prev: Optional[torch.Tensor], beta: int):
    """(m, yb): d = y - c; m = d where m_prev is None (the step starts the state), else d + (bf * m_prev); yb = c + m - fp32,
    each operation rounded once (three separate torch operations: no fused multiply-add)."""
    d = y - c
    if m_prev is None:
        m = d
    else:
        bp = factor(beta) * m_prev
        m = d + bp
    return m, c + m


def group_ab(c: torch.Tensor, u: Optional[torch.Tensor], w: float, m_prev: Optional[torch.Tensor], beta: int, project: int, norm: int,
             groups, plan=None):
    """((G, 2) fp32 (a, b) of the groups over yb, m (the state the step leaves)) of the predictions c / u (B, ..., T, 88)
    combined with weight w; plan = (O, mode): a window batch, y and c each blended over the shared frames first."""
    c, y = PR.blended(c, u, w, groups, plan)
    with np.errstate(all="ignore"):
        m, yb = recurrence(y, c, m_prev, beta)
    out = np.empty((len(groups), 2), dtype=np.float32)
    for i, rows in enumerate(groups):
        out[i] = PR.coefficients(project, norm, w, *PR.group_sums(c, yb, rows))
    return out, m


def explicit_sum(ds, beta: int) -> torch.Tensor:
    """m_t = sum_j beta^j d_{t-j} in float64 over the list ds = [d_0, .., d_t] (bf as the kernels round it)."""
    bf = float(factor(beta))
    out = torch.zeros_like(ds[0], dtype=torch.float64)
    for j, d in enumerate(reversed(ds)):
        out = out + (bf ** j) * d.to(torch.float64)
    return out


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, cfg_momentum: int = 0,
                 cfg_project: int = 0, cfg_norm: int = 0, w: float = 0.0, code: int = 0, O: int = 0, mode: int = 0, marks=(), draws: int = 1,
                 interval=None, order: int = 0, solver_noise: int = 0, start: Optional[int] = None):
    """project_ref.sample_chain with the momentum: at a step that guides, y and c after the blend -> m, yb by the recurrence
    (the first guided step the chain runs starts the state; a step that does not guide neither reads nor writes it) -> (a, b)
    per group over yb -> y' = (a c) + (b yb) -> the clamp of code -> update.  cfg_momentum = 0: project_ref's chain, bit for bit.
    Returns (the final roll, {t: [(k, rho, s, a, b) float64 per group]}, {t: (rms |m|, rms |d|)}) over the guided steps."""
    S = int(hp["timesteps"])
    family, branch = CR.SAMPLERS[sampler]
    B, T = x.shape[0], x.shape[-2]
    groups = TR.window_groups(B, O, marks, draws) if O else TR.clip_groups(B)
    noisy = solver_noise if order else family in (0, 2, 4)
    lo, hi = (0, S - 1) if interval is None else interval
    table = CR.R.build_embedding(S)
    prev, seen, state, rms = None, {}, None, {}
    with torch.no_grad():
        for t, row in CR.chain_rows(hp, sampler, n, order, solver_noise, start).items():
            guides = branch is not None and w != 0.0 and lo <= t <= hi
            y = CR.prediction(params, hp, sampler, x, spec_c, t, w if guides else 0.0, table)
            c = CR.prediction(params, hp, sampler, x, spec_c, t, 0.0, table) if guides and (cfg_project or cfg_norm) else None
            if O:
                y = BR.blend_groups(y, groups, T - O, O, mode)
                c = BR.blend_groups(c, groups, T - O, O, mode) if c is not None else None
            if c is not None:
                if cfg_momentum:
                    state, yb = recurrence(y, c, state, cfg_momentum)
                    d = (y - c).double()
                    rms[t] = (float(state.double().pow(2).mean().sqrt()), float(d.pow(2).mean().sqrt()))
                    y = yb
                ab = np.empty((len(groups), 2), dtype=np.float32)
                seen[t] = []
                for i, rows in enumerate(groups):
                    sums = PR.group_sums(c, y, rows)
                    ab[i] = PR.coefficients(cfg_project, cfg_norm, w, *sums)
                    seen[t].append(PR.parts(cfg_project, cfg_norm, w, *sums))
                y = PR.apply(c, y, ab, groups)
            if code:
                y = y.clamp(*CL.BOUNDS[code])
            z = noise[t] if noisy and t > 0 else None
            x = CR.solver_update(t, row, x, y, prev, z) if order else CR.update(family, t, row, x, y, z)
            prev = y
    return x, seen, rms
