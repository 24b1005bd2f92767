"""CPU restatement of chains under option "solver_noise" (include/diffroll_amd.h) - test infrastructure.

The stochastic form of the solver of tests/dpmpp_ref.py (SDE-DPM-Solver++, Lu et al. 2022: first order and 2M) on the x0
prediction, over the visited steps of tests/respaced_ref.py: the rows in float64 from the committed fp32 scalars (one
rounding to fp32), the fp32 expression order of solver_quad in diffroll_amd/csrc/update_quad.h, a chain loop built from
respaced_ref's prediction and shared-frame mean - and, in float64, the exact covariance propagation of a chain on a
Gaussian prior (the integrator's own error, no network).
"""
from typing import List, Optional

import numpy as np
import torch

from oracle import diffroll_ref as R

import dpmpp_ref as DR
import respaced_ref as RR


def rows64(AS: np.ndarray, steps: List[int], order: int, noise: int = 1) -> dict:
    """t -> float64 row [(Smp / Sm) exp(-h), Ap (-expm1(-2h)), A, c, Smp sqrt(-expm1(-2h))] of visited step t, c as
    dpmpp_ref.rows64; noise = 0: dpmpp_ref's rows.  AS: (S, 2) float64 A / Sm per step."""
    det = DR.rows64(AS, steps, order)
    if not noise:
        return det
    lam = np.log(AS[:, 0] / AS[:, 1])
    out = {}
    for i, t in enumerate(steps):
        A, Sm = AS[t]
        if t == 0:
            out[t] = np.array([0.0, 0.0, A, 0.0, 0.0])
            continue
        Ap, Smp = AS[steps[i + 1]]
        h = lam[steps[i + 1]] - lam[t]
        g = -np.expm1(-2.0 * h)
        out[t] = np.array([(Smp / Sm) * np.exp(-h), Ap * g, A, det[t][3], Smp * np.sqrt(g)])
    return out


def rows(hp, n: int, order: int, noise: int = 1) -> dict:
    """t -> (5,) fp32 row of visited step t of the n-step chain: float64 from the committed fp32 scalars, rounded once."""
    steps = RR.visited(int(hp["timesteps"]), n)
    return {t: r.astype(np.float32) for t, r in rows64(DR.scalars(hp), steps, order, noise).items()}


def update(t: int, row: np.ndarray, x: torch.Tensor, y: torch.Tensor, p: Optional[torch.Tensor],
           z: Optional[torch.Tensor]) -> torch.Tensor:
    """solver_quad's expressions, one rounding per operation in the tensors' dtype: y the prediction, p the previous
    step's, z the step's noise (read where the row's c4 is not 0)."""
    c0, c1, c2, c, c4 = (torch.tensor(float(v), dtype=x.dtype) for v in row)
    if t == 0:
        return y / c2
    d = y + c * (y - p) if float(c) != 0.0 else y
    o = c0 * x + c1 * d
    return o + c4 * z if float(c4) != 0.0 else o


def sample_chain(params, hp, sampler: str, x_T: torch.Tensor, spec: Optional[torch.Tensor], noise, n: int, order: int,
                 w: float = 0.0, plan=None, guidance=None, trajectory: bool = False, solver_noise: int = 1,
                 start: Optional[int] = None):
    """respaced_ref.sample_chain's loop under solver order 1 / 2 with option "solver_noise": noise (S, B, 1, T, 88) or a
    dict t -> (B, 1, T, 88) - row t is the z of visited step t > 0.  guidance = (lo, hi): its interval; start: the visited
    step the chain begins at (x_T is x at that step; its row has c = 0)."""
    S = int(hp["timesteps"])
    steps = RR.visited(S, n)
    rw = rows(hp, n, order, solver_noise)
    lo, hi = (0, S - 1) if guidance is None else guidance
    table = R.build_embedding(S)
    if start is not None:
        steps = steps[steps.index(start):]
    x, prev, traj = x_T, None, []
    with torch.no_grad():
        for i, t in enumerate(steps):
            y = RR.prediction(params, hp, sampler, x, spec, t, w if lo <= t <= hi else 0.0, table)
            if plan is not None:
                y = RR.shared_mean(y, plan)
            row = rw[t].copy()
            if i == 0:
                row[3] = 0.0
            x = update(t, row, x, y, prev, noise[t] if t > 0 and solver_noise else None)
            prev = y
            traj.append(x)
    return torch.stack(traj, 0) if trajectory else x


def philox_rows(seed: int, keys: List[int], S: int, n: int, T: int) -> dict:
    """t -> (len(keys), 1, T, 88): the engine's Philox z of every visited step t > 0 of the n-step chain for the clips with
    sample keys `keys` (first_sample + row; under "draws" / sharding whatever key the row has) - oracle.philox replayed."""
    from oracle import philox
    return {t: torch.from_numpy(np.concatenate([philox.step_noise(seed, k, 1, T * 88, t) for k in keys], 0)).reshape(len(keys), 1, T, 88)
            for t in RR.visited(S, n) if t > 0}


def variance_error(AS: np.ndarray, steps: List[int], order: int, s2: float) -> float:
    """Relative error of the final variance of the stochastic chain on the prior N(0, s2), in float64 and in closed form.
    The denoiser of that prior is linear - E[x0 | x_t] = k_t x, k_t = A s2 / (A^2 s2 + Sm^2) - so the covariance of the
    state (x, previous prediction) propagates exactly: with M = [[c0 + c1 (1 + c) k, -c1 c], [k, 0]],
    Cov' = M Cov M^T + diag(c4^2, 0).  x at the first visited step has its exact marginal variance A^2 s2 + Sm^2; the
    last step is x0 = k_0 x / A_0.  Returns |Var(x0) / s2 - 1|."""
    rw = rows64(AS, steps, order, 1)
    k = AS[:, 0] * s2 / (AS[:, 0] ** 2 * s2 + AS[:, 1] ** 2)
    A, Sm = AS[steps[0]]
    cov = np.array([[A * A * s2 + Sm * Sm, 0.0], [0.0, 0.0]])
    for t in steps:
        c0, c1, c2, c, c4 = rw[t]
        if t == 0:
            return abs((k[t] / c2) ** 2 * cov[0, 0] / s2 - 1.0)
        M = np.array([[c0 + c1 * (1.0 + c) * k[t], -c1 * c], [k[t], 0.0]])
        cov = M @ cov @ M.T + np.diag([c4 * c4, 0.0])
    raise AssertionError("the chain does not end at step 0")
