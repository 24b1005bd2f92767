"""CPU restatement of chains under option "solver_order" (include/diffroll_amd.h) - test infrastructure.

The first-order exponential integrator in lambda = log(sqrt_acp / sqrt_1m_acp) and DPM-Solver++ (2M) (Lu et al. 2022) on
the x0 prediction, over the visited steps of tests/respaced_ref.py: the rows in float64 from the committed fp32 scalars
(one rounding to fp32) and the fp32 expression order of solver_quad in diffroll_amd/csrc/update_quad.h, which the chain loop of
respaced_ref runs under order = 1 / 2 - and a float64 variant of the pure integrator that takes any denoiser.
"""
from typing import Callable, List, Optional

import numpy as np
import torch

import respaced_ref as RR


def scalars(hp) -> np.ndarray:
    """(S, 2) float64 of the committed fp32 sqrt_acp / sqrt_1m_acp (family 0, columns 2 and 3)."""
    return RR.committed(hp)[0, :, 2:4].astype(np.float64)


def rows64(AS: np.ndarray, steps: List[int], order: int) -> dict:
    """t -> float64 row [Smp / Sm, -Ap expm1(-h), A, c, 0] of visited step t; AS: (S, 2) float64 A / Sm per step."""
    lam = np.log(AS[:, 0] / AS[:, 1])
    out = {}
    for i, t in enumerate(steps):
        A, Sm = AS[t]
        if t == 0:
            out[t] = np.array([0.0, 0.0, A, 0.0, 0.0])
            continue
        tp = steps[i + 1]
        Ap, Smp = AS[tp]
        h = lam[tp] - lam[t]
        c = h / (2.0 * (lam[t] - lam[steps[i - 1]])) if order == 2 and i > 0 and tp != 0 else 0.0
        out[t] = np.array([Smp / Sm, -Ap * np.expm1(-h), A, c, 0.0])
    return out


def rows(hp, n: int, order: int) -> dict:
    """t -> (5,) fp32 row of visited step t of the n-step chain: float64 from the committed fp32 scalars, rounded once."""
    steps = RR.visited(int(hp["timesteps"]), n)
    return {t: r.astype(np.float32) for t, r in rows64(scalars(hp), steps, order).items()}


def update(t: int, row: np.ndarray, x: torch.Tensor, y: torch.Tensor, p: Optional[torch.Tensor]) -> torch.Tensor:
    """solver_quad's expressions, one fp32 rounding per operation: y the prediction, p the previous step's."""
    c0, c1, c2, c = (torch.tensor(float(v), dtype=torch.float32) for v in row[:4])
    if t == 0:
        return y / c2
    d = y + c * (y - p) if float(c) != 0.0 else y
    return c0 * x + c1 * d


def sample_chain(params, hp, sampler: str, x_T: torch.Tensor, spec: Optional[torch.Tensor], n: int, order: int,
                 w: float = 0.0, plan=None, guidance=None, trajectory: bool = False):
    """respaced_ref.sample_chain under solver order 1 / 2 (no noise); guidance = (lo, hi): its interval."""
    return RR.sample_chain(params, hp, sampler, x_T, spec, None, n, w, plan, trajectory, interval=guidance, order=order)


def integrate64(denoise: Callable, AS: np.ndarray, steps: List[int], order: int, x_T: np.ndarray, final: bool = True):
    """The pure integrator in float64: denoise(x, t) -> x0 prediction; AS (S, 2) float64 A / Sm.  final=False returns the
    state BEFORE the last step's y / A_0 (the state at t = 0)."""
    rw = rows64(AS, steps, order)
    x, p = np.asarray(x_T, dtype=np.float64), None
    for t in steps:
        if t == 0:
            return denoise(x, t) / rw[t][2] if final else x
        y = denoise(x, t)
        c0, c1, _, c, _ = rw[t]
        d = y + c * (y - p) if c != 0.0 else y
        x = c0 * x + c1 * d
        p = y
    return x
