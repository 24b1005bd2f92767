"""CPU restatement of respaced chains (option "sampling_steps" of include/diffroll_amd.h) - test infrastructure.

Composed from oracle.diffroll_ref.denoise (the network), oracle.philox (the engine's noise), the header's rule for the
visited steps and their coefficient rows (float64 from the committed fp32 scalars, one rounding to fp32) and the fp32
expression order of the posterior update in diffroll_amd/csrc/update_quad.h.  The committed rows are the tables the
engine is handed (diffroll_amd.schedule.sampler_coef_tables, pinned to the reference by tests/test_oracle_golden.py).
"""
from typing import List, Optional

import numpy as np
import torch

from oracle import diffroll_ref as R
from oracle import philox

# sampler -> (coefficient family, guided branch: None / "uncond" (spec = -1) / "zero" (spec = 0))
SAMPLERS = {
    "ddpm_x0": (0, None), "cfdg_ddpm_x0": (0, "uncond"), "generation_ddpm_x0": (0, None),
    "inpainting_ddpm_x0": (0, "uncond"), "ddim_x0": (1, None), "cfdg_ddim_x0": (1, "zero"),
    "ddpm": (2, None), "ddim": (3, None), "ddim2ddpm": (4, None),
}


def visited(S: int, n: int) -> List[int]:
    """t_i = (2 i (S - 1) + (n - 1)) // (2 (n - 1)), i = n-1 .. 0; n = 0 or S: every step."""
    if n in (0, S):
        return list(range(S - 1, -1, -1))
    return [(2 * i * (S - 1) + (n - 1)) // (2 * (n - 1)) for i in range(n - 1, -1, -1)]


def committed(hp) -> np.ndarray:
    """(5, S, 5) fp32: the coefficient tables the engine holds."""
    from diffroll_amd.schedule import make_schedule, sampler_coef_tables
    return sampler_coef_tables(make_schedule(hp["beta_start"], hp["beta_end"], int(hp["timesteps"]))).numpy()


def derived_rows(A, Ap, Sm, Smp) -> np.ndarray:
    """(5, 5) fp32: the five families' rows for a step with sqrt_acp A / sqrt_1m_acp Sm and successor Ap / Smp."""
    A, Ap, Sm, Smp = (float(np.float32(v)) for v in (A, Ap, Sm, Smp))       # float64 of the fp32 scalars
    r2 = (A / Ap) * (A / Ap)
    sigma = (Smp / Sm) * np.sqrt(1.0 - r2)
    direction = np.sqrt(max(0.0, 1.0 - Ap * Ap - sigma * sigma))
    beta = 1.0 - r2
    rows = [[Ap, direction, A, Sm, sigma],
            [Ap, np.sqrt(1.0 - Ap * Ap), A, Sm, 0.0],
            [Ap / A, beta, Sm, np.sqrt(beta * Smp * Smp / (Sm * Sm)), 0.0],
            [Ap, Smp, A, Sm, 0.0],
            [Ap, direction, A, Sm, sigma]]
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def rows_for(tab: np.ndarray, steps: List[int]) -> dict:
    """t -> (5, 5) fp32 rows used at visited step t (committed when t == 0 or its successor is t - 1)."""
    out = {}
    for i, t in enumerate(steps):
        tp = steps[i + 1] if i + 1 < len(steps) else None
        if tp is None or tp == t - 1:
            out[t] = tab[:, t, :].copy()
        else:
            out[t] = derived_rows(tab[0, t, 2], tab[0, tp, 2], tab[0, t, 3], tab[0, tp, 3])
    return out


def update(family: int, t: int, row: np.ndarray, x: torch.Tensor, y: torch.Tensor, z: Optional[torch.Tensor]) -> torch.Tensor:
    """update_quad.h's expressions, one fp32 rounding per operation (y: x0 prediction, families 0/1; epsilon, 2-4)."""
    c0, c1, c2, c3, c4 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    if z is None:
        z = torch.zeros_like(x)
    if family <= 1:
        if t == 0:
            return y / c2
        t1 = c0 * y
        t2 = (c1 * (x - c2 * y)) / c3
        return (t1 + t2) + c4 * z if family == 0 else t1 + t2
    if family == 2:
        m = c0 * (x - (c1 * y) / c2)
        return m if t == 0 else m + c3 * z
    xe = (x - c3 * y) / c2
    if t == 0:
        return xe
    return c0 * xe + c1 * y if family == 3 else (c0 * xe + c1 * y) + c4 * z


def prediction(params, hp, sampler, x, spec_c, t, w, table):
    """The network output an update consumes: guided as task/diffusion.py:953 / :1039-1041 where the sampler guides."""
    family, branch = SAMPLERS[sampler]
    tt = torch.tensor(t).repeat(x.shape[0])
    if sampler == "generation_ddpm_x0":
        spec_u = R.uncond_spec(params, hp, torch.empty(x.shape[0], int(hp["n_mels"]), x.shape[2]))
        return R.denoise(params, hp, x, spec_u, tt, table)
    y_c = R.denoise(params, hp, x, spec_c, tt, table)
    if branch is None:
        return y_c
    spec_2 = R.uncond_spec(params, hp, spec_c) if branch == "uncond" else torch.zeros_like(spec_c)
    return (1 + w) * y_c - w * R.denoise(params, hp, x, spec_2, tt, table)


def shared_mean(y: torch.Tensor, plan) -> torch.Tensor:
    """Long-form windows (n, 1, T, 88): frames two windows share take the mean of both predictions."""
    ym = y.clone()
    H, O, T = plan.stride, plan.overlap, plan.T
    for b in range(plan.n - 1):
        m = 0.5 * (y[b, :, H:T] + y[b + 1, :, 0:O])
        ym[b, :, H:T] = m
        ym[b + 1, :, 0:O] = m
    return ym


def sample_chain(params, hp, sampler: str, x_T: torch.Tensor, spec_c: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                 n: int, w: float = 0.0, plan=None, trajectory: bool = False, interval=None, order: int = 0):
    """THE chain loop of the tests' restatements: predict -> shared-frame mean -> update, over the n visited steps (0: all).
    x_T (B, 1, T, 88), spec_c (B, n_mels, T) (conditional samplers), noise (S, B, 1, T, 88) - row t is the z of visited step
    t.  plan: long-form windows (B = plan.n), the shared-frame mean before each update (and in the solver's history).
    interval = (lo, hi): a guidance interval - the weight is w at lo <= t <= hi and 0 elsewhere, as the reference's sampler
    with hparams.sampling.w set per step; BOTH network branches are evaluated at every step and combined as
    (1 + w_t) c - w_t u, so this is the reference's arithmetic, not the engine's shortcut.
    order = 1 / 2: option "solver_order" - the rows and the update of tests/dpmpp_ref.py on the x0 prediction, no noise, the
    previous step's prediction carried along; 0: the sampler's own update.
    Returns the final roll, or every intermediate roll (n, B, 1, T, 88) with trajectory=True."""
    S = int(hp["timesteps"])
    steps = visited(S, n)
    family = SAMPLERS[sampler][0]
    if order:
        import dpmpp_ref                       # (builds on this module)
        rows = dpmpp_ref.rows(hp, n, order)
    else:
        rows = {t: r[family] for t, r in rows_for(committed(hp), steps).items()}
    lo, hi = (0, S - 1) if interval is None else interval
    table = R.build_embedding(S)
    x, prev, traj = x_T, None, []
    with torch.no_grad():
        for t in steps:
            y = prediction(params, hp, sampler, x, spec_c, t, w if lo <= t <= hi else 0.0, table)
            if plan is not None:
                y = shared_mean(y, plan)
            if order:
                x = dpmpp_ref.update(t, rows[t], x, y, prev)
            else:
                x = update(family, t, rows[t], x, y, noise[t] if family in (0, 2, 4) and t > 0 else None)
            prev = y
            traj.append(x)
    return torch.stack(traj, 0) if trajectory else x


def philox_noise(seed: int, first_sample: int, S: int, B: int, T: int) -> torch.Tensor:
    """The injected-noise tensor (S, B, 1, T, 88) equal to the engine's Philox draws (keyed by the real step)."""
    return philox.chain_noise(seed, first_sample, S, B, T)
