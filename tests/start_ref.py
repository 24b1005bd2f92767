"""CPU restatement of chains that start at an intermediate step (options "start_step" / "start_noise" of
include/diffroll_amd.h) - test infrastructure.

The chain loop of tests/respaced_ref.py entered in the middle: the visited steps t <= t_s with the rows the whole chain uses
at them (keyed by the real t), the updates of respaced_ref / dpmpp_ref, and under solver order 2 a first started row with
c = 0.  The forward diffusion of a clean roll is the fp32 expression of dr_q_sample, (A * x0) + (Sm * z), with z from
oracle.philox.step_noise at the step word timesteps + t_s - for windows one canvas draw per recording, gathered.
"""
from typing import Optional

import numpy as np
import torch

from oracle import diffroll_ref as R
from oracle import philox

import dpmpp_ref as DR
import respaced_ref as RR


def start_of(S: int, n: int, t_s: int) -> int:
    """The effective start step: t_s, or the chain's first visited step for -1."""
    return RR.visited(S, n)[0] if t_s < 0 else t_s


def diffuse(hp, x0: torch.Tensor, t_s: int, z: torch.Tensor) -> torch.Tensor:
    """(A * x0) + (Sm * z) in fp32, each product rounded once, then the sum: A / Sm the committed scalars of step t_s."""
    tab = RR.committed(hp)
    A, Sm = (torch.tensor(float(tab[0, t_s, c]), dtype=torch.float32) for c in (2, 3))
    return (A * x0.to(torch.float32)) + (Sm * z.to(torch.float32))


def diffusion_noise(seed: int, first_sample: int, S: int, B: int, T: int, t_s: int) -> torch.Tensor:
    """(B, 1, T, 88): the engine's Philox z of the diffusion to t_s for rows first_sample .. first_sample + B - 1."""
    return torch.from_numpy(philox.step_noise(seed, first_sample, B, T * 88, S + t_s).reshape(B, 1, T, 88).copy())


def window_noise(seed: int, recording: int, S: int, plan, t_s: int) -> torch.Tensor:
    """(n, 1, T, 88): one canvas draw of the recording (keyed by the canvas element), gathered into its windows."""
    from diffroll_amd import longform
    canvas = torch.from_numpy(philox.step_noise(seed, recording, 1, plan.T_c * 88, S + t_s).reshape(plan.T_c, 88).copy())
    return longform.gather_windows(canvas, plan).unsqueeze(1)


def rows_of(hp, sampler: str, n: int, order: int, t_s: int) -> dict:
    """t -> the row the started chain reads at visited step t <= t_s: the whole chain's row, except that under a solver
    order the first started step has c = 0 (it has no previous prediction)."""
    S = int(hp["timesteps"])
    steps = RR.visited(S, n)
    i0 = steps.index(start_of(S, n, t_s))
    if order:
        rows = dict(DR.rows(hp, n, order))
        first = rows[steps[i0]].copy()
        first[3] = 0.0
        rows[steps[i0]] = first
    else:
        family = RR.SAMPLERS[sampler][0]
        rows = {t: r[family] for t, r in RR.rows_for(RR.committed(hp), steps).items()}
    return {t: rows[t] for t in steps[i0:]}


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                 n: int, t_s: int = -1, w: float = 0.0, plan=None, trajectory: bool = False, interval=None, order: int = 0):
    """respaced_ref.sample_chain from the visited step t_s on: x (B, 1, T, 88) is x AT t_s; noise (S, B, 1, T, 88), row t the
    z of visited step t (None under a solver order).  Returns the final roll, or the rolls after each step run."""
    S = int(hp["timesteps"])
    rows = rows_of(hp, sampler, n, order, t_s)
    family = RR.SAMPLERS[sampler][0]
    lo, hi = (0, S - 1) if interval is None else interval
    table = R.build_embedding(S)
    prev, traj = None, []
    with torch.no_grad():
        for t in rows:                                 # (insertion order: chain order)
            y = RR.prediction(params, hp, sampler, x, spec_c, t, w if lo <= t <= hi else 0.0, table)
            if plan is not None:
                y = RR.shared_mean(y, plan)
            if order:
                x = DR.update(t, rows[t], x, y, prev)
            else:
                x = RR.update(family, t, rows[t], x, y, noise[t] if family in (0, 2, 4) and t > 0 else None)
            prev = y
            traj.append(x)
    return torch.stack(traj, 0) if trajectory else x


def refine_chain(params, hp, sampler: str, x0: torch.Tensor, spec_c, noise, n: int, t_s: int, z: torch.Tensor, **kw):
    """Option "start_noise": the clean roll x0 diffused to the start step with z, then the started chain."""
    t0 = start_of(int(hp["timesteps"]), n, t_s)
    return sample_chain(params, hp, sampler, diffuse(hp, x0, t0, z), spec_c, noise, n, t0, **kw)
