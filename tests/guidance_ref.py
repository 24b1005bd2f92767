"""CPU restatement of a chain under a guidance interval (options "guidance_t_min" / "guidance_t_max" of
include/diffroll_amd.h) - test infrastructure, built on tests/respaced_ref.py.

It is respaced_ref.sample_chain with a per-step weight: w where lo <= t <= hi, 0 elsewhere - the reference's sampler
(task/diffusion.py:943-969, :999-1025, :1027-1055) with self.hparams.sampling.w set per step.  BOTH network branches are
evaluated at every step and combined as (1 + w_t) c - w_t u: nothing here skips, so this is the reference's arithmetic, not
the engine's shortcut.
"""
from typing import Optional, Sequence

import torch

from oracle import diffroll_ref as R

import respaced_ref as RR


def step_weight(t: int, w: float, interval: Sequence[int]) -> float:
    lo, hi = interval
    return w if lo <= t <= hi else 0.0


def sample_chain(params, hp, sampler: str, x_T: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, w: float,
                 interval: Sequence[int], plan=None, trajectory: bool = False):
    """respaced_ref.sample_chain's arguments + interval = (lo, hi) in real diffusion steps (hi inclusive)."""
    S = int(hp["timesteps"])
    steps = RR.visited(S, n)
    rows = RR.rows_for(RR.committed(hp), steps)
    family = RR.SAMPLERS[sampler][0]
    table = R.build_embedding(S)
    x = x_T
    traj = []
    with torch.no_grad():
        for t in steps:
            y = RR.prediction(params, hp, sampler, x, spec_c, t, step_weight(t, w, interval), table)
            if plan is not None:
                y = RR.shared_mean(y, plan)
            noisy = family in (0, 2, 4) and t > 0
            x = RR.update(family, t, rows[t][family], x, y, noise[t] if noisy else None)
            traj.append(x)
    return torch.stack(traj, 0) if trajectory else x
