"""Option "x0_clip" (include/diffroll_amd.h) restated on the CPU - test infrastructure: the chain loop of
chain_ref.sample_chain with one added line, the clamp of the prediction behind the shared-frame mean, composed from
chain_ref's chain_rows, prediction, shared_mean, update and solver_update.  Beside the roll it returns how much of the
prediction each bound moved at every step, so that a test can tell whether its inputs exercise the clamp at all."""
from typing import Optional

import torch

from oracle import diffroll_ref as R

import chain_ref as CR

BOUNDS = {0: None, 1: (0.0, 1.0), 2: (-1.0, 1.0)}      # the option's code -> [lo, hi]


def last_scale(hp) -> float:
    """c2 of step 0 (sqrt_acp[0], the committed fp32 value): a clipped final roll lies in [lo / c2, hi / c2]."""
    return float(CR.committed(hp)[0, 0, 2])


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, code: int = 0,
                 w: float = 0.0, plan=None, trajectory: bool = False, interval=None, order: int = 0, solver_noise: int = 0,
                 start: Optional[int] = None):
    """chain_ref.sample_chain's arguments and `code`, the option's value.  Returns (the final roll - or the trajectory -,
    {t: (share of y below lo, share above hi)} over the steps run; the shares are 0 under code 0)."""
    S = int(hp["timesteps"])
    family = CR.SAMPLERS[sampler][0]
    assert family <= 1 or not code, "an epsilon sampler has no x0 prediction to clamp"
    draws = solver_noise if order else family in (0, 2, 4)
    lo, hi = (0, S - 1) if interval is None else interval
    table = R.build_embedding(S)
    prev, traj, moved = None, [], {}
    with torch.no_grad():
        for t, row in CR.chain_rows(hp, sampler, n, order, solver_noise, start).items():
            y = CR.prediction(params, hp, sampler, x, spec_c, t, w if lo <= t <= hi else 0.0, table)
            if plan is not None:
                y = CR.shared_mean(y, plan)
            moved[t] = (0.0, 0.0)
            if code:
                b_lo, b_hi = BOUNDS[code]
                moved[t] = (float((y < b_lo).float().mean()), float((y > b_hi).float().mean()))
                y = y.clamp(b_lo, b_hi)                                   # THE added line
            z = noise[t] if draws and t > 0 else None
            x = CR.solver_update(t, row, x, y, prev, z) if order else CR.update(family, t, row, x, y, z)
            prev = y
            traj.append(x)
    return (torch.stack(traj, 0) if trajectory else x), moved
