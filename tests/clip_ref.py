"""Option "x0_clip" (include/diffroll_amd.h) restated on the CPU - test infrastructure: the chain loop of
chain_ref.sample_chain with one hook, the clamp of the prediction behind the shared-frame mean.  Beside the roll it returns how much of the
prediction each bound moved at every step, so that a test can tell whether its inputs exercise the clamp at all."""
from typing import Optional

import torch

import chain_ref as CR

BOUNDS = {0: None, 1: (0.0, 1.0), 2: (-1.0, 1.0)}      # the option's code -> [lo, hi]


def last_scale(hp) -> float:
    """c2 of step 0 (sqrt_acp[0], the committed fp32 value): a clipped final roll lies in [lo / c2, hi / c2]."""
    return float(CR.committed(hp)[0, 0, 2])


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, code: int = 0, **kw):
    """chain_ref.sample_chain's arguments and `code`, the option's value.  Returns (the final roll - or the trajectory -,
    {t: (share of y below lo, share above hi)} over the steps run; the shares are 0 under code 0)."""
    assert CR.SAMPLERS[sampler][0] <= 1 or not code, "an epsilon sampler has no x0 prediction to clamp"
    moved = {}

    def clamp(t, y):
        moved[t] = (0.0, 0.0)
        if code:
            b_lo, b_hi = BOUNDS[code]
            moved[t] = (float((y < b_lo).float().mean()), float((y > b_hi).float().mean()))
            y = y.clamp(b_lo, b_hi)
        return y

    return CR.sample_chain(params, hp, sampler, x, spec_c, noise, n, hook=clamp, **kw), moved
