"""Option "guidance_stride" (include/diffroll_amd.h) restated on the CPU - test infrastructure.  The refresh rule over the
steps that guide (refreshes / schedule), and chain_ref.sample_chain's loop with it: a refresh step stores d = y - c, a reuse step
consumes y = c + d, torch fp32, every operation its own rounding, the blend through blend_ref and the clamp through clip_ref.
Nothing of chain_ref or of the other restatements is edited.  Two variants exist for the record of why the form was chosen:
"skip" drops guidance at the reuse steps, "u" reuses a stale unconditional prediction instead of the stale difference."""
from typing import List, Optional

import torch

import blend_ref as BR
import chain_ref as CR
import clip_ref as CL
import thresh_ref as TR


def refreshes(n: int, k: int, t: int) -> bool:
    """Guided step t with ordinal k refreshes: every n-th one, and step 0 (n <= 1: off - every guided step)."""
    return n <= 1 or k % n == 0 or t == 0


def schedule(steps: List[int], n: int, S: int, interval=None, start: Optional[int] = None, guiding: bool = True, w: float = 1.0):
    """[(t, what)] over the visited steps `steps` (chain order) from `start` on: what = "refresh" / "reuse" for the steps that
    guide - a sampler that guides, w != 0, lo <= t <= hi - numbered in chain order, and "unguided" for the others."""
    lo, hi = (0, S - 1) if interval is None else interval
    steps = steps if start is None else steps[steps.index(start):]
    out, k = [], 0
    for t in steps:
        if not (guiding and w != 0.0 and lo <= t <= hi):
            out.append((t, "unguided"))
            continue
        out.append((t, "refresh" if refreshes(n, k, t) else "reuse"))
        k += 1
    return out


def evaluations(sched, B: int = 1) -> int:
    """Network evaluations of a chain with that schedule: 2 B at a refresh, B at every other step."""
    return sum(2 * B if what == "refresh" else B for _, what in sched)


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, guidance_stride: int = 0,
                 variant: str = "d", w: float = 0.0, code: int = 0, O: int = 0, mode: int = 0, marks=(), draws: int = 1, interval=None,
                 order: int = 0, solver_noise: int = 0, start: Optional[int] = None, trajectory: bool = False):
    """chain_ref.sample_chain's loop with the stride: at a step that refreshes y (weight w) and c (weight 0) are predicted, both
    blended over the shared frames (O > 0: a window batch as thresh_ref.window_groups reads it), d = y - c is stored and y goes
    on; at a step that reuses c alone is predicted and blended and y = c + d; then the clamp of code, then the update.
    guidance_stride 0 / 1: chain_ref.sample_chain, bit for bit.  variant "skip": a reuse step consumes c; "u": a refresh stores
    the unconditional prediction and a reuse step combines c with it at weight w (clips only).
    Returns (the final roll - or with trajectory=True the roll behind every step, (steps, B, 1, T, 88) - and [(t, what)])."""
    S = int(hp["timesteps"])
    family, branch = CR.SAMPLERS[sampler]
    B, T = x.shape[0], x.shape[-2]
    groups = TR.window_groups(B, O, marks, draws) if O else None
    noisy = solver_noise if order else family in (0, 2, 4)
    table = CR.R.build_embedding(S)
    rows = CR.chain_rows(hp, sampler, n, order, solver_noise, start)
    sched = dict(schedule(list(rows), guidance_stride, S, interval, None, branch is not None, w))
    blend = (lambda v: BR.blend_groups(v, groups, T - O, O, mode)) if O else (lambda v: v)
    prev, state, traj = None, None, []
    with torch.no_grad():
        for t, row in rows.items():
            what = sched[t]
            if what == "reuse":
                c = blend(CR.prediction(params, hp, sampler, x, spec_c, t, 0.0, table))
                if variant == "d":
                    y = c + state
                elif variant == "u":
                    y = (1 + w) * c - w * state
                else:
                    y = c
            else:
                y = blend(CR.prediction(params, hp, sampler, x, spec_c, t, w if what == "refresh" else 0.0, table))
                if what == "refresh" and guidance_stride > 1:
                    # (weight -1 is (1 - 1) c + u: the unconditional prediction itself)
                    state = y - blend(CR.prediction(params, hp, sampler, x, spec_c, t, 0.0, table)) if variant != "u" else \
                        blend(CR.prediction(params, hp, sampler, x, spec_c, t, -1.0, table))
            if code:
                y = y.clamp(*CL.BOUNDS[code])
            z = noise[t] if noisy and t > 0 else None
            x = CR.solver_update(t, row, x, y, prev, z) if order else CR.update(family, t, row, x, y, z)
            prev = y
            traj.append(x)
    return (torch.stack(traj, 0) if trajectory else x), list(sched.items())
