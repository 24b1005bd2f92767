"""Several draws per clip (option "draws" of include/diffroll_amd.h, hparams.sampling.draws): the layout of a draw-major
batch, the Philox key of its rows, and what is made of the D rolls of a clip - their mean (the point estimate that is
scored and exported), the per-cell vote and the spread.  Plain torch on finished rolls: plumbing, not a hot path.

Draw-major: a batch of D draws of n clips holds D * n rolls, row b = draw b // n of clip b % n - the rolls of the batch
whose waveform is tiled D times, which is what the engine computes bit for bit from ONE set of conditioner tensors.
"""
from __future__ import annotations

from typing import Tuple

import torch


def check_draws(d) -> int:
    """hparams.sampling.draws / the draws= arguments: None = 1, else an integer >= 1.  Returns D; anything else raises
    ValueError."""
    if d is None:
        return 1
    if isinstance(d, bool) or not isinstance(d, int) or d < 1:
        raise ValueError(f"draws must be None / 1 (one roll per clip) or an integer >= 1, got {d!r}")
    return d


def draw_key(first_sample: int, b: int, n: int, stride: int = 0) -> int:
    """The Philox sample key of row b of a draw-major batch of n clips (option "draw_stride" = stride; 0 = n, and the key
    is first_sample + b): first_sample + b % n + (b // n) * stride."""
    return int(first_sample) + b % n + (b // n) * (int(stride) if stride else n)


def split_draws(rolls: torch.Tensor, draws: int) -> torch.Tensor:
    """Draw-major rolls (D * n, ...) -> (D, n, ...) (a view)."""
    D = check_draws(draws)
    if rolls.shape[0] % D:
        raise ValueError(f"{rolls.shape[0]} rolls are not a whole number of draws = {D}")
    return rolls.reshape((D, rolls.shape[0] // D) + tuple(rolls.shape[1:]))


def aggregate(rolls: torch.Tensor, draws: int, threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Draw-major rolls (D * n, 1, T, 88) -> (mean, votes, std), each (n, 1, T, 88) in fp32: the mean over the D draws of
    a clip, the fraction of its draws above the threshold, and the population standard deviation over the draws (0 for
    D = 1)."""
    x = split_draws(rolls, draws).to(torch.float32)
    mean = x.mean(0)
    votes = (x > float(threshold)).to(torch.float32).mean(0)
    std = (x - mean).pow(2).mean(0).sqrt()
    return mean, votes, std
