"""Long-form transcription: a recording of any length as jointly sampled 640-frame windows (pure functions, no GPU).

Definitions (include/diffroll_amd.h, option "window_overlap"):
  * window T frames (640: the shipping geometry, sampling.py:27), hop `hop` samples, W = T * hop samples per window;
    overlap O frames with 1 <= O <= T / 2, stride H = T - O.
  * a recording of L samples has T_out = ceil(L / hop) output frames, covered by n = 1 + max(0, ceil((T_out - T) / H))
    windows on a canvas of T_c = (n - 1) * H + T frames.
  * window b's audio is recording[b * H * hop : b * H * hop + W], zero-padded past the end (audio.crop_or_pad); its
    spectrogram, normalisation and conditioner are those of dr_frontend for that clip.
  * joint step: on a frame shared by windows b and b + 1 (frames [H, T) of b = frames [0, O) of b + 1) both windows use
    0.5f * (y_b + y_b+1), the mean of their guided x0 predictions, before the posterior update; noise is drawn per
    canvas frame.  Option "window_blend" (check_window_blend below) replaces the mean by a linear cross-fade over the
    overlap or by a hand-over at its middle; both windows still take the same value.  If x_T agrees on shared frames, every x_t does, bit for bit, so the stitched roll is a plain gather
    from the canvas (stitch), sliced to T_out.
  * several recordings in one chain (option "window_break", plan_batch): the windows of the recordings one after another;
    a window shares frames only with windows of its own recording, and recording r of the batch draws the noise of
    first_sample + r on its own canvas - each recording's roll is what a chain of its own would give.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, TypeVar

import torch

WINDOW_FRAMES = 640
DEFAULT_OVERLAP = 160
# windows one chain can hold: the engine's fused launches keep counters for 512 evaluations (launch_plan.h STACK_GROUPS),
# i.e. 256 guided windows (about 65 minutes of audio at the default overlap)
MAX_WINDOWS = 256
# option "window_blend": what a frame shared by windows b and b + 1 takes of their two guided predictions
WINDOW_BLENDS = {"mean": 0, "linear": 1, "nearest": 2}


def check_window_blend(blend) -> int:
    """blend= of sample_long / sample_long_batch and the CLI's task.window_blend -> the value of option "window_blend":
    None or "mean" = 0, the mean of the two predictions; "linear" = 1, the cross-fade y_lo + wu (y_up - y_lo) with
    wu = (j + 1) / (O + 1) at position j of the overlap; "nearest" = 2, the hand-over at the middle of the overlap - every
    canvas frame from the window whose centre is nearer.  The integers 0 / 1 / 2 themselves pass.  Anything else: ValueError."""
    if blend is None:
        return 0
    if isinstance(blend, str) and blend in WINDOW_BLENDS:
        return WINDOW_BLENDS[blend]
    if isinstance(blend, int) and not isinstance(blend, bool) and blend in (0, 1, 2):
        return blend
    raise ValueError(f"window blend is None, 'mean', 'linear', 'nearest' or 0 / 1 / 2, got {blend!r}")


@dataclass(frozen=True)
class WindowPlan:
    n: int                   # windows
    offsets: List[int]       # first canvas frame of each window (b * H)
    T: int                   # frames per window
    overlap: int             # O
    stride: int              # H = T - O
    T_c: int                 # canvas frames, (n - 1) * H + T
    T_out: int               # output frames of the recording, ceil(L / hop) (or the requested frame count)


def plan_windows(L_or_frames: int, hop: Optional[int], T: int = WINDOW_FRAMES, overlap: int = DEFAULT_OVERLAP) -> WindowPlan:
    """Window geometry of a recording of L samples (hop given: T_out = ceil(L / hop)) or of T_out frames (hop None)."""
    T = int(T)
    overlap = int(overlap)
    if T < 2:
        raise ValueError(f"window of {T} frames: need at least 2")
    if not 1 <= overlap <= T // 2:
        raise ValueError(f"overlap {overlap} out of range: 1 <= overlap <= T / 2 = {T // 2} (at most two windows share a frame)")
    L = int(L_or_frames)
    if L < 1:
        raise ValueError(f"empty recording ({L} {'samples' if hop else 'frames'})")
    T_out = L if hop is None else -(-L // int(hop))
    H = T - overlap
    n = 1 + max(0, -(-(T_out - T) // H))
    return WindowPlan(n=n, offsets=[b * H for b in range(n)], T=T, overlap=overlap, stride=H, T_c=(n - 1) * H + T, T_out=T_out)


def window_audio(recording: torch.Tensor, plan: WindowPlan, hop: int) -> torch.Tensor:
    """(L,) recording -> (n, W) window clips, W = T * hop: recording[off * hop : off * hop + W], zero-padded at the end."""
    from .audio import crop_or_pad
    if recording.dim() != 1:
        raise ValueError(f"recording must be 1-D (L,), got {tuple(recording.shape)}")
    W = plan.T * int(hop)
    return torch.stack([crop_or_pad(recording[o * int(hop):], W) for o in plan.offsets])


def gather_windows(canvas: torch.Tensor, plan: WindowPlan) -> torch.Tensor:
    """Canvas tensor (..., T_c, 88) -> windows (..., n, T, 88), window b = canvas frames [b * H, b * H + T) (a copy)."""
    if canvas.shape[-2] != plan.T_c:
        raise ValueError(f"canvas has {canvas.shape[-2]} frames, the plan {plan.T_c}")
    return torch.stack([canvas[..., o:o + plan.T, :] for o in plan.offsets], dim=-3).contiguous()


def stitch(windows: torch.Tensor, plan: WindowPlan) -> torch.Tensor:
    """Windows (..., n, T, 88) -> the recording's roll (..., T_out, 88): each canvas frame from the first window that
    holds it (shared frames are bitwise equal in both: the joint chain's invariant), sliced to T_out."""
    if windows.shape[-3] != plan.n or windows.shape[-2] != plan.T:
        raise ValueError(f"windows {tuple(windows.shape)} do not match the plan (n={plan.n}, T={plan.T})")
    parts = [windows[..., 0, :, :]] + [windows[..., b, plan.overlap:, :] for b in range(1, plan.n)]
    return torch.cat(parts, dim=-2)[..., :plan.T_out, :]


@dataclass(frozen=True)
class BatchPlan:
    """Several recordings in ONE chain (option "window_break"): recording r owns windows [first[r], first[r] + plans[r].n)
    of the batch; marks = the first window of every recording but the first."""
    plans: List[WindowPlan]
    first: List[int]
    marks: List[int]
    n: int                   # windows in the batch


def plan_batch(lengths_or_frames: Sequence[int], hop: Optional[int], T: int = WINDOW_FRAMES,
               overlap: int = DEFAULT_OVERLAP) -> BatchPlan:
    """plan_windows of every recording (lengths in samples, or frame counts when hop is None) and where each sits in the
    window batch of one chain."""
    plans = [plan_windows(L, hop, T, overlap) for L in lengths_or_frames]
    if not plans:
        raise ValueError("no recordings")
    first, n = [], 0
    for p in plans:
        first.append(n)
        n += p.n
    return BatchPlan(plans=plans, first=first, marks=first[1:], n=n)


def gather_batch(canvases: Sequence[torch.Tensor], batch: BatchPlan) -> torch.Tensor:
    """Per-recording canvases (..., T_c_r, 88) -> the chain's window batch (..., n, T, 88): gather_windows per recording,
    recordings in order."""
    if len(canvases) != len(batch.plans):
        raise ValueError(f"{len(canvases)} canvases for {len(batch.plans)} recordings")
    return torch.cat([gather_windows(c, p) for c, p in zip(canvases, batch.plans)], dim=-3)


def stitch_batch(windows: torch.Tensor, batch: BatchPlan) -> List[torch.Tensor]:
    """The chain's window batch (..., n, T, 88) -> one roll (..., T_out_r, 88) per recording (stitch per recording)."""
    if windows.shape[-3] != batch.n:
        raise ValueError(f"{windows.shape[-3]} windows, the batch plan has {batch.n}")
    return [stitch(windows[..., f:f + p.n, :, :], p) for f, p in zip(batch.first, batch.plans)]


def pack_chains(window_counts: Sequence[int], max_recordings: int, max_windows: int = MAX_WINDOWS) -> List[List[int]]:
    """Recordings (by their window counts, in file order) -> chains, greedily: a chain is a run of at most max_recordings
    consecutive recordings, closed early when the next one would take its windows past max_windows.  Returns the
    recording indices of each chain.  A single recording above max_windows cannot be placed: ValueError."""
    if max_recordings < 1:
        raise ValueError(f"max_recordings {max_recordings}: at least 1")
    chains: List[List[int]] = []
    total = 0
    for i, n in enumerate(window_counts):
        if n > max_windows:
            raise ValueError(f"recording {i}: {n} windows, one chain holds at most {max_windows} (longform.MAX_WINDOWS); "
                             f"split the recording")
        if not chains or len(chains[-1]) >= max_recordings or total + n > max_windows:
            chains.append([])
            total = 0
        chains[-1].append(i)
        total += n
    return chains


_T = TypeVar("_T")


def deal(items: Sequence[_T], rank: int, world: int) -> List[_T]:
    """Round-robin dealing of recordings to ranks: rank r takes items r, r + world, r + 2 world, ..."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    return list(items[rank::world])


def deal_chains(chains: Sequence[_T], rank: int, world: int) -> List[_T]:
    """Round-robin dealing of CHAINS (pack_chains) to ranks: the recordings of a chain stay together on one rank."""
    return deal(chains, rank, world)
