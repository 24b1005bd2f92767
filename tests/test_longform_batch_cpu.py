"""Several recordings in one long-form chain, without a GPU: the batch geometry (longform.plan_batch, gather_batch /
stitch_batch), the packing of files into chains and their dealing to ranks, the CLI's task.recordings_per_chain and the
public option "window_break"."""
import math
import os
import re

import pytest
import torch

from diffroll_amd import cli, longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 512
W = 640 * HOP
LONG = ["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null"]


def test_plan_batch_gather_and_stitch():
    lengths = [W + 1, W - 1000, 1400 * HOP - 100]            # 2, 1 and 3 windows at O = 160
    batch = longform.plan_batch(lengths, HOP, overlap=160)
    assert [p.n for p in batch.plans] == [2, 1, 3]
    assert batch.first == [0, 2, 3] and batch.marks == [2, 3] and batch.n == 6
    assert [p.T_out for p in batch.plans] == [math.ceil(L / HOP) for L in lengths]
    assert batch.plans == [longform.plan_windows(L, HOP, overlap=160) for L in lengths]
    g = torch.Generator().manual_seed(0)
    canvases = [torch.randn(p.T_c, 88, generator=g) for p in batch.plans]
    win = longform.gather_batch(canvases, batch)
    assert win.shape == (6, 640, 88) and win.is_contiguous()
    for r, (f, p) in enumerate(zip(batch.first, batch.plans)):
        assert torch.equal(win[f:f + p.n], longform.gather_windows(canvases[r], p))
    rolls = longform.stitch_batch(win, batch)
    assert len(rolls) == 3
    for roll, c, p in zip(rolls, canvases, batch.plans):
        assert roll.shape == (p.T_out, 88) and torch.equal(roll, c[:p.T_out])
    # leading dimensions (the injected-noise rows) ride along
    z = [torch.randn(4, p.T_c, 88, generator=g) for p in batch.plans]
    zw = longform.gather_batch(z, batch)
    assert zw.shape == (4, 6, 640, 88)
    for roll, c, p in zip(longform.stitch_batch(zw, batch), z, batch.plans):
        assert torch.equal(roll, c[:, :p.T_out])
    # frame counts instead of samples (generation); one recording = plan_windows
    b1 = longform.plan_batch([1500], None, overlap=160)
    assert b1.marks == [] and b1.first == [0] and b1.n == 3
    with pytest.raises(ValueError):
        longform.plan_batch([], HOP)
    with pytest.raises(ValueError):
        longform.gather_batch(canvases[:2], batch)
    with pytest.raises(ValueError):
        longform.stitch_batch(win[:5], batch)


def test_pack_chains():
    counts = [2, 1, 3, 1, 1, 4, 1]
    chains = longform.pack_chains(counts, 3)
    assert chains == [[0, 1, 2], [3, 4, 5], [6]]                       # the max_recordings cap
    assert longform.pack_chains(counts, 1) == [[i] for i in range(7)]
    # closed early when the next recording would take the chain past max_windows
    assert longform.pack_chains(counts, 8, max_windows=6) == [[0, 1, 2], [3, 4, 5], [6]]
    assert longform.pack_chains(counts, 8, max_windows=4) == [[0, 1], [2, 3], [4], [5], [6]]
    assert longform.pack_chains([200, 56, 1], 8) == [[0, 1], [2]]      # the default bound: MAX_WINDOWS = 256
    assert longform.pack_chains([longform.MAX_WINDOWS], 2) == [[0]]
    with pytest.raises(ValueError, match="MAX_WINDOWS"):
        longform.pack_chains([1, longform.MAX_WINDOWS + 1], 4)
    with pytest.raises(ValueError):
        longform.pack_chains([5], 4, max_windows=4)
    with pytest.raises(ValueError):
        longform.pack_chains(counts, 0)
    # every file in exactly one chain, in order, whatever the bounds
    for cap in (1, 2, 3, 7, 100):
        for mw in (4, 5, 9, 256):
            ch = longform.pack_chains(counts, cap, max_windows=mw)
            assert sum(ch, []) == list(range(len(counts)))
            assert all(1 <= len(c) <= cap and sum(counts[i] for i in c) <= mw for c in ch)
    assert longform.pack_chains([], 3) == []


def test_chains_are_dealt_whole_to_ranks():
    chains = longform.pack_chains([1] * 11, 3)
    shares = [longform.deal_chains(chains, r, 3) for r in range(3)]
    assert shares == [[[0, 1, 2], [9, 10]], [[3, 4, 5]], [[6, 7, 8]]]
    assert sorted(sum(shares, [])) == chains                            # a partition of the chains
    assert longform.deal_chains(chains, 0, 1) == chains
    with pytest.raises(ValueError):
        longform.deal_chains(chains, 3, 3)


def test_build_config_recordings_per_chain():
    assert "recordings_per_chain" not in cli.build_config(LONG)["task"]  # the default path is untouched
    cfg = cli.build_config(LONG + ["task.recordings_per_chain=3"])
    assert cfg["task"]["recordings_per_chain"] == 3 and cli.is_long_form(cfg)
    assert cli.build_config(LONG + ["task.recordings_per_chain=1"])["task"]["recordings_per_chain"] == 1
    for bad in ("0", "-1", "x", "2.5", "true"):
        with pytest.raises(SystemExit, match="recordings_per_chain"):
            cli.build_config(LONG + [f"task.recordings_per_chain={bad}"])
    # only meaningful for whole recordings
    with pytest.raises(SystemExit, match="recordings_per_chain"):
        cli.build_config(["task=transcription", "dataset=Custom", "task.recordings_per_chain=2"])
    with pytest.raises(SystemExit, match="recordings_per_chain"):
        cli.build_config(["task=generation", "task.recordings_per_chain=2"])


def test_window_break_is_a_documented_public_option():
    from diffroll_amd import _cabi
    assert "window_break" in _cabi.PUBLIC_OPTIONS
    hdr = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    block = re.search(r"/\*\s*\n \* Integer options.*?\*/\s*\nint dr_set_option", hdr, re.S)
    assert block and '"window_break"' in block.group(0)
    # next to "window_overlap", and the three values are stated
    text = block.group(0)
    assert text.index('"window_overlap"') < text.index('"window_break"') < text.index('"sampling_steps"')
    assert "clears all marks" in text and "DR_EINVAL" in text[text.index('"window_break"'):text.index('"sampling_steps"')]
