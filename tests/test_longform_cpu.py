"""Long-form transcription without a GPU: window geometry (diffroll_amd/longform.py), gather / stitch, round-robin dealing
of recordings to ranks, the CLI's max_segment_samples=null configuration and the public option "window_overlap"."""
import math
import os
import re

import numpy as np
import pytest
import torch

from diffroll_amd import cli, longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 512
W = 640 * HOP


def expect(L, O, hop=HOP, T=640):
    T_out = math.ceil(L / hop) if hop else L
    H = T - O
    n = 1 + max(0, math.ceil((T_out - T) / H))
    return n, [b * H for b in range(n)], (n - 1) * H + T, T_out


@pytest.mark.parametrize("O", [1, 160, 320])
@pytest.mark.parametrize("L", [W - 1000, W, W + 1, 5 * 60 * 16000])
def test_plan_windows_geometry(L, O):
    p = longform.plan_windows(L, HOP, overlap=O)
    n, offs, T_c, T_out = expect(L, O)
    assert (p.n, p.offsets, p.T_c, p.T_out, p.stride, p.overlap, p.T) == (n, offs, T_c, T_out, 640 - O, O, 640)
    # the windows cover every output frame, and the last one is needed
    assert p.offsets[-1] + p.T >= p.T_out
    assert p.n == 1 or p.offsets[-2] + p.T < p.T_out


def test_plan_windows_exact_values():
    # L < W, L = W: one window; L = W + 1: 641 frames, two windows
    assert longform.plan_windows(W - 1000, HOP).n == 1 and longform.plan_windows(W - 1000, HOP).T_out == 639
    p = longform.plan_windows(W, HOP)
    assert (p.n, p.offsets, p.T_c, p.T_out) == (1, [0], 640, 640)
    p = longform.plan_windows(W + 1, HOP, overlap=160)
    assert (p.n, p.offsets, p.T_c, p.T_out) == (2, [0, 480], 1120, 641)
    p = longform.plan_windows(W + 1, HOP, overlap=1)
    assert (p.n, p.offsets, p.T_c, p.T_out) == (2, [0, 639], 1279, 641)
    p = longform.plan_windows(W + 1, HOP, overlap=320)
    assert (p.n, p.offsets, p.T_c, p.T_out) == (2, [0, 320], 960, 641)
    # five minutes at 16 kHz: 9375 frames
    p = longform.plan_windows(5 * 60 * 16000, HOP, overlap=160)
    assert (p.n, p.T_c, p.T_out) == (20, 19 * 480 + 640, 9375) and p.offsets[-1] == 19 * 480
    p = longform.plan_windows(5 * 60 * 16000, HOP, overlap=1)
    assert (p.n, p.T_c, p.T_out) == (15, 14 * 639 + 640, 9375)
    p = longform.plan_windows(5 * 60 * 16000, HOP, overlap=320)
    assert (p.n, p.T_c, p.T_out) == (29, 28 * 320 + 640, 9375)
    # a frame count instead of samples (generation)
    p = longform.plan_windows(1500, None, overlap=160)
    assert (p.n, p.offsets, p.T_c, p.T_out) == (3, [0, 480, 960], 1600, 1500)


@pytest.mark.parametrize("O", [0, -1, 321, 640])
def test_plan_windows_rejects_overlap(O):
    with pytest.raises(ValueError, match="overlap"):
        longform.plan_windows(W * 3, HOP, overlap=O)


def test_window_audio_crops_and_pads():
    L = W + 5000
    rec = torch.arange(L, dtype=torch.float32)
    p = longform.plan_windows(L, HOP, overlap=160)
    clips = longform.window_audio(rec, p, HOP)
    assert clips.shape == (2, W)
    assert torch.equal(clips[0], rec[:W])
    start = 480 * HOP
    assert torch.equal(clips[1, :L - start], rec[start:])
    assert torch.count_nonzero(clips[1, L - start:]) == 0


def test_gather_and_stitch():
    p = longform.plan_windows(1500, None, overlap=160)
    canvas = torch.randn(1, p.T_c, 88)
    win = longform.gather_windows(canvas, p)
    assert win.shape == (1, 3, 640, 88) and win.is_contiguous()
    for b, o in enumerate(p.offsets):
        assert torch.equal(win[0, b], canvas[0, o:o + 640])
    # shared frames agree by construction: the stitch is the canvas, sliced to T_out
    assert torch.equal(longform.stitch(win, p), canvas[:, :1500])
    # the stitch takes each frame from the first window that holds it
    win2 = win.clone()
    win2[0, 1, :160] = -7.0        # the lower window's copy of frames [480, 640) wins
    assert torch.equal(longform.stitch(win2, p), canvas[:, :1500])
    # noise rows gather the same way: (S, T_c, 88) -> (S, n, T, 88)
    z = torch.randn(4, p.T_c, 88)
    zw = longform.gather_windows(z, p)
    assert zw.shape == (4, 3, 640, 88) and torch.equal(zw[2, 2], z[2, 960:1600])
    with pytest.raises(ValueError):
        longform.gather_windows(torch.randn(p.T_c + 1, 88), p)
    with pytest.raises(ValueError):
        longform.stitch(win[:, :2], p)


def test_round_robin_dealing():
    files = [f"f{i}" for i in range(7)]
    shares = [longform.deal(files, r, 3) for r in range(3)]
    assert shares == [["f0", "f3", "f6"], ["f1", "f4"], ["f2", "f5"]]
    assert sorted(sum(shares, [])) == sorted(files)
    assert longform.deal(files, 0, 1) == files
    assert longform.deal(files[:1], 2, 4) == []
    with pytest.raises(ValueError):
        longform.deal(files, 3, 3)


def test_build_config_long_form():
    cfg = cli.build_config(["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null"])
    assert cfg["dataset"]["args"]["max_segment_samples"] is None and cli.is_long_form(cfg)
    cfg = cli.build_config(["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null",
                            "task.window_overlap=320"])
    assert cfg["task"]["window_overlap"] == 320
    # an integer segment length is the clip path, as before
    cfg = cli.build_config(["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=32000"])
    assert not cli.is_long_form(cfg) and cfg["dataset"]["args"]["max_segment_samples"] == 32000
    assert not cli.is_long_form(cli.build_config(["task=transcription", "dataset=Custom"]))
    with pytest.raises(SystemExit, match="inpainting"):
        cli.build_config(["task=inpainting", "dataset=Custom", "dataset.args.max_segment_samples=null"])
    with pytest.raises(SystemExit, match="window_overlap"):
        cli.build_config(["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null",
                          "task.window_overlap=321"])


def test_ingest_whole_recording(tmp_path):
    from scipy.io import wavfile
    from diffroll_amd.audio import ingest
    x = (0.1 * np.random.default_rng(0).standard_normal(50000)).astype(np.float32)
    wavfile.write(str(tmp_path / "a.wav"), 16000, x)
    whole = ingest(str(tmp_path / "a.wav"), 16000, None)
    assert whole.shape == (50000,) and np.array_equal(whole.numpy(), x)
    assert ingest(str(tmp_path / "a.wav"), 16000, 20000).shape == (20000,)


def test_window_overlap_is_a_documented_public_option():
    from diffroll_amd import _cabi
    assert "window_overlap" in _cabi.PUBLIC_OPTIONS
    hdr = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    block = re.search(r"/\*\s*\n \* Integer options.*?\*/\s*\nint dr_set_option", hdr, re.S)
    assert block and '"window_overlap"' in block.group(0)
