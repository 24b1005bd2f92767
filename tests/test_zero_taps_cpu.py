"""csrc/zero_taps.h without a GPU: edge_taps - how many leading / trailing taps of a dilated conv read nothing but zero padding
for the whole first / last 32-frame MFMA tile of a block - against a scan of every frame index of every tap's window.

The K loop of the fp32 128-frame conv blocks issues no MFMAs for the taps this function counts (option "zero_taps"), so one tap
too many is a wrong result and one too few only a lost saving: the test asserts that NO counted tap has a valid frame in its
window, for every geometry, and that the count is exact (every leading / trailing tap that could go is counted) wherever the
block exists (t0 < T).  A stand-alone program is compiled around the header, as tests/test_launch_variants_cpu.py does."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "zero_taps.h"
int main() {
    int T, t0, dil, taps, NW;
    while (std::scanf("%d %d %d %d %d", &T, &t0, &dil, &taps, &NW) == 5) {
        const dr::EdgeTaps e = dr::edge_taps(T, t0, dil, taps, NW);
        std::printf("%d %d\n", e.nlo, e.nhi);
    }
    return 0;
}
"""

TS = range(1, 301)
T0S = (0, 128)
DILS = (1, 2, 4, 8)
TAPS = (3, 9, 15)
NWS = (2, 4)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("zero_taps")
    src = d / "zero_taps_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "zero_taps_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = list(itertools.product(TS, T0S, DILS, TAPS, NWS))
    r = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    return {c: tuple(int(v) for v in ln.split()) for c, ln in zip(cases, out)}


def all_padding(T, first, shift):
    """The 32 frames first + shift .. first + shift + 31, every index looked at: none lies in [0, T)."""
    f = first + shift + np.arange(32)
    return not bool(((f >= 0) & (f < T)).any())


def test_edge_taps_never_counts_a_tap_with_a_valid_frame_and_counts_every_one_it_can(answers):
    assert len(answers) == 300 * 2 * 4 * 3 * 2
    counted = 0
    for (T, t0, dil, taps, NW), (nlo, nhi) in answers.items():
        cen = (taps - 1) // 2
        last = t0 + 32 * (NW - 1)
        assert 0 <= nlo <= cen and 0 <= nhi <= cen, (T, t0, dil, taps, NW, nlo, nhi)       # the centre tap is never counted
        for j in range(nlo):
            assert all_padding(T, t0, (j - cen) * dil), ("leading", T, t0, dil, taps, NW, j)
        for j in range(taps - nhi, taps):
            assert all_padding(T, last, (j - cen) * dil), ("trailing", T, t0, dil, taps, NW, j)
        counted += nlo + nhi
        if t0 < T:      # the block exists: the counts are exact
            lo = 0
            while lo < cen and all_padding(T, t0, (lo - cen) * dil):
                lo += 1
            hi = 0
            while hi < cen and all_padding(T, last, (cen - hi) * dil):
                hi += 1
            assert (nlo, nhi) == (lo, hi), (T, t0, dil, taps, NW, (nlo, nhi), (lo, hi))
    assert counted > 0


def test_edge_taps_at_the_geometries_the_kernel_meets(answers):
    # the bench geometry: one 128-frame block per 125-frame clip, k = 9; only the d = 8 layers have an edge tap
    assert [answers[(125, 0, d, 9, 4)] for d in DILS] == [(0, 0), (0, 0), (0, 0), (1, 1)]
    assert answers[(128, 0, 8, 9, 4)] == (1, 1)          # a full last tile: tap 8 reads [128, 160)
    assert answers[(97, 0, 8, 9, 4)] == (1, 4)           # ONE valid frame in tile 3 = [96, 128): tap 5 already reads [104, 136),
    assert answers[(104, 0, 8, 9, 4)] == (1, 4)          # ... past the clip as long as the tile holds at most 8 frames,
    assert answers[(105, 0, 8, 9, 4)] == (1, 3)          # ... and reaches frame 104 when it holds 9
    assert answers[(96, 0, 8, 9, 4)] == (1, 4) and answers[(60, 0, 8, 9, 4)] == (1, 4)      # empty last tile(s): all but the centre
    assert answers[(250, 0, 8, 9, 4)] == (1, 0)          # two frame tiles: the first has the leading edge alone,
    assert answers[(250, 128, 8, 9, 4)] == (0, 1)        # ... the second (frames 128 .. 249, tile 3 = [224, 256)) the trailing one
    assert answers[(125, 0, 8, 15, 4)] == (4, 4)         # k = 15 at d = 8: four taps per edge (the kernel clamps to one)
    assert answers[(125, 0, 8, 3, 4)] == (0, 0)          # k = 3: the outer taps sit at -+8 frames
