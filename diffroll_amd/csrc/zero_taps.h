// Which taps of a dilated conv read nothing but zero padding for a whole 32-frame MFMA tile (host and device, no HIP in it:
// tests/test_zero_taps_cpu.py compiles it alone and holds it to a scan of every frame index).
//
// A block contracts frames [t0, t0 + 32 NW) of a clip of T frames as NW tiles of 32 frames; tap j of `taps` (odd) reads the
// tile's frames shifted by (j - cen) * dil, cen = (taps - 1) / 2, and frames outside [0, T) are zero padding.  The products of
// such a tap with a tile whose whole shifted window is padding are w * (+0): the K loop may leave them out without changing a
// bit of the sum (a chain that starts from +0 never holds -0).
//   nlo   leading taps (j = 0 .. nlo - 1) whose window of tile 0 ends at or before frame 0:
//         (cen - j) * dil >= t0 + 32
//   nhi   trailing taps (j = taps - nhi .. taps - 1) whose window of tile NW - 1 starts at or after frame T:
//         (j - cen) * dil >= T - t0 - 32 (NW - 1); the centre tap is never counted, also where the tile holds no frame at all
// Counting fewer taps than possible is always correct, one too many is not: both counts are exact, never rounded up.
#pragma once

namespace dr {

struct EdgeTaps { int nlo, nhi; };

// (constexpr: callable from host and device code alike, without an attribute)
constexpr EdgeTaps edge_taps(const int T, const int t0, const int dil, const int taps, const int NW) {
    const int cen = (taps - 1) / 2;
    const int first = (t0 + 32 + dil - 1) / dil;                 // ceil((t0 + 32) / dil): t0 >= 0, dil >= 1
    const int rest = T - t0 - 32 * (NW - 1);                     // valid frames from the last tile's first on (may be <= 0)
    const int last = rest <= dil ? 1 : (rest + dil - 1) / dil;   // max(1, ceil(rest / dil))
    return EdgeTaps{cen - first + 1 > 0 ? cen - first + 1 : 0, cen - last + 1 > 0 ? cen - last + 1 : 0};
}

}  // namespace dr
