// Option "x0_threshold" (include/diffroll_amd.h), the per-quad pieces: the prediction the selection ranks, the group a row
// belongs to, and the thresholding the update applies - shared by threshold.hip and update_thresh_kernel (update.hip).
#pragma once
#include "update_quad.h"

namespace dr {

// Option "x0_threshold": the prediction y in front of the clamp - guided, after the shared-frame mean or blend - for a kernel that
// needs y without the update (threshold.hip ranks |y - m|).  It RESTATES the first part of update_quad, which keeps its own
// text: the tail kernel's register budget moves with the shape of that code (profiles/start_kernel_resources.txt).  The
// same guided_quad, the same blend_quad with the lower window's value first, contraction off: the same bits, held to by
// tests/test_gpu_x0_threshold.py and tests/test_gpu_window_blend.py.
DR_DEVINL void pred_quad(const UpdateArgs& a, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    const float gw = a.dyn ? a.dyn->w : a.w, g1pw = a.dyn ? a.dyn->onepw : a.onepw;
    guided_quad(a, i4, gw, g1pw, y);
    if (win_H(a) > 0) {
        const long e0 = i4 * 4;
        const long smp = e0 / a.per_sample;
        const int f = (int)((e0 - smp * a.per_sample) / 88);
        const long o4 = a.per_sample / 4 - (long)win_H(a) * 22;
        bool has_up = (smp + 1) * a.per_sample < a.n, has_lo = smp > 0;
        if (a.win_tab) {
            has_lo = window_idx(a.win_tab[smp]) > 0;
            has_up = has_up && window_idx(a.win_tab[smp + 1]) > 0;
        }
        long p4 = -1;
        bool upper = false;
        if (f >= win_H(a) && has_up) { p4 = i4 + o4; upper = true; }
        else if (f < (int)(o4 / 22) && has_lo) p4 = i4 - o4;
        if (p4 >= 0) {
            float yp[4];
            guided_quad(a, p4, gw, g1pw, yp);
            if (upper) blend_quad(win_blend(a), f - win_H(a), (int)(o4 / 22), y, yp, y);
            else blend_quad(win_blend(a), f, (int)(o4 / 22), yp, y, y);
        }
    }
}
// The group of row smp (kernels.h: ThreshArgs): its first row - where the group's {q, s} live - and the first frame of the
// row that counts (a window that is not its recording's first has its frames [0, O) counted by its predecessor).
DR_DEVINL void thresh_place(const UpdateArgs& a, const long smp, long& first, int& f_lo) {
    first = smp; f_lo = 0;
    if (win_H(a) > 0) {
        const long idx = a.win_tab ? window_idx(a.win_tab[smp]) : smp;
        first = smp - idx;
        f_lo = idx > 0 ? (int)(a.per_sample / 88) - win_H(a) : 0;
    }
}
// ... and what the update does with s of its quad's group: with u = y - m, y' = m + (clamp(u, -s, s) r) / s where s > r, else
// the static clamp itself - a step whose quantile does not exceed r is bit-identical to the "x0_clip" step.  One rounding
// per operation; compare-and-select as in clamp_quad (a NaN stays a NaN).
DR_DEVINL void form_quad(const UpdateArgs& a, const ThreshUpd& th, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    long first;
    int f_lo;
    thresh_place(a, i4 * 4 / a.per_sample, first, f_lo);
    const float s = th.qs[first * THRESH_ROW_WORDS + 1], ns = -s;
    if (s > th.r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = y[e] - th.m;
            const float c = u < ns ? ns : (u > s ? s : u);
            y[e] = th.m + (c * th.r) / s;
        }
    } else clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

}  // namespace dr
