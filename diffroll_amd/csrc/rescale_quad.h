// Option "cfg_rescale" (include/diffroll_amd.h), the per-quad pieces: the product the update and the threshold launches apply,
// and a frame's five sums - shared by rescale.hip, threshold.hip's rescaled forms and update_rescale_kernel (update.hip).
#pragma once
#include "threshold_quad.h"

namespace dr {

// y' = g y, g of the quad's group (the record of the group's first row: thresh_place): one fp32 product per element, the
// identity where g == 1.0f
DR_DEVINL void rescale_quad(const UpdateArgs& a, const float* g, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    long first;
    int f_lo;
    thresh_place(a, i4 * 4 / a.per_sample, first, f_lo);
    const float gv = g[first * GS_ROW_WORDS];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = gv * y[e];
}

// ... and what update_kernel's rescaling form does between the shared-frame blend and the update (update_quad.h): the
// product, then the thresholding of "x0_threshold" where rs.th is set, else the clamp of "x0_clip" where UpdateArgs names one
DR_DEVINL void form_quad(const UpdateArgs& a, const RescaleUpd& rs, const long i4, float (&y)[4]) {
    rescale_quad(a, rs.g, i4, y);
    if (rs.th.qs) form_quad(a, rs.th, i4, y);
    else if (a.clamp_lo < a.clamp_hi) clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

// The sums of one frame: s = {S1c, S2c, S1y, S2y} over the frame's 88 elements in pitch order, each a sequential sum in
// double from 0.  y is pred_quad's value, c pred_quad's of uc = the same arguments with x0u null.  (A square of an fp32
// value is exact in double: only the additions round, and fusing product and sum changes no bit.)
DR_DEVINL void rescale_frame(const UpdateArgs& u, const UpdateArgs& uc, const long row, const int f, double (&s)[4]) {
#pragma clang fp contract(off)
    s[0] = s[1] = s[2] = s[3] = 0.0;
    const long q0 = row * (u.per_sample >> 2) + (long)f * 22;
    for (int q = 0; q < 22; ++q) {
        float y[4], c[4];
        pred_quad(u, q0 + q, y);
        pred_quad(uc, q0 + q, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double cd = (double)c[e], yd = (double)y[e];
            s[0] = s[0] + cd; s[1] = s[1] + cd * cd;
            s[2] = s[2] + yd; s[3] = s[3] + yd * yd;
        }
    }
}

// g of a group of N elements from its sums; 1.0f exactly where the spread of y is not positive, that of c negative or not
// a number, or g not finite (constant rolls, inf / NaN inputs)
DR_DEVINL float rescale_factor(const int phi, const double N, const double (&s)[4]) {
#pragma clang fp contract(off)
    const double mc = s[0] / N, my = s[2] / N;
    const double pc = s[0] * mc, py = s[2] * my;
    const double Vc = s[1] - pc, Vy = s[3] - py;
    if (!(Vy > 0.0) || !(Vc >= 0.0)) return 1.0f;
    const double rho = sqrt(Vc / Vy);
    const double phid = (double)phi / 10000.0;
    const double d = phid * (rho - 1.0);
    const float g = (float)(1.0 + d);
    return (g - g == 0.f) ? g : 1.0f;      // (inf - inf and NaN - NaN are NaN)
}

}  // namespace dr
