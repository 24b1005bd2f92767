// Options "cfg_project" / "cfg_norm" (include/diffroll_amd.h), the per-quad pieces of adaptive projected guidance (Sadat et al.
// 2024): a frame's three sums, a group's coefficients (a, b) from its sums, and what the update applies - shared by
// project.hip and update_project_kernel (update.hip).
// Not here: APG's momentum - it needs a roll-sized state with validity rules like the solver history's and is option
// "cfg_momentum", momentum_quad.h - and the combined forms with "cfg_rescale" (which would need the spread of y') and
// "x0_threshold"; both combinations are refused.
#pragma once
#include "threshold_quad.h"

namespace dr {

// The sums of one frame: s = {Scc, Scd, Sdd} over the frame's 88 elements in pitch order, each a sequential sum in double
// from 0, d = (double)y - (double)c.  y is pred_quad's value, c pred_quad's of uc = the same arguments with x0u null.  Every
// difference, product and addition is rounded once (c c alone is exact in double).
// in_y(i4, c, y): what a quad's y is replaced by in front of the sums - nothing under these two options (PlainY); option
// "cfg_momentum" puts its yb there (momentum_quad.h: MomentumY).
struct PlainY {
    DR_DEVINL void operator()(const long, const float (&)[4], float (&)[4]) const {
#pragma clang fp contract(off)
    }
};
template <class InY>
DR_DEVINL void project_frame(const UpdateArgs& u, const UpdateArgs& uc, const long row, const int f, double (&s)[3], const InY& in_y) {
#pragma clang fp contract(off)
    s[0] = s[1] = s[2] = 0.0;
    const long q0 = row * (u.per_sample >> 2) + (long)f * 22;
    for (int q = 0; q < 22; ++q) {
        float y[4], c[4];
        pred_quad(u, q0 + q, y);
        pred_quad(uc, q0 + q, c);
        in_y(q0 + q, c, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double cd = (double)c[e], dd = (double)y[e] - cd;
            const double cc = cd * cd, cx = cd * dd, xx = dd * dd;
            s[0] = s[0] + cc; s[1] = s[1] + cx; s[2] = s[2] + xx;
        }
    }
}

// (a, b) of a group of N elements from its sums, at the step's weight w: k the share of c inside the update y - c, s the
// factor that bounds the rms of c - u = (y - c) / w by r.  (0.0f, 1.0f) exactly where either is not finite.
DR_DEVINL void project_coef(const int rho_i, const int norm_i, const float w, const double N, const double (&sum)[3], float& a, float& b) {
#pragma clang fp contract(off)
    double k = 0.0;
    if (sum[0] > 0.0) k = sum[1] / sum[0];
    const double rho = (double)rho_i / 10000.0;
    double s = 1.0;
    if (norm_i != 0) {
        const double r = (double)norm_i / 10000.0;
        const double ms = sum[2] / N;
        const double q = sqrt(ms) / fabs((double)w);
        if (q > r) s = r / q;
    }
    const double rk = rho * k;
    const double srk = s * rk;
    const double one_s = 1.0 - s;
    a = (float)(one_s - srk);
    b = (float)s;
    if (!(a - a == 0.f) || !(b - b == 0.f)) { a = 0.0f; b = 1.0f; }      // (inf - inf and NaN - NaN are NaN)
}
// ... into the record of the group's first row, at the step's weight as guided_quad reads it - with and without the momentum
DR_DEVINL void project_record(const ProjectArgs& a, const long row, const double N, const double (&s)[3]) {
#pragma clang fp contract(off)
    float av, bv;
    project_coef(a.rho, a.norm, a.u.dyn ? a.u.dyn->w : a.u.w, N, s, av, bv);
    float* const rec = reinterpret_cast<float*>(a.work + GS_HEAD) + row * GS_ROW_WORDS;
    rec[0] = av; rec[1] = bv;
}

// What update_kernel's projecting form does between the shared-frame blend and the update (update_quad.h): y' = (a c) + (b y)
// with (a, b) of the quad's group (the record of the group's first row: thresh_place) and c recomputed - y itself, bit for
// bit, where a == 0.0f and b == 1.0f - then the clamp of "x0_clip" where UpdateArgs names one.
DR_DEVINL void form_quad(const UpdateArgs& a, const ProjectUpd& pj, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    long first;
    int f_lo;
    thresh_place(a, i4 * 4 / a.per_sample, first, f_lo);
    const float av = pj.ab[first * GS_ROW_WORDS], bv = pj.ab[first * GS_ROW_WORDS + 1];
    if (!(av == 0.0f && bv == 1.0f)) {
        UpdateArgs uc = a;
        uc.x0u = nullptr;
        float c[4];
        pred_quad(uc, i4, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ac = av * c[e], by = bv * y[e];
            y[e] = ac + by;
        }
    }
    if (a.clamp_lo < a.clamp_hi) clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

}  // namespace dr
