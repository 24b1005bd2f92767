// Option "cfg_momentum" (include/diffroll_amd.h), the per-quad pieces of the momentum of adaptive projected guidance (Sadat et
// al. 2024): the state's recurrence, a frame's three sums over yb = c + m, and what the update's momentum form applies -
// shared by the statistics launches and update_momentum_kernel (momentum.hip).  The coefficients and the groups are
// project_quad.h's (project_coef, thresh_place): one definition of (a, b) with and without the momentum.
#pragma once
#include "project_quad.h"

namespace dr {

// The recurrence of one float4: y the guided prediction and c the conditional one (pred_quad of u and of uc = u with x0u
// null), d = y - c, m = d where m_prev is null (the step starts the state), else m = d + (bf * m_prev[i4]); yb = c + m.  fp32,
// each operation rounded once.  A non-finite m_prev gives a non-finite m (bf is not 0): it stays so for the rest of the chain.
DR_DEVINL void momentum_quad(const float (&y)[4], const float (&c)[4], const float* m_prev, const float bf, const long i4,
                             float (&m)[4], float (&yb)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = y[e] - c[e];
    if (m_prev) {
        const float4 pv = reinterpret_cast<const float4*>(m_prev)[i4];
        const float p[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float bp = bf * p[e];
            m[e] = m[e] + bp;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) yb[e] = c[e] + m[e];
}

// project_frame over yb (project_quad.h: its in_y): s = {Scc, Scd, Sdd} of one frame with d = (double)yb - (double)c, the same
// order and roundings.
struct MomentumY {
    const float* m_prev;
    float bf;
    DR_DEVINL void operator()(const long i4, const float (&c)[4], float (&y)[4]) const {
#pragma clang fp contract(off)
        float m[4], yb[4];
        momentum_quad(y, c, m_prev, bf, i4, m, yb);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = yb[e];
    }
};

// What update_kernel's momentum form does between the shared-frame blend and the update (update_quad.h): m recomputed from
// the y it is handed and c, stored over m_prev by the element's own thread; y' = (a c) + (b yb) with (a, b) of the quad's
// group - yb itself, bit for bit, where a == 0.0f and b == 1.0f - then the clamp of "x0_clip" where UpdateArgs names one.
DR_DEVINL void form_quad(const UpdateArgs& a, const MomentumUpd& mo, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    UpdateArgs uc = a;
    uc.x0u = nullptr;
    float c[4], m[4], yb[4];
    pred_quad(uc, i4, c);
    momentum_quad(y, c, mo.start ? nullptr : mo.m, mo.bf, i4, m, yb);
    reinterpret_cast<float4*>(mo.m)[i4] = make_float4(m[0], m[1], m[2], m[3]);
    long first;
    int f_lo;
    thresh_place(a, i4 * 4 / a.per_sample, first, f_lo);
    const float av = mo.ab[first * GS_ROW_WORDS], bv = mo.ab[first * GS_ROW_WORDS + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = yb[e];
    if (!(av == 0.0f && bv == 1.0f)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ac = av * c[e], by = bv * yb[e];
            y[e] = ac + by;
        }
    }
    if (a.clamp_lo < a.clamp_hi) clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

}  // namespace dr
