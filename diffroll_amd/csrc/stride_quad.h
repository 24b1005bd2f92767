// Option "guidance_stride" (include/diffroll_amd.h), the per-quad piece: what the update's stride form applies between the
// shared-frame blend and the update - used by update_stride_kernel (stride.hip).  The conditional prediction behind the blend
// is threshold_quad.h's pred_quad with x0u null, as in momentum_quad.h.
#pragma once
#include "threshold_quad.h"

namespace dr {

// What the update's stride form needs beside UpdateArgs (its second kernel argument, in MomentumUpd's place)
struct StrideUpd {
    float* d;              // the state: written by a refresh step, read by a reuse step, by the element's own thread
    int reuse;             // 1: the step reuses (UpdateArgs::x0u is null: the y it is handed is c); 0: it refreshes
};

// A refresh step: y is the guided prediction, c the conditional one (pred_quad of uc = a with x0u null); d = y - c is stored
// over the state and y goes on unchanged - the roll the step leaves is the roll of the same step without the option.  A reuse
// step: the y it is handed is c (the step ran no unconditional evaluation), and y = c + d.  fp32, one rounding each.  Then the
// clamp of "x0_clip" where UpdateArgs names one.
DR_DEVINL void form_quad(const UpdateArgs& a, const StrideUpd& su, const long i4, float (&y)[4]) {
#pragma clang fp contract(off)
    if (su.reuse) {
        const float4 dv = reinterpret_cast<const float4*>(su.d)[i4];
        const float d[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = y[e] + d[e];
    } else {
        UpdateArgs uc = a;
        uc.x0u = nullptr;
        float c[4];
        pred_quad(uc, i4, c);
        reinterpret_cast<float4*>(su.d)[i4] = make_float4(y[0] - c[0], y[1] - c[1], y[2] - c[2], y[3] - c[3]);
    }
    if (a.clamp_lo < a.clamp_hi) clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

}  // namespace dr
