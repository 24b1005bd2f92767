// gfx950 (MI355X, CDNA4): option "cfg_rescale" - the statistics behind the guidance rescale (Lin et al. 2024, section 3.4).
// Per GROUP (kernels.h: RescaleArgs - a clip's roll, or a recording's canvas) the launch here leaves
//   g = (float)(1 + phi (sqrt(Vc / Vy) - 1)),   V = S2 - S1 (S1 / N)
// in the group's record: the sums over the conditional prediction c and the guided prediction y, in the fixed order and by the
// two launch forms of group_sums.h.  Here: the statistic, its two kernels and launcher, and the debug entries' gather.
#include "rescale_quad.h"
#include "group_sums.h"

namespace dr {
#pragma clang fp contract(off)

struct RescaleStat {
    static constexpr int K = RESCALE_SUMS;
    using Args = RescaleArgs;
    __host__ __device__ static inline const UpdateArgs& u(const Args& a) { return a.u; }
    __host__ __device__ static inline unsigned* work(const Args& a) { return a.work; }
    static DR_DEVINL void frame(const Args& a, const UpdateArgs& uc, const long row, const int f, double (&s)[K]) {
        rescale_frame(a.u, uc, row, f, s);
    }
    static DR_DEVINL void record(const Args& a, const long row, const double N, const double (&s)[K]) {
        reinterpret_cast<float*>(a.work + GS_HEAD)[row * GS_ROW_WORDS] = rescale_factor(a.phi, N, s);
    }
};

__global__ __launch_bounds__(256) void rescale_roll_kernel(const RescaleArgs a) { gs_roll<RescaleStat>(a); }
__global__ __launch_bounds__(64) void rescale_grid_kernel(const RescaleArgs a) { gs_grid<RescaleStat>(a); }

hipError_t launch_rescale(const RescaleArgs& a, int B, hipStream_t s) {
    if (a.phi < 1 || a.phi > 10000) return hipErrorInvalidValue;
    return gs_launch<RescaleStat>(rescale_roll_kernel, rescale_grid_kernel, a, B, s);
}

// (dr_debug_rescale / dr_debug_project / dr_debug_momentum) the first `words` words of the records of the groups' first rows,
// in row order
__global__ __launch_bounds__(256) void group_gather_kernel(const UpdateArgs u, const float* rec, int words, int B, float* out) {
    for (long b = threadIdx.x; b < B; b += 256) {
        long first;
        int f_lo;
        thresh_place(u, b, first, f_lo);
        if (first != b) continue;
        long g = b;
        if (win_H(u) > 0) {
            g = 0;
            if (u.win_tab)
                for (long j = 0; j < b; ++j) g += window_idx(u.win_tab[j]) == 0;
        }
        for (int k = 0; k < words; ++k) out[g * words + k] = rec[b * GS_ROW_WORDS + k];
    }
}
hipError_t launch_group_gather(const UpdateArgs& u, const unsigned* work, int words, int B, float* out, hipStream_t s) {
    if (!work || !out || B < 1 || words < 1 || words > GS_ROW_WORDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_gather_kernel, dim3(1), dim3(256), 0, s, u, gs_records(work), words, B, out);
    return hipGetLastError();
}

}  // namespace dr
