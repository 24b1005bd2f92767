// gfx950 (MI355X, CDNA4): option "cfg_momentum" - the momentum of adaptive projected guidance (Sadat et al. 2024), beside
// options "cfg_project" / "cfg_norm" (project.hip).  A guided step under the option runs, behind the head projections,
//   the statistics launch in its momentum form: per element d = y - c, m = d + (bf * m_prev) (m = d at the step that starts
//       the state), yb = c + m, formed on the fly from the head projections' L2-resident output and the state; the three
//       sums of project.hip over yb in place of y, in the same fixed order (include/diffroll_amd.h), and (a, b) by
//       project_coef into the group's record.  It reads the state and writes nothing but the records;
//   update_momentum_kernel, a further instantiation of update_quad: m recomputed and stored over m_prev by the element's
//       own thread, y' = (a c) + (b yb), the clamp, the update.
// The statistics have project.hip's two forms (group_sums.h) on project.hip's work buffer (a step runs one of the two):
//   momentum_roll_kernel   clips of at most THRESH_ROLL_MAX elements: one workgroup per roll, the blocks' sums in LDS;
//   momentum_grid_kernel   windows and longer clips: (blocks, rows) workgroups of one wave, a slot per workgroup and a
//                          ticket; the workgroup that draws the last one adds up every group's slots and leaves the ticket
//                          zero.
// No floating-point atomic, no workgroup waits for another, no dependence on the grid or on timing: a captured chain replays
// with no host help, and "the step starts the state" is a kernel argument baked per node.
#include "momentum_quad.h"
#include "group_sums.h"

namespace dr {
#pragma clang fp contract(off)

// project.hip's statistic over yb: the frame's sums with MomentumY in front of them, (a, b) by project_coef into the same record
struct MomentumStat {
    static constexpr int K = PROJECT_SUMS;
    using Args = MomentumArgs;
    __host__ __device__ static inline const UpdateArgs& u(const Args& a) { return a.p.u; }
    __host__ __device__ static inline unsigned* work(const Args& a) { return a.p.work; }
    static DR_DEVINL void frame(const Args& a, const UpdateArgs& uc, const long row, const int f, double (&s)[K]) {
        project_frame(a.p.u, uc, row, f, s, MomentumY{a.m_prev, a.bf});
    }
    static DR_DEVINL void record(const Args& a, const long row, const double N, const double (&s)[K]) { project_record(a.p, row, N, s); }
};

__global__ __launch_bounds__(256) void momentum_roll_kernel(const MomentumArgs a) { gs_roll<MomentumStat>(a); }
__global__ __launch_bounds__(64) void momentum_grid_kernel(const MomentumArgs a) { gs_grid<MomentumStat>(a); }

hipError_t launch_momentum(const MomentumArgs& a, int B, hipStream_t s) {
    if (a.p.rho < 0 || a.p.rho > 10000 || a.p.norm < 0 || a.p.norm > 100000 || (a.p.rho == 0 && a.p.norm == 0) ||
        !(a.bf > -1.f && a.bf < 1.f) || a.bf == 0.f)
        return hipErrorInvalidValue;
    return gs_launch<MomentumStat>(momentum_roll_kernel, momentum_grid_kernel, a, B, s);
}

// ---------------------------------------------------------------------------------------------- the update
// The update of update_kernel (update.hip) on y' = (a c) + (b yb): the state is read, advanced and stored by the quad's thread.
__global__ __launch_bounds__(256) void update_momentum_kernel(const UpdateArgs a, const MomentumUpd mo) {
    const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
    if (i4 * 4 >= a.n) return;
    float4 y;
    reinterpret_cast<float4*>(a.x)[i4] = update_quad(a, i4, &y, mo);
    if (a.mode == 5 && hist_next(a)) reinterpret_cast<float4*>(hist_next(a))[i4] = y;
}

hipError_t launch_update_momentum(const UpdateArgs& a, const MomentumUpd& mo, hipStream_t s) {
    if (!mo.ab || !mo.m || !a.x0u || a.n % 4) return hipErrorInvalidValue;
    const long n4 = a.n / 4;
    hipLaunchKernelGGL(update_momentum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a, mo);
    return hipGetLastError();
}

// (dr_debug_momentum) the state a step would leave, by the update's own device function, into a buffer of the caller's
__global__ __launch_bounds__(256) void momentum_state_kernel(const UpdateArgs a, const float* m_prev, const float bf, float* m_next) {
    const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
    if (i4 * 4 >= a.n) return;
    UpdateArgs uc = a;
    uc.x0u = nullptr;
    float y[4], c[4], m[4], yb[4];
    pred_quad(a, i4, y);
    pred_quad(uc, i4, c);
    momentum_quad(y, c, m_prev, bf, i4, m, yb);
    reinterpret_cast<float4*>(m_next)[i4] = make_float4(m[0], m[1], m[2], m[3]);
}

hipError_t launch_momentum_state(const UpdateArgs& a, const float* m_prev, float bf, float* m_next, hipStream_t s) {
    if (!a.x0c || !m_next || a.n < 4 || a.n % 4) return hipErrorInvalidValue;
    const long n4 = a.n / 4;
    hipLaunchKernelGGL(momentum_state_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a, m_prev, bf, m_next);
    return hipGetLastError();
}

}  // namespace dr
