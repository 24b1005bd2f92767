// gfx950 (MI355X, CDNA4): option "cfg_momentum" - the momentum of adaptive projected guidance (Sadat et al. 2024), beside
// options "cfg_project" / "cfg_norm" (project.hip).  A guided step under the option runs, behind the head projections,
//   the statistics launch in its momentum form: per element d = y - c, m = d + (bf * m_prev) (m = d at the step that starts
//       the state), yb = c + m, formed on the fly from the head projections' L2-resident output and the state; the three
//       sums of project.hip over yb in place of y, in the same fixed order (include/diffroll_amd.h), and (a, b) by
//       project_coef into the group's record.  It reads the state and writes nothing but the records;
//   update_momentum_kernel, a further instantiation of update_quad: m recomputed and stored over m_prev by the element's
//       own thread, y' = (a c) + (b yb), the clamp, the update.
// The statistics have project.hip's two forms on project.hip's work buffer (a step runs one of the two):
//   momentum_roll_kernel   clips of at most THRESH_ROLL_MAX elements: one workgroup per roll, the blocks' sums in LDS;
//   momentum_grid_kernel   windows and longer clips: (blocks, rows) workgroups of one wave, a slot per workgroup and a
//                          ticket; the workgroup that draws the last one adds up every group's slots and leaves the ticket
//                          zero.
// No floating-point atomic, no workgroup waits for another, no dependence on the grid or on timing: a captured chain replays
// with no host help, and "the step starts the state" is a kernel argument baked per node.
#include "momentum_quad.h"

namespace dr {
#pragma clang fp contract(off)

constexpr int MM_ROLL_BLOCKS = (int)((THRESH_ROLL_MAX / 88 + PROJECT_BLOCK - 1) / PROJECT_BLOCK);      // blocks of the longest roll of the one-workgroup form

// One wave: lane l leaves the sums of frame f0 + l of `row` in fs (PROJECT_BLOCK x 3 doubles of LDS); behind a workgroup
// barrier lane 0 adds up the block's frames [f0, f1) in frame order.
DR_DEVINL void mm_frames(const MomentumArgs& a, const UpdateArgs& uc, const long row, const int f0, const int f1, double* fs) {
    const int lane = (int)(threadIdx.x & 63);
    if (f0 + lane < f1) {
        double s[3];
        momentum_frame(a.p.u, uc, a.m_prev, a.bf, row, f0 + lane, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) fs[lane * 3 + k] = s[k];
    }
}
DR_DEVINL void mm_block(const int frames, const double* fs, double (&b)[3]) {
#pragma clang fp contract(off)
    b[0] = b[1] = b[2] = 0.0;
    for (int j = 0; j < frames; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = b[k] + fs[j * 3 + k];
}
// (a, b) of a group into the record of its first row, at the step's weight as guided_quad reads it
DR_DEVINL void mm_record(const ProjectArgs& a, const long row, const double N, const double (&s)[3]) {
    float av, bv;
    project_coef(a.rho, a.norm, a.u.dyn ? a.u.dyn->w : a.u.w, N, s, av, bv);
    float* const rec = reinterpret_cast<float*>(a.work + PROJECT_HEAD) + row * PROJECT_ROW_WORDS;
    rec[0] = av; rec[1] = bv;
}

// ---------------------------------------------------------------------------------------------- one workgroup per roll
__global__ __launch_bounds__(256) void momentum_roll_kernel(const MomentumArgs a) {
#pragma clang fp contract(off)
    __shared__ double fs[4][PROJECT_BLOCK * 3];
    __shared__ double bs[MM_ROLL_BLOCKS][3];
    const long row = blockIdx.x;
    const int T = (int)(a.p.u.per_sample / 88), nb = (T + PROJECT_BLOCK - 1) / PROJECT_BLOCK;      // (nb <= MM_ROLL_BLOCKS: launcher)
    const int wave = (int)(threadIdx.x >> 6);
    UpdateArgs uc = a.p.u;
    uc.x0u = nullptr;
    for (int j0 = 0; j0 < nb; j0 += 4) {      // (uniform over the workgroup: four blocks per round, one per wave)
        const int j = j0 + wave;
        const int f0 = j * PROJECT_BLOCK, f1 = f0 + PROJECT_BLOCK < T ? f0 + PROJECT_BLOCK : T;
        mm_frames(a, uc, row, f0, f1, fs[wave]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && j < nb) {
            double b[3];
            mm_block(f1 - f0, fs[wave], b);
#pragma unroll
            for (int k = 0; k < 3; ++k) bs[j][k] = b[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < nb; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = s[k] + bs[j][k];
        mm_record(a.p, row, (double)a.p.u.per_sample, s);
    }
}

// ---------------------------------------------------------------------------------------------- one launch over all rows
DR_DEVINL double mm_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
DR_DEVINL void mm_store(double* p, const double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (blocks of PROJECT_BLOCK frames, rows), one wave each.  Block j of a row covers its counted frames
// [f_lo + j PROJECT_BLOCK, ..): a row that counts fewer frames than it has leaves its last slots unwritten and unread.
__global__ __launch_bounds__(64) void momentum_grid_kernel(const MomentumArgs a) {
#pragma clang fp contract(off)
    __shared__ double fs[PROJECT_BLOCK * 3];
    __shared__ unsigned last_s;
    const UpdateArgs& u = a.p.u;
    const long row = blockIdx.y, B = gridDim.y, nbmax = gridDim.x;
    const int T = (int)(u.per_sample / 88);
    double* const slots = reinterpret_cast<double*>(a.p.work + PROJECT_HEAD + B * PROJECT_ROW_WORDS);
    long first;
    int f_lo;
    thresh_place(u, row, first, f_lo);
    const int f0 = f_lo + (int)blockIdx.x * PROJECT_BLOCK, f1 = f0 + PROJECT_BLOCK < T ? f0 + PROJECT_BLOCK : T;
    UpdateArgs uc = u;
    uc.x0u = nullptr;
    mm_frames(a, uc, row, f0, f1, fs);
    __syncthreads();
    if (threadIdx.x == 0 && f0 < T) {
        double b[3];
        mm_block(f1 - f0, fs, b);
#pragma unroll
        for (int k = 0; k < 3; ++k) mm_store(slots + (row * nbmax + blockIdx.x) * 3 + k, b[k]);
    }
    // this workgroup's slot is written -> ticket; the last arriver sees every workgroup's
    __threadfence();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(a.p.work, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = ticket == gridDim.x * gridDim.y - 1u;
    }
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    for (long g = threadIdx.x; g < B; g += 64) {      // one lane per group
        long gf;
        int gl;
        thresh_place(u, g, gf, gl);
        if (gf != g) continue;
        double s[3] = {0.0, 0.0, 0.0};
        long frames = 0;
        for (long r = g; r < B; ++r) {
            thresh_place(u, r, gf, gl);
            if (gf != g) break;
            const int nb = (T - gl + PROJECT_BLOCK - 1) / PROJECT_BLOCK;
            for (int j = 0; j < nb; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = s[k] + mm_load(slots + (r * nbmax + j) * 3 + k);
            frames += T - gl;
        }
        mm_record(a.p, g, (double)(frames * 88), s);
    }
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(a.p.work, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_momentum(const MomentumArgs& a, int B, hipStream_t s) {
    const UpdateArgs& u = a.p.u;
    if (!u.x0c || !a.p.work || B < 1 || u.per_sample < 88 || u.per_sample % 88 || u.n != (long)B * u.per_sample ||
        u.n >= (1l << 31) || a.p.rho < 0 || a.p.rho > 10000 || a.p.norm < 0 || a.p.norm > 100000 || (a.p.rho == 0 && a.p.norm == 0) ||
        !(a.bf > -1.f && a.bf < 1.f) || a.bf == 0.f)
        return hipErrorInvalidValue;
    if (win_H(u) == 0 && u.per_sample <= THRESH_ROLL_MAX) {
        hipLaunchKernelGGL(momentum_roll_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(momentum_grid_kernel, dim3((unsigned)project_blocks((int)(u.per_sample / 88)), (unsigned)B), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the update
// The update of update_kernel (update.hip) on y' = (a c) + (b yb): the state is read, advanced and stored by the quad's thread.
__global__ __launch_bounds__(256) void update_momentum_kernel(const UpdateArgs a, const MomentumUpd mo) {
    const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
    if (i4 * 4 >= a.n) return;
    float4 y;
    reinterpret_cast<float4*>(a.x)[i4] = update_quad<false, false, false, true>(a, i4, &y, nullptr, nullptr, nullptr, &mo);
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
