// gfx950 (MI355X, CDNA4): options "cfg_project" / "cfg_norm" - the statistics behind adaptive projected guidance (Sadat et al.
// 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models"), without its momentum.
// Per GROUP (kernels.h: ProjectArgs - a clip's roll, or a recording's canvas) the launch here leaves
//   a = (float)((1 - s) - s (rho k)),  b = (float)s,   k = Scd / Scc,  s = min(1, r / (sqrt(Sdd / N) / |w|))
// in the group's record, the sums over the conditional prediction c and d = y - c of the guided prediction y, both after the
// shared-frame mean / blend, in double and in ONE fixed order (include/diffroll_amd.h states it; it is "cfg_rescale"'s):
//   a frame's 88 elements in pitch order;
//   the frames a row counts in blocks of PROJECT_BLOCK from its first counted frame, a block's frames in frame order;
//   a group's blocks in row, then block order;
// every level a sequential sum from 0.  A lane owns a frame, a wave a block: the block's frame sums meet in LDS and lane 0
// adds them up in frame order.  A function of the inputs alone - no floating-point atomic, no dependence on the grid or on
// timing.  y and c are recomputed by pred_quad from the head projections' L2-resident output; nothing but sums is stored.
//
// Two forms, chosen by the launcher:
//   project_roll_kernel   clips of at most THRESH_ROLL_MAX elements: one workgroup per roll, the blocks' sums in LDS, no
//                         work word touched but the result;
//   project_grid_kernel   windows and longer clips: (blocks, rows) workgroups of one wave.  A workgroup parks its block's
//                         sums in its slot and draws a ticket; the workgroup that draws the last one adds up every group's
//                         slots and leaves the ticket zero (every slot that is read was written by this launch, so the
//                         slots need no re-arming).
// No workgroup ever waits for another, so neither form assumes anything about what else is resident; a captured chain
// replays with no host help.
#include "project_quad.h"

namespace dr {
#pragma clang fp contract(off)

constexpr int PJ_ROLL_BLOCKS = (int)((THRESH_ROLL_MAX / 88 + PROJECT_BLOCK - 1) / PROJECT_BLOCK);      // blocks of the longest roll of the one-workgroup form

// One wave, two steps with a workgroup barrier between them: lane l leaves the sums of frame f0 + l of `row` in fs (the
// wave's PROJECT_BLOCK x 3 doubles of LDS); then lane 0 adds up the block's frames [f0, f1) in frame order.
DR_DEVINL void pj_frames(const UpdateArgs& u, const UpdateArgs& uc, const long row, const int f0, const int f1, double* fs) {
    const int lane = (int)(threadIdx.x & 63);
    if (f0 + lane < f1) {
        double s[3];
        project_frame(u, uc, row, f0 + lane, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) fs[lane * 3 + k] = s[k];
    }
}
DR_DEVINL void pj_block(const int frames, const double* fs, double (&b)[3]) {
#pragma clang fp contract(off)
    b[0] = b[1] = b[2] = 0.0;
    for (int j = 0; j < frames; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = b[k] + fs[j * 3 + k];
}
// the step's weight as guided_quad reads it
DR_DEVINL float pj_weight(const UpdateArgs& u) { return u.dyn ? u.dyn->w : u.w; }
DR_DEVINL void pj_record(const ProjectArgs& a, const long row, const double N, const double (&s)[3]) {
    float av, bv;
    project_coef(a.rho, a.norm, pj_weight(a.u), N, s, av, bv);
    float* const rec = reinterpret_cast<float*>(a.work + PROJECT_HEAD) + row * PROJECT_ROW_WORDS;
    rec[0] = av; rec[1] = bv;
}

// ---------------------------------------------------------------------------------------------- one workgroup per roll
__global__ __launch_bounds__(256) void project_roll_kernel(const ProjectArgs a) {
#pragma clang fp contract(off)
    __shared__ double fs[4][PROJECT_BLOCK * 3];
    __shared__ double bs[PJ_ROLL_BLOCKS][3];
    const long row = blockIdx.x;
    const int T = (int)(a.u.per_sample / 88), nb = (T + PROJECT_BLOCK - 1) / PROJECT_BLOCK;      // (nb <= PJ_ROLL_BLOCKS: launcher)
    const int wave = (int)(threadIdx.x >> 6);
    UpdateArgs uc = a.u;
    uc.x0u = nullptr;
    for (int j0 = 0; j0 < nb; j0 += 4) {      // (uniform over the workgroup: four blocks per round, one per wave)
        const int j = j0 + wave;
        const int f0 = j * PROJECT_BLOCK, f1 = f0 + PROJECT_BLOCK < T ? f0 + PROJECT_BLOCK : T;
        pj_frames(a.u, uc, row, f0, f1, fs[wave]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && j < nb) {
            double b[3];
            pj_block(f1 - f0, fs[wave], b);
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
        pj_record(a, row, (double)a.u.per_sample, s);
    }
}

// ---------------------------------------------------------------------------------------------- one launch over all rows
DR_DEVINL double pj_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
DR_DEVINL void pj_store(double* p, const double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (blocks of PROJECT_BLOCK frames, rows), one wave each.  Block j of a row covers its counted frames
// [f_lo + j PROJECT_BLOCK, ..): a row that counts fewer frames than it has leaves its last slots unwritten and unread.
__global__ __launch_bounds__(64) void project_grid_kernel(const ProjectArgs a) {
#pragma clang fp contract(off)
    __shared__ double fs[PROJECT_BLOCK * 3];
    __shared__ unsigned last_s;
    const long row = blockIdx.y, B = gridDim.y, nbmax = gridDim.x;
    const int T = (int)(a.u.per_sample / 88);
    double* const slots = reinterpret_cast<double*>(a.work + PROJECT_HEAD + B * PROJECT_ROW_WORDS);
    long first;
    int f_lo;
    thresh_place(a.u, row, first, f_lo);
    const int f0 = f_lo + (int)blockIdx.x * PROJECT_BLOCK, f1 = f0 + PROJECT_BLOCK < T ? f0 + PROJECT_BLOCK : T;
    UpdateArgs uc = a.u;
    uc.x0u = nullptr;
    pj_frames(a.u, uc, row, f0, f1, fs);
    __syncthreads();
    if (threadIdx.x == 0 && f0 < T) {
        double b[3];
        pj_block(f1 - f0, fs, b);
#pragma unroll
        for (int k = 0; k < 3; ++k) pj_store(slots + (row * nbmax + blockIdx.x) * 3 + k, b[k]);
    }
    // this workgroup's slot is written -> ticket; the last arriver sees every workgroup's
    __threadfence();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(a.work, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = ticket == gridDim.x * gridDim.y - 1u;
    }
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    for (long g = threadIdx.x; g < B; g += 64) {      // one lane per group
        long gf;
        int gl;
        thresh_place(a.u, g, gf, gl);
        if (gf != g) continue;
        double s[3] = {0.0, 0.0, 0.0};
        long frames = 0;
        for (long r = g; r < B; ++r) {
            thresh_place(a.u, r, gf, gl);
            if (gf != g) break;
            const int nb = (T - gl + PROJECT_BLOCK - 1) / PROJECT_BLOCK;
            for (int j = 0; j < nb; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = s[k] + pj_load(slots + (r * nbmax + j) * 3 + k);
            frames += T - gl;
        }
        pj_record(a, g, (double)(frames * 88), s);
    }
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(a.work, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_project(const ProjectArgs& a, int B, hipStream_t s) {
    const UpdateArgs& u = a.u;
    if (!u.x0c || !a.work || B < 1 || u.per_sample < 88 || u.per_sample % 88 || u.n != (long)B * u.per_sample ||
        u.n >= (1l << 31) || a.rho < 0 || a.rho > 10000 || a.norm < 0 || a.norm > 100000 || (a.rho == 0 && a.norm == 0))
        return hipErrorInvalidValue;
    if (win_H(u) == 0 && u.per_sample <= THRESH_ROLL_MAX) {
        hipLaunchKernelGGL(project_roll_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(project_grid_kernel, dim3((unsigned)project_blocks((int)(u.per_sample / 88)), (unsigned)B), dim3(64), 0, s, a);
    return hipGetLastError();
}

// (dr_debug_project) (a, b) of the groups' first rows, in row order
__global__ __launch_bounds__(256) void project_gather_kernel(const ProjectArgs a, int B, float* out) {
    for (long b = threadIdx.x; b < B; b += 256) {
        long first;
        int f_lo;
        thresh_place(a.u, b, first, f_lo);
        if (first != b) continue;
        long g = b;
        if (win_H(a.u) > 0) {
            g = 0;
            if (a.u.win_tab)
                for (long j = 0; j < b; ++j) g += window_idx(a.u.win_tab[j]) == 0;
        }
        const float* const rec = reinterpret_cast<const float*>(a.work + PROJECT_HEAD) + b * PROJECT_ROW_WORDS;
        out[g * 2] = rec[0];
        out[g * 2 + 1] = rec[1];
    }
}
hipError_t launch_project_gather(const ProjectArgs& a, int B, float* out, hipStream_t s) {
    if (!a.work || !out || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(project_gather_kernel, dim3(1), dim3(256), 0, s, a, B, out);
    return hipGetLastError();
}

}  // namespace dr
