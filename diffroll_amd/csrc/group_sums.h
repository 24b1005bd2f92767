// gfx950 (MI355X, CDNA4): the statistics launch of options "cfg_rescale", "cfg_project" / "cfg_norm" and "cfg_momentum" -
// K sums per GROUP (kernels.h: a clip's roll, or a recording's canvas, every canvas frame counted once) over the conditional
// prediction c and the guided prediction y, both after the shared-frame mean / blend, in double and in ONE fixed order
// (include/diffroll_amd.h states it):
//   a frame's 88 elements in pitch order;
//   the frames a row counts in blocks of GS_BLOCK from its first counted frame, a block's frames in frame order;
//   a group's blocks in row, then block order;
// every level a sequential sum from 0.  A lane owns a frame, a wave a block: the block's frame sums meet in LDS and lane 0
// adds them up in frame order.  A function of the inputs alone - no floating-point atomic, no dependence on the grid or on
// timing: the same bits on every grid and on every replay.  y and c are recomputed by pred_quad from the head projections'
// L2-resident output; nothing but sums is stored.
//
// What an option brings is its statistic S (rescale.hip, project.hip, momentum.hip):
//   S::K                          the sums per frame
//   S::Args, S::u(a), S::work(a)  the kernel argument, its UpdateArgs and its work buffer (kernels.h has the layout)
//   S::frame(a, uc, row, f, s)    the K sums of frame f of `row`; uc = u(a) with x0u null, what pred_quad forms c from
//   S::record(a, row, N, s)       a group's sums over its N elements -> the record of the group's first row
// and two kernels of one line each, in the two forms the launcher chooses between:
//   gs_roll   clips of at most THRESH_ROLL_MAX elements: one workgroup per roll, the blocks' sums in LDS, no work word
//             touched but the result;
//   gs_grid   windows and longer clips: (blocks, rows) workgroups of one wave.  A workgroup parks its block's sums in its
//             slot and draws a ticket; the workgroup that draws the last one adds up every group's slots and leaves the
//             ticket zero (frame_counts_kernel's pattern; every slot that is read was written by this launch, so the slots
//             need no re-arming).
// No workgroup ever waits for another, so neither form assumes anything about what else is resident; a captured chain
// replays with no host help.
#pragma once
#include "threshold_quad.h"

namespace dr {
#pragma clang fp contract(off)

constexpr int GS_ROLL_BLOCKS = (int)((THRESH_ROLL_MAX / 88 + GS_BLOCK - 1) / GS_BLOCK);      // blocks of the longest roll of the one-workgroup form

// a slot's double, read and written as one 64-bit word at agent scope
DR_DEVINL double gs_load(const double* p) {
#pragma clang fp contract(off)
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
DR_DEVINL void gs_store(double* p, const double v) {
#pragma clang fp contract(off)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave, two steps with a workgroup barrier between them: lane l leaves the sums of frame f0 + l of `row` in fs (the
// wave's GS_BLOCK x K doubles of LDS); then lane 0 adds up the block's frames [f0, f1) in frame order.
template <class S>
DR_DEVINL void gs_frames(const typename S::Args& a, const UpdateArgs& uc, const long row, const int f0, const int f1, double* fs) {
#pragma clang fp contract(off)
    const int lane = (int)(threadIdx.x & 63);
    if (f0 + lane < f1) {
        double s[S::K];
        S::frame(a, uc, row, f0 + lane, s);
#pragma unroll
        for (int k = 0; k < S::K; ++k) fs[lane * S::K + k] = s[k];
    }
}
template <int K>
DR_DEVINL void gs_block(const int frames, const double* fs, double (&b)[K]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < K; ++k) b[k] = 0.0;
    for (int j = 0; j < frames; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) b[k] = b[k] + fs[j * K + k];
}

// ---------------------------------------------------------------------------------------------- one workgroup per roll
// (a kernel of 256 threads, grid (rows))
template <class S>
DR_DEVINL void gs_roll(const typename S::Args& a) {
#pragma clang fp contract(off)
    constexpr int K = S::K;
    __shared__ double fs[4][GS_BLOCK * K];
    __shared__ double bs[GS_ROLL_BLOCKS][K];
    const UpdateArgs& u = S::u(a);
    const long row = blockIdx.x;
    const int T = (int)(u.per_sample / 88), nb = (T + GS_BLOCK - 1) / GS_BLOCK;      // (nb <= GS_ROLL_BLOCKS: launcher)
    const int wave = (int)(threadIdx.x >> 6);
    UpdateArgs uc = u;
    uc.x0u = nullptr;
    for (int j0 = 0; j0 < nb; j0 += 4) {      // (uniform over the workgroup: four blocks per round, one per wave)
        const int j = j0 + wave;
        const int f0 = j * GS_BLOCK, f1 = f0 + GS_BLOCK < T ? f0 + GS_BLOCK : T;
        gs_frames<S>(a, uc, row, f0, f1, fs[wave]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && j < nb) {
            double b[K];
            gs_block(f1 - f0, fs[wave], b);
#pragma unroll
            for (int k = 0; k < K; ++k) bs[j][k] = b[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double s[K] = {};
        for (int j = 0; j < nb; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = s[k] + bs[j][k];
        S::record(a, row, (double)u.per_sample, s);
    }
}

// ---------------------------------------------------------------------------------------------- one launch over all rows
// (a kernel of 64 threads) grid (blocks of GS_BLOCK frames, rows), one wave each.  Block j of a row covers its counted frames
// [f_lo + j GS_BLOCK, ..): a row that counts fewer frames than it has leaves its last slots unwritten and unread.
template <class S>
DR_DEVINL void gs_grid(const typename S::Args& a) {
#pragma clang fp contract(off)
    constexpr int K = S::K;
    __shared__ double fs[GS_BLOCK * K];
    __shared__ unsigned last_s;
    const UpdateArgs& u = S::u(a);
    unsigned* const work = S::work(a);
    const long row = blockIdx.y, B = gridDim.y, nbmax = gridDim.x;
    const int T = (int)(u.per_sample / 88);
    double* const slots = reinterpret_cast<double*>(work + GS_HEAD + B * GS_ROW_WORDS);
    long first;
    int f_lo;
    thresh_place(u, row, first, f_lo);
    const int f0 = f_lo + (int)blockIdx.x * GS_BLOCK, f1 = f0 + GS_BLOCK < T ? f0 + GS_BLOCK : T;
    UpdateArgs uc = u;
    uc.x0u = nullptr;
    gs_frames<S>(a, uc, row, f0, f1, fs);
    __syncthreads();
    if (threadIdx.x == 0 && f0 < T) {
        double b[K];
        gs_block(f1 - f0, fs, b);
#pragma unroll
        for (int k = 0; k < K; ++k) gs_store(slots + (row * nbmax + blockIdx.x) * K + k, b[k]);
    }
    // this workgroup's slot is written -> ticket; the last arriver sees every workgroup's
    __threadfence();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(work, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
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
        double s[K] = {};
        long frames = 0;
        for (long r = g; r < B; ++r) {
            thresh_place(u, r, gf, gl);
            if (gf != g) break;
            const int nb = (T - gl + GS_BLOCK - 1) / GS_BLOCK;
            for (int j = 0; j < nb; ++j)
#pragma unroll
                for (int k = 0; k < K; ++k) s[k] = s[k] + gs_load(slots + (r * nbmax + j) * K + k);
            frames += T - gl;
        }
        S::record(a, g, (double)(frames * 88), s);
    }
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(work, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The launcher of a statistic's two kernels: what every statistic checks (its own ranges: its launch_*), then the form.
template <class S>
hipError_t gs_launch(void (*roll)(const typename S::Args), void (*grid)(const typename S::Args), const typename S::Args& a, int B, hipStream_t s) {
    const UpdateArgs& u = S::u(a);
    if (!u.x0c || !S::work(a) || B < 1 || u.per_sample < 88 || u.per_sample % 88 || u.n != (long)B * u.per_sample || u.n >= (1l << 31))
        return hipErrorInvalidValue;
    if (win_H(u) == 0 && u.per_sample <= THRESH_ROLL_MAX) {
        hipLaunchKernelGGL(roll, dim3((unsigned)B), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grid, dim3((unsigned)gs_blocks((int)(u.per_sample / 88)), (unsigned)B), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace dr
