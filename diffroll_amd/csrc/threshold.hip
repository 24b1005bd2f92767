// gfx950 (MI355X, CDNA4): option "x0_threshold" - the exact order statistic behind dynamic thresholding (Saharia et al. 2022),
// the first reduction on the sampling path.  Per GROUP (kernels.h: ThreshArgs - a clip's roll, or a recording's canvas) the
// launches here select a[k] and a[k + 1] of the ascending |y - m| and leave
//   q = rem == 0 ? a[k] : a[k] + f (a[k + 1] - a[k]),   s = q > r ? q : r
// in the group's record, num = v (N - 1), k = num / 10000, rem = num % 10000, f = (float)((double)rem / 10000.0).
//
// Selection: radix selection over the 31-bit pattern of |y - m| (the bits of y - m with the sign cleared: as unsigned
// integers they order like the values, -0 == +0, inf above every finite value, NaN last), digits of 8, 8, 8 and 7 bits from
// the top.  A pass counts, per digit value, the elements that carry the bits selected so far; the bin that holds rank k is
// the next digit.  After four passes the pattern of a[k] is complete, and the last bin's count tells whether a[k + 1] is
// a[k] again (more than k + 1 elements are <= a[k]) - else a[k + 1] is the smallest pattern above a[k], one more pass.
// Exact, and a function of the inputs alone: every count is an integer (LDS / device integer atomics), no floating-point
// atomic, no dependence on the grid or on timing.  y is recomputed by pred_quad (threshold_quad.h) in every pass - the
// network's outputs are L2-resident behind the head projections - so nothing but the record is stored.
//
// Two forms, chosen by the launcher:
//   thresh_roll_kernel   clips of at most THRESH_ROLL_MAX elements: ONE launch, one workgroup per roll, all passes in LDS,
//                        no work word touched but the result;
//   thresh_pass_kernel   windows and longer clips: FIVE launches of (chunks, rows) workgroups.  A workgroup counts its
//                        chunk in LDS, adds its non-empty bins to the group's record with device atomics and draws a
//                        ticket; the workgroup that draws the last one reads every group's counts, picks the digit and
//                        leaves the counts and the ticket zero (frame_counts_kernel's pattern).  The hand-over from pass
//                        to pass is the launch boundary.
// No workgroup ever waits for another, so neither form assumes anything about what else is resident; the work words are
// re-armed by the kernels themselves, so a captured chain replays with no host help.
//
// Option "cfg_rescale": at a guided step under it the launches rank |g y - m|.  Each kernel has a rescaled form that takes
// the groups' g records as a second argument and puts rescale_quad behind pred_quad.  Both forms are ONE text, the second
// part of this file, which the first part includes once per form with
//   TH_ROLL_KERNEL / TH_PASS_KERNEL   the kernels' names
//   TH_PARAMS                         their parameters (the first is `const ThreshArgs a`)
//   TH_PRED(i4, y)                    the prediction the selection ranks
// Text and not a function template: the plain form compiles to what it compiled to before the option existed, register for
// register (profiles/rescale_kernel_resources.txt) - as a template inlined into two kernels thresh_pass_kernel did not.
#ifndef TH_ROLL_KERNEL      // ================================================================ part 1: the unit
#include "rescale_quad.h"

namespace dr {

constexpr int TH_CHUNK = 4096;      // quads a workgroup of the multi-launch form counts (16 per lane)

DR_DEVINL unsigned th_shift(const int p) { return p == 0 ? 23u : (p == 1 ? 15u : (p == 2 ? 7u : 0u)); }
DR_DEVINL unsigned th_pattern(const float y, const float m) {
#pragma clang fp contract(off)
    return __float_as_uint(y - m) & 0x7FFFFFFFu;
}
// pass p: does the pattern carry the bits selected so far (everything above the pass's digit)?
DR_DEVINL bool th_match(const int p, const unsigned pat, const unsigned prefix) {
    const unsigned hs = th_shift(p) + (p == 3 ? 7u : 8u);
    return p == 0 || (pat >> hs) == (prefix >> hs);
}
DR_DEVINL unsigned th_digit(const int p, const unsigned pat) { return p == 3 ? (pat & 0x7Fu) : ((pat >> th_shift(p)) & 0xFFu); }

// One wave: lane l holds the counts of bins 4 l .. 4 l + 3; rank `want` (< the sum of all bins) lies in bin `digit`, which
// has `eq` elements, `below` elements in the bins under it.  Returned in every lane.
DR_DEVINL void th_pick(const unsigned (&c)[4], const unsigned want, unsigned& digit, unsigned& below, unsigned& eq) {
    const int lane = (int)(threadIdx.x & 63);
    const unsigned mine = c[0] + c[1] + c[2] + c[3];
    unsigned inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    const unsigned exc = inc - mine;
    const unsigned long long hit = __ballot(exc <= want && want < inc);
    const int src = hit ? __builtin_ctzll(hit) : 63;
    unsigned d = (unsigned)lane * 4u, run = exc, e = c[0];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (want >= run + c[j] && d == (unsigned)lane * 4u + (unsigned)j) { run += c[j]; d += 1u; e = c[j + 1]; }
    digit = __shfl(d, src); below = __shfl(run, src); eq = __shfl(e, src);
}

// k and rem of a group of N elements
DR_DEVINL void th_rank(const int v, const unsigned N, unsigned& k, unsigned& rem) {
    const unsigned long long num = (unsigned long long)v * (unsigned long long)(N - 1u);
    k = (unsigned)(num / 10000ull); rem = (unsigned)(num % 10000ull);
}
DR_DEVINL void th_finish(const float m, const float r, const unsigned ak, const unsigned ak1, const unsigned rem, float* qs) {
#pragma clang fp contract(off)
    const float a0 = __uint_as_float(ak);
    float q = a0;
    if (rem != 0u) {
        const float f = (float)((double)rem / 10000.0);
        const float d = __uint_as_float(ak1) - a0;
        const float fd = f * d;
        q = a0 + fd;
    }
    qs[0] = q;
    qs[1] = q > r ? q : r;      // (a NaN q: s = r)
}

DR_DEVINL unsigned th_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DR_DEVINL void th_store(unsigned* p, const unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the plain forms: thresh_roll_kernel, thresh_pass_kernel rank |y - m|
#define TH_ROLL_KERNEL thresh_roll_kernel
#define TH_PASS_KERNEL thresh_pass_kernel
#define TH_PARAMS const ThreshArgs a
#define TH_PRED(i4, y) pred_quad(a.u, i4, y)
#include "threshold.hip"
#undef TH_ROLL_KERNEL
#undef TH_PASS_KERNEL
#undef TH_PARAMS
#undef TH_PRED
// the rescaled forms (option "cfg_rescale"): thresh_roll_rs_kernel, thresh_pass_rs_kernel rank |g y - m|, g of the quad's group
// from the records the statistics launch left (rs: RescaleUpd::g)
#define TH_ROLL_KERNEL thresh_roll_rs_kernel
#define TH_PASS_KERNEL thresh_pass_rs_kernel
#define TH_PARAMS const ThreshArgs a, const float* rs
#define TH_PRED(i4, y) (pred_quad(a.u, i4, y), rescale_quad(a.u, rs, i4, y))
#include "threshold.hip"
#undef TH_ROLL_KERNEL
#undef TH_PASS_KERNEL
#undef TH_PARAMS
#undef TH_PRED

// g: null = the plain forms; else the rescaled ones
static hipError_t launch_threshold_forms(ThreshArgs a, const float* g, int B, hipStream_t s) {
    const UpdateArgs& u = a.u;
    if (!u.x0c || !a.work || B < 1 || u.per_sample < 4 || (u.per_sample & 3) || u.n != (long)B * u.per_sample ||
        u.n >= (1l << 31) || a.v < 5000 || a.v > 10000 || !(a.r > 0.f))
        return hipErrorInvalidValue;
    if (win_H(u) == 0 && u.per_sample <= THRESH_ROLL_MAX) {
        if (g) hipLaunchKernelGGL(thresh_roll_rs_kernel, dim3((unsigned)B), dim3(512), 0, s, a, g);
        else hipLaunchKernelGGL(thresh_roll_kernel, dim3((unsigned)B), dim3(512), 0, s, a);
        return hipGetLastError();
    }
    if (B > 65535) return hipErrorInvalidValue;
    const long nq = u.per_sample >> 2;
    const dim3 grid((unsigned)((nq + TH_CHUNK - 1) / TH_CHUNK), (unsigned)B);
    for (a.pass = 0; a.pass < 5; ++a.pass) {
        if (g) hipLaunchKernelGGL(thresh_pass_rs_kernel, grid, dim3(256), 0, s, a, g);
        else hipLaunchKernelGGL(thresh_pass_kernel, grid, dim3(256), 0, s, a);
        const hipError_t st = hipGetLastError();
        if (st != hipSuccess) return st;
    }
    return hipSuccess;
}
hipError_t launch_threshold(ThreshArgs a, int B, hipStream_t s) { return launch_threshold_forms(a, nullptr, B, s); }
hipError_t launch_threshold_rescaled(ThreshArgs a, const float* g, int B, hipStream_t s) {
    return g ? launch_threshold_forms(a, g, B, s) : hipErrorInvalidValue;
}

// (dr_debug_threshold) the records of the groups' first rows, in row order, as (G, 2)
__global__ __launch_bounds__(256) void thresh_gather_kernel(const ThreshArgs a, int B, float* out) {
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
        const float* qs = reinterpret_cast<const float*>(a.work + THRESH_HEAD + b * THRESH_ROW_WORDS + THRESH_QS);
        out[2 * g] = qs[0];
        out[2 * g + 1] = qs[1];
    }
}
hipError_t launch_thresh_gather(const ThreshArgs& a, int B, float* out, hipStream_t s) {
    if (!a.work || !out || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(thresh_gather_kernel, dim3(1), dim3(256), 0, s, a, B, out);
    return hipGetLastError();
}

}  // namespace dr

#else      // ================================================ part 2: the two kernels, as part 1 includes them (inside namespace dr)
// ---------------------------------------------------------------------------------------------- one workgroup per roll
__global__ __launch_bounds__(512) void TH_ROLL_KERNEL(TH_PARAMS) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[4];      // the pattern so far, the rank sought within it, the selected bin's count, the successor
    const long row = blockIdx.x;
    const long nq = a.u.per_sample >> 2, q0 = row * nq;
    unsigned k, rem;
    th_rank(a.v, (unsigned)a.u.per_sample, k, rem);
    unsigned prefix = 0u, want = k;
    for (int p = 0; p < 4; ++p) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
        if (threadIdx.x == 0) sel[3] = 0xFFFFFFFFu;
        __syncthreads();
        for (long q = threadIdx.x; q < nq; q += 512) {
            float y[4];
            TH_PRED(q0 + q, y);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned pat = th_pattern(y[e], a.m);
                if (th_match(p, pat, prefix)) atomicAdd(&hist[th_digit(p, pat)], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const unsigned c[4] = {hist[4 * threadIdx.x], hist[4 * threadIdx.x + 1], hist[4 * threadIdx.x + 2], hist[4 * threadIdx.x + 3]};
            unsigned digit, below, eq;
            th_pick(c, want, digit, below, eq);
            if (threadIdx.x == 0) { sel[0] = prefix | (digit << th_shift(p)); sel[1] = want - below; sel[2] = eq; }
        }
        __syncthreads();
        prefix = sel[0]; want = sel[1];
    }
    // a[k] = prefix; `want` is its rank among its sel[2] copies: a[k + 1] is another copy unless it is the last one
    const bool successor = rem != 0u && want + 1u >= sel[2];      // (uniform over the workgroup)
    if (successor) {
        unsigned mn = 0xFFFFFFFFu;
        for (long q = threadIdx.x; q < nq; q += 512) {
            float y[4];
            TH_PRED(q0 + q, y);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned pat = th_pattern(y[e], a.m);
                if (pat > prefix && pat < mn) mn = pat;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const unsigned o = __shfl_xor(mn, off); mn = o < mn ? o : mn; }
        if ((threadIdx.x & 63) == 0) atomicMin(&sel[3], mn);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // (rem != 0 implies k < N - 1: an element above a[k] exists wherever a successor is sought)
        const unsigned ak1 = successor ? sel[3] : prefix;
        th_finish(a.m, a.r, prefix, ak1, rem, reinterpret_cast<float*>(a.work + THRESH_HEAD + row * THRESH_ROW_WORDS + THRESH_QS));
    }
}

// ---------------------------------------------------------------------------------------------- five launches over all rows
// grid (chunks of TH_CHUNK quads, rows).  Pass 0-3: count; pass 4: the smallest pattern above a[k], then q and s.
__global__ __launch_bounds__(256) void TH_PASS_KERNEL(TH_PARAMS) {
    __shared__ unsigned hist[256];
    __shared__ unsigned last_s;
    const int p = a.pass;
    const long row = blockIdx.y, B = gridDim.y;
    const long nq = a.u.per_sample >> 2;
    long first;
    int f_lo;
    thresh_place(a.u, row, first, f_lo);
    unsigned* const rec = a.work + THRESH_HEAD + first * THRESH_ROW_WORDS;
    const unsigned prefix = p > 0 ? rec[THRESH_SEL] : 0u;      // (written by the previous launch)
    hist[threadIdx.x] = 0u;
    __syncthreads();
    long qa = (long)blockIdx.x * TH_CHUNK, qb = qa + TH_CHUNK;
    qa = qa < (long)f_lo * 22 ? (long)f_lo * 22 : qa;
    qb = qb > nq ? nq : qb;
    unsigned mn = 0xFFFFFFFFu;
    for (long q = qa + threadIdx.x; q < qb; q += 256) {
        float y[4];
        TH_PRED(row * nq + q, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned pat = th_pattern(y[e], a.m);
            if (p < 4) {
                if (th_match(p, pat, prefix)) atomicAdd(&hist[th_digit(p, pat)], 1u);
            } else if (pat > prefix && pat < mn) mn = pat;
        }
    }
    if (p < 4) {
        __syncthreads();
        const unsigned c = hist[threadIdx.x];
        if (c) __hip_atomic_fetch_add(rec + threadIdx.x, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const unsigned o = __shfl_xor(mn, off); mn = o < mn ? o : mn; }
        // (kept inverted, so that zero is the armed state)
        if ((threadIdx.x & 63) == 0 && mn != 0xFFFFFFFFu)
            __hip_atomic_fetch_max(rec + THRESH_SEL + 3, ~mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // this workgroup's atomics are performed -> ticket; the last arriver sees every workgroup's
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(a.work, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = ticket == gridDim.x * gridDim.y - 1u;
    }
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    const int lane = (int)(threadIdx.x & 63);
    for (long g = threadIdx.x >> 6; g < B; g += 4) {      // one wave per group
        long gf;
        int gl;
        thresh_place(a.u, g, gf, gl);
        if (gf != g) continue;
        unsigned* const gr = a.work + THRESH_HEAD + g * THRESH_ROW_WORDS;
        if (p < 4) {
            unsigned c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = th_load(gr + 4 * lane + j); th_store(gr + 4 * lane + j, 0u); }
            unsigned want, rem = 0u;
            if (p == 0) {      // every element was counted: the sum is N
                unsigned N = c[0] + c[1] + c[2] + c[3];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) N += __shfl_xor(N, off);
                th_rank(a.v, N, want, rem);
            } else want = th_load(gr + THRESH_SEL + 1);
            unsigned digit, below, eq;
            th_pick(c, want, digit, below, eq);
            if (lane == 0) {
                const unsigned pre = p > 0 ? th_load(gr + THRESH_SEL) : 0u;
                th_store(gr + THRESH_SEL, pre | (digit << th_shift(p)));
                th_store(gr + THRESH_SEL + 1, want - below);
                th_store(gr + THRESH_SEL + 2, eq);
                if (p == 0) th_store(gr + THRESH_SEL + 4, rem);
            }
        } else if (lane == 0) {
            const unsigned ak = th_load(gr + THRESH_SEL), want = th_load(gr + THRESH_SEL + 1), eq = th_load(gr + THRESH_SEL + 2);
            const unsigned inv = th_load(gr + THRESH_SEL + 3), rem = th_load(gr + THRESH_SEL + 4);
            const unsigned ak1 = (rem != 0u && want + 1u >= eq) ? ~inv : ak;
            th_finish(a.m, a.r, ak, ak1, rem, reinterpret_cast<float*>(gr + THRESH_QS));
            th_store(gr + THRESH_SEL + 3, 0u);
        }
    }
    if (threadIdx.x == 0) th_store(a.work, 0u);
}

#endif
