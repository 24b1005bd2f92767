// gfx950 (MI355X, CDNA4) kernels of the DiffRoll sampling engine.
//
// One implicit-GEMM design carries every contraction of the path, in three consumer flavours that share
// the LDS-DMA producers, the P4 / S3 activation layouts and the packed weights:
//   gemm_kernel<.., PREC=0>  exact fp32 on v_mfma_f32_32x32x2_f32      (default; 64/128-frame blocks)
//   gemm_kernel<.., PREC=1>  split-bf16 on v_mfma_f32_32x32x16_bf16    (opt-in "bf16x3", hot kernels)
//   gemm_kernel<.., PREC=2>  one-pass bf16 on the same MFMA            (opt-in "bf16", hot kernels)
//   gemm_kernel<.., PREC=4>  one-pass fp16 on v_mfma_f32_32x32x16_f16   (opt-in "f16", hot kernels)
//   gemm16_kernel            exact fp32 on v_mfma_f32_16x16x4_f32      (96/160-frame blocks, hot kernels)
// used for
//   * dilated Conv1d (k taps) + conditioner add + sigmoid*tanh gate   (model/diffwave.py:139-147)
//   * 1x1 output projection + residual/skip update (+ h + d_next)      (model/diffwave.py:149-151, :138)
//   * input / skip / output projections of the net                     (model/diffwave.py:667-668, 683-685)
//   * conditioner projections, step-embedding MLP                      (hoisted; :126,128,65-74)
//   * the STFT as a windowed-DFT GEMM and the mel filterbank GEMM      (torchaudio MelSpectrogram)
// plus small HBM-bound kernels: posterior update (all nine samplers) + classifier-free combine + Philox
// noise (task/diffusion.py:804-1055), reflect padding, per-sample min/max + normalise/mask/trim
// (model/utils.py:21-32, model/diffwave.py:644-662), frame confusion counts (:381-383) and the
// roll -> note-run scan (:1185-1233).
//
// Written for wave64, 512-thread workgroups (4 consumer + 4 producer waves); gfx950 only.
#include "gemm_body.h"

namespace dr {

Tuning& tuning() { static Tuning t; return t; }
std::atomic<unsigned>& tuning_epoch() { static std::atomic<unsigned> n{0}; return n; }
PlanKnobs plan_knobs() {
    const Tuning& t = tuning();
    PlanKnobs k;
    k.tile = t.tile; k.pw = t.pw; k.pw_nw = t.pw_nw; k.pwk = t.pwk; k.ksplit_max = t.ksplit_max;
    k.ksplit_blocks = t.ksplit_blocks; k.stack3 = t.stack3; k.stack_fl = t.stack_fl;
    k.xcd_n = t.xcd_n; k.xcd_model = t.xcd_model; k.tail_t4 = t.tail_t4; k.one_ks = t.one_ks;
    return k;
}

DR_BOUNDS_TU(gemm)
hipError_t read_bounds(unsigned long long* out4) {
    unsigned long long t[4];
    hipError_t e;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    hipError_t (*readers[])(unsigned long long*) = {read_bounds_gemm, read_bounds_stack, read_bounds_tail};
    for (auto rd : readers) {
        if ((e = rd(t)) != hipSuccess) return e;
        if (!out4[0] && t[0]) { out4[0] = t[0]; out4[1] = t[1]; out4[2] = t[2]; }
        out4[3] += t[3];
    }
    return hipSuccess;
}
hipError_t reset_bounds() {
    hipError_t e;
    if ((e = reset_bounds_gemm()) != hipSuccess) return e;
    if ((e = reset_bounds_stack()) != hipSuccess) return e;
    return reset_bounds_tail();
}

// Block -> (M tile, frame tile, K split) of a per-phase GEMM launch.
// blockIdx.x % MT = M tile: with MT == 8 each XCD (block b runs on XCD b % 8) streams exactly
// one 128-row weight panel, which then stays resident in that XCD's private L2.
// xcd_n != 0 (X-heavy 1x1 GEMMs: small weights, big activations): the 8 M tiles of one frame tile
// run on the SAME XCD instead, so the X tile is fetched from HBM once per XCD and hits L2 for the
// other M tiles, while the (small) weight matrix is L2-resident in every XCD.
// Split-K (ksplit > 1, gemm_kernel's under-filled launches only: few samples / narrow GEMMs): ksplit blocks share
// one output tile, each contracts a contiguous range of the K chunks; see the reduction in gemm_body.
struct BlockTile { int mt, nt, ks; };
DR_DEVINL BlockTile block_tile(const GemmArgs& a, const int ksplit) {
    BlockTile o;
    if (a.xcd_n) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        o.mt = idx % a.MT;
        const int rest = idx / a.MT;
        o.ks = rest % ksplit;
        o.nt = (rest / ksplit) * 8 + xcd;
    } else {
        o.mt = blockIdx.x % a.MT;
        const int rest = blockIdx.x / a.MT;
        o.ks = rest % ksplit;
        o.nt = rest / ksplit;
    }
    return o;
}

template <int NI, int KS, int EPI, int PREC, int FOLDP = (NI == 1)>
__global__ __launch_bounds__(512) void gemm_kernel(const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BlockTile bt = block_tile(a, a.ksplit);
    gemm_body<NI, KS, EPI, PREC, 0, FOLDP>(a, smem, bt.mt, bt.nt, bt.ks);
}

template <int NW>
__global__ __launch_bounds__(256) void pw_kernel(const GemmArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const BlockTile bt = block_tile(a, 1);
    // + mt0: launches over a sub-range of the M tiles (the last layer only needs its skip rows)
    pw_body<NW, 0, 0>(a, bt.mt + a.mt0, bt.nt, wave);
}

// ---------------------------------------------------------------------------------------------
// The 1x1 residual / skip GEMM for launches that cannot fill the chip (single clips: 2 evaluations x 125 frames are 32
// of pw_kernel's tiles).  Block = 4 waves on ONE 32-row x 32*NW-frame output tile, the waves splitting K in-block: wave
// w contracts the w-th quarter of the channel slabs (k ascending inside it) with both operands straight from L2, the
// four partial tiles meet in LDS and are added in wave order ((p0 + p1) + p2) + p3 - deterministic, independent of
// timing - and wave w runs the epilogue of register quad w (8 rows x 4... = one float4 of the P4 layout per lane and
// frame tile).  256 blocks at config 1 with a K loop of 64 MFMAs per wave instead of 32 tiles x 8 K slices exchanged
// through a workspace with tickets: 13.9 -> ~8 us per launch.  Same epilogue arithmetic as pw_body (EPI_RES_SKIP).
// ---------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(256) void pwk_kernel(const GemmArgs a) {
    __shared__ float4 part[4][NW][4][64];                      // [wave][frame tile][quad][lane]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, hi = lane >> 5;
    constexpr int BN = 32 * NW;
    const int RT = a.MT * 4;                                   // 32-row tiles
    const int rt = blockIdx.x % RT + a.mt0 * 4, nt = blockIdx.x / RT;
    const int mt = rt >> 2, sr = rt & 3;                       // 128-row weight panel, 32-row sub-tile
    const int tps = (a.T + BN - 1) / BN;
    const int b = nt / tps;
    const int t0 = (nt % tps) * BN;
    const int NS = a.kchunks, NSW = NS >> 2;                   // slabs (32 channels) in all / per wave
    const int s0 = wave * NSW;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.Wp + (long)mt * NS * 4096), 0, (unsigned)NS * 16384u, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.X + (long)b * a.x_bs), 0, (unsigned)(a.x_planes * a.x_ps * 4), 0x00020000);
    const int wvo = (hi * 128 + sr * 32 + r) * 16;
    const int xps = (int)a.x_ps * 4;
    int xvo[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni) xvo[ni] = hi * xps + min(t0 + ni * 32 + r, a.T - 1) * 16;
    using BF = BF4<NW>;
    auto load_a = [&](int slab) { return load_a4(wr, wvo, slab, NS, 140); };
    auto load_b = [&](int slab) { return load_b4(xr, xvo, xps, slab); };
    // the epilogue operands of THIS wave's quad (q = wave): requested first, their latency hides behind the K loop
    const int p0 = mt * 128 + sr * 32 + 8 * wave + 4 * hi;     // first of the lane's 4 packed rows
    const bool res_rows = p0 < a.y_rows;                       // wave-uniform (y_rows is a multiple of 64)
    const float4 ebias = *reinterpret_cast<const float4*>(a.bias + p0);
    const float4 ed2 = *reinterpret_cast<const float4*>(a.d2 + (a.tsel ? (long)a.tsel[b] * a.d2_ts : 0) + min(p0, a.y_rows - 4));
    float4 eop[NW];
    {
        const float* base = res_rows ? a.Y + (long)b * a.y_bs + (long)(p0 >> 2) * a.y_ps
                                     : a.skip + (long)b * a.s_bs + (long)((p0 - a.y_rows) >> 2) * a.T * 4;
        const long fs = res_rows ? a.y_fs : 4;
#pragma unroll
        for (int ni = 0; ni < NW; ++ni) eop[ni] = *reinterpret_cast<const float4*>(base + (long)min(t0 + ni * 32 + r, a.T - 1) * fs);
    }

    f32x16 acc[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
    AF4 aA = load_a(s0), aB;
    BF bA = load_b(s0), bB;
    auto mma = [&](const AF4& af, const BF& bf) {
#pragma unroll
        for (int g = 0; g < 4; ++g) mma_f32x4<0, 0, NW>(acc, af.v[g], bf.v[g]);
    };
    int slab = 0;
    for (; slab + 2 <= NSW; slab += 2) {          // two register sets, prefetch distance one slab
        aB = load_a(s0 + slab + 1); bB = load_b(s0 + slab + 1);
        mma(aA, bA);
        const int nx = s0 + min(slab + 2, NSW - 1);
        aA = load_a(nx); bA = load_b(nx);
        mma(aB, bB);
    }
    if (slab < NSW) mma(aA, bA);

    // the four partial tiles meet in LDS; wave w sums register quad w of every frame tile in wave order
#pragma unroll
    for (int ni = 0; ni < NW; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            part[wave][ni][q][lane] = make_float4(acc[ni][4 * q], acc[ni][4 * q + 1], acc[ni][4 * q + 2], acc[ni][4 * q + 3]);
    __syncthreads();
#pragma unroll
    for (int ni = 0; ni < NW; ++ni) {
        const int t = t0 + ni * 32 + r;
        if (t >= a.T) continue;
        float v[4], o[4], u[4];
        f4arr(part[0][ni][wave][lane], v);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            f4arr(part[w][ni][wave][lane], u);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += u[e];
        }
        if (res_rows) {          // h in place, hd = h + d_{l+1}
            float* dst = y_quad_ptr(a, b, p0, t);
            residual_quad(v, ebias, eop[ni], o);
            store_quad(dst, o);
            if (a.Y2) {          // (fp32 only: launch_pointwise_ksplit)
                float o2[4];
                hd_quad(o, ed2, o2);
                float* dst2 = a.Y2 + (long)b * a.y2_bs + (long)(p0 >> 2) * a.y_ps + (long)t * a.y_fs;
                store_quad(dst2, o2);
            }
        } else {
            float* dst = skip_quad_ptr(a, b, p0, t);
            skip_quad(v, ebias, eop[ni], a.skip_init, o);
            store_quad(dst, o);
        }
    }
}

template <int NW>
static hipError_t launch_pwk_t(const GemmArgs& a, hipStream_t s) {
    const int BN = 32 * NW;
    const int NT = a.NB * ((a.T + BN - 1) / BN);
    DR_CHECK_EXTENTS(a, EPI_RES_SKIP, 0, "pwk_kernel");
    hipLaunchKernelGGL((pwk_kernel<NW>), dim3((unsigned)(a.MT * 4 * NT)), dim3(256), 0, s, a);
    return hipGetLastError();
}
// 1x1 EPI_RES_SKIP GEMM of an under-filled launch, fp32: block = 32 rows x 32*NW frames, K split over its 4 waves
hipError_t launch_pointwise_ksplit(const GemmArgs& a, int NW, hipStream_t s) {
    if (a.taps != 1 || a.kchunks < 4 || (a.kchunks & 3) || a.x_fs != 4 || a.out_s3) return hipErrorInvalidValue;
    return NW == 1 ? launch_pwk_t<1>(a, s) : NW == 2 ? launch_pwk_t<2>(a, s) : hipErrorInvalidValue;
}

// Block -> XCD mapping of this launch: launch_plan.h: pick_xcd_mapping, under the knobs as they are now
static int pick_xcd_mapping(const GemmArgs& a, int NT, int BN) {
    return pick_xcd_mapping(plan_knobs(), a.MT, NT, BN, a.kchunks, a.taps);
}

template <int NW>
static hipError_t launch_pw_t(const GemmArgs& a, hipStream_t s) {
    const int BN = 32 * NW;
    const int NT = a.NB * ((a.T + BN - 1) / BN);
    GemmArgs b = a;
    b.xcd_n = pick_xcd_mapping(a, NT, BN);      // (a.taps == 1: launch_pointwise)
    DR_CHECK_EXTENTS(b, EPI_RES_SKIP, 0, "pw_kernel");
    hipLaunchKernelGGL((pw_kernel<NW>), dim3((unsigned)(a.MT * NT)), dim3(256), 0, s, b);
    return hipGetLastError();
}
// 1x1 EPI_RES_SKIP GEMM, fp32, operands direct from L2; block = 128 rows x 32*NW frames, NW in {2,3,4,5}
hipError_t launch_pointwise(const GemmArgs& a, int NW, hipStream_t s) {
    if (a.taps != 1 || a.kchunks < 1 || a.x_fs != 4) return hipErrorInvalidValue;
    switch (NW) {
        case 2: return launch_pw_t<2>(a, s);
        case 3: return launch_pw_t<3>(a, s);
        case 4: return launch_pw_t<4>(a, s);
        case 5: return launch_pw_t<5>(a, s);
    }
    return hipErrorInvalidValue;
}

template <int NJ, int KS, int EPI>
__global__ __launch_bounds__(512) void gemm16_kernel(const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BlockTile bt = block_tile(a, 1);
    gemm16_body<NJ, KS, EPI>(a, smem, bt.mt, bt.nt);
}

template <int NJ, int KS, int EPI>
static hipError_t launch_gemm16_t(const GemmArgs& a, hipStream_t s) {
    const int BN = 32 * NJ;
    const int halo = ((a.taps - 1) / 2) * a.dil;
    const size_t lds = (size_t)2 * 8 * KS * (BN + 2 * halo) * 16 + (EPI == EPI_RES_SKIP ? (size_t)32 * BN * 16 : 0);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int NT = a.NB * ((a.T + BN - 1) / BN);
    GemmArgs b = a;
    b.xcd_n = pick_xcd_mapping(a, NT, BN);
    b.lds_bytes = (int)lds;
    DR_CHECK_EXTENTS(b, EPI, 0, "gemm16_kernel");
    hipLaunchKernelGGL((gemm16_kernel<NJ, KS, EPI>), dim3((unsigned)(a.MT * NT)), dim3(512), lds, s, b);
    return hipGetLastError();
}
// frames per block = 32 * NJ; NJ in {3, 5}: 96 / 160 (64 and 128 are served by gemm_kernel; 192 does not fit the
// 256-register budget of a 512-thread block without spilling)
hipError_t launch_gemm16(const GemmArgs& a, int epi, int NJ, hipStream_t s) {
    if (a.kchunks < 1) return hipErrorInvalidValue;
    if (epi == EPI_GATE) {
        if (NJ == 3) return launch_gemm16_t<3, 1, EPI_GATE>(a, s);
        if (NJ == 5) return launch_gemm16_t<5, 1, EPI_GATE>(a, s);
    } else if (epi == EPI_RES_SKIP && a.taps == 1 && a.kchunks % 2 == 0) {
        if (NJ == 3) return launch_gemm16_t<3, 2, EPI_RES_SKIP>(a, s);
        if (NJ == 5) return launch_gemm16_t<5, 2, EPI_RES_SKIP>(a, s);
    }
    return hipErrorInvalidValue;
}
static hipError_t init_gemm16() {
    return allow_max_lds(&gemm16_kernel<3, 1, EPI_GATE>, &gemm16_kernel<5, 1, EPI_GATE>,
                         &gemm16_kernel<3, 2, EPI_RES_SKIP>, &gemm16_kernel<5, 2, EPI_RES_SKIP>);
}

template <int NI, int KS, int EPI, int PREC>
static hipError_t launch_gemm_t(const GemmArgs& a, hipStream_t s) {
    const int BN = gemm_block_frames(NI);
    const int tps = (a.T + BN - 1) / BN;
    const size_t lds = gemm_lds_bytes(NI, KS, a.taps, a.dil, PREC, EPI);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int NT = a.NB * tps;
    GemmArgs b = a;
    // Split-K: launches that cannot fill the chip, and launches that fill it unevenly.  The ticket reduction needs no
    // co-residency (nobody spins), so a launch may be cut into MORE blocks than the chip holds: 10 evaluations of 125
    // frames are 160 tiles = one round of full-K blocks on 62 % of the CUs; cut 4x in K they are 640 blocks = 3 rounds
    // of quarter-length blocks: 136 -> 107 us per conv launch.  The decision is plan_ksplit's (shared with the engine).
    b.ksplit = 1;
    if (a.ws && a.ws_cnt) b.ksplit = plan_ksplit(plan_knobs(), (long)a.MT * NT, a.kchunks / KS, a.kchunks, a.taps, NI, PREC, a.ws_floats, a.ws_cnt_n).ks;
    b.lds_bytes = (int)lds;
    const dim3 grid((unsigned)(a.MT * NT * b.ksplit));
    b.xcd_n = pick_xcd_mapping(a, NT, BN);
    DR_CHECK_EXTENTS(b, EPI, PREC, "gemm_kernel");
    // the 128-frame gated conv exists with and without blocked accumulation (GemmArgs::fold128)
    if constexpr (NI == 2 && KS == 1 && EPI == EPI_GATE) {
        if (a.fold128) {
            hipLaunchKernelGGL((gemm_kernel<2, 1, EPI_GATE, PREC, 1>), grid, dim3(512), lds, s, b);
            return hipGetLastError();
        }
    }
    if constexpr (NI == 1 && KS == 1 && EPI == EPI_GATE && PREC == 0) {
        if (a.nofold64 && b.ksplit == 1) {    // (see GemmArgs::nofold64)
            hipLaunchKernelGGL((gemm_kernel<1, 1, EPI_GATE, 0, 0>), grid, dim3(512), lds, s, b);
            return hipGetLastError();
        }
    }
    if constexpr (NI == 3 || NI == 5) {       // 96 / 160-frame blocks: the gated conv with blocked accumulation only
        hipLaunchKernelGGL((gemm_kernel<NI, 1, EPI_GATE, 0, 1>), grid, dim3(512), lds, s, b);
        return hipGetLastError();
    } else {
        hipLaunchKernelGGL((gemm_kernel<NI, KS, EPI, PREC>), grid, dim3(512), lds, s, b);
        return hipGetLastError();
    }
}

template <int NI, int KS>
static hipError_t init_gemm_ni() {
    return allow_max_lds(&gemm_kernel<NI, KS, EPI_PLAIN, 0>, &gemm_kernel<NI, KS, EPI_RELU, 0>, &gemm_kernel<NI, KS, EPI_SILU, 0>,
                         &gemm_kernel<NI, KS, EPI_GATE, 0>, &gemm_kernel<NI, KS, EPI_RES_SKIP, 0>, &gemm_kernel<NI, KS, EPI_POWER, 0>,
                         &gemm_kernel<NI, KS, EPI_LOG, 0>);
}
// allow > 64 KiB of dynamic LDS for every instantiation; call once per process before any launch
// (and never inside a stream capture)
hipError_t init_kernels() {
    hipError_t e;
    if ((e = init_gemm_ni<1, 1>()) != hipSuccess) return e;
    if ((e = init_gemm_ni<2, 1>()) != hipSuccess) return e;
    if ((e = init_gemm_ni<1, 2>()) != hipSuccess) return e;
    if ((e = init_gemm_ni<2, 2>()) != hipSuccess) return e;
    if ((e = init_gemm_ni<1, 4>()) != hipSuccess) return e;
    if ((e = init_gemm_ni<2, 4>()) != hipSuccess) return e;
    // split-bf16 instantiations: dilated conv (KS = 1) and 1x1 (NI = 1: KS = 4)
    if ((e = allow_max_lds(&gemm_kernel<1, 1, EPI_GATE, 1>, &gemm_kernel<2, 1, EPI_GATE, 1>, &gemm_kernel<1, 4, EPI_RES_SKIP, 1>,
                           &gemm_kernel<1, 1, EPI_RES_SKIP, 1>)) != hipSuccess) return e;
    // one-pass bf16 instantiations: the same four, and the 128-frame conv with blocked accumulation
    if ((e = allow_max_lds(&gemm_kernel<1, 1, EPI_GATE, 2>, &gemm_kernel<2, 1, EPI_GATE, 2>, &gemm_kernel<1, 4, EPI_RES_SKIP, 2>,
                           &gemm_kernel<1, 1, EPI_RES_SKIP, 2>, &gemm_kernel<2, 1, EPI_GATE, 2, 1>)) != hipSuccess) return e;
    // one-pass f16 instantiations: the same five
    if ((e = allow_max_lds(&gemm_kernel<1, 1, EPI_GATE, 4>, &gemm_kernel<2, 1, EPI_GATE, 4>, &gemm_kernel<1, 4, EPI_RES_SKIP, 4>,
                           &gemm_kernel<1, 1, EPI_RES_SKIP, 4>, &gemm_kernel<2, 1, EPI_GATE, 4, 1>)) != hipSuccess) return e;
    // the explicit FOLDP flavours of the gated conv, and the 96 / 160-frame blocks
    if ((e = allow_max_lds(&gemm_kernel<2, 1, EPI_GATE, 0, 1>, &gemm_kernel<1, 1, EPI_GATE, 0, 0>, &gemm_kernel<2, 1, EPI_GATE, 1, 1>,
                           &gemm_kernel<5, 1, EPI_GATE, 0, 1>, &gemm_kernel<3, 1, EPI_GATE, 0, 1>)) != hipSuccess) return e;
    if ((e = init_frontend_kernels()) != hipSuccess) return e;
    if ((e = init_update_kernels()) != hipSuccess) return e;
    if ((e = init_tail_kernels()) != hipSuccess) return e;
    if ((e = init_stack_kernels()) != hipSuccess) return e;
    return init_gemm16();
}

// precisions "bf16" / "f16": the P4 fp32 tensor as one 16-bit plane set.  One thread per (sample, plane8, frame): two float4
// in (the planes 2 p and 2 p + 1 of that frame), one 16-byte unit out; pack2(lo, hi) = the mode's rounding of two values.
template <class Pack2>
DR_DEVINL void round16_unit(const float* __restrict__ src, float* __restrict__ dst, const int P8, const int T, const long n, Pack2 pack2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;       // = (b * P8 + p) * T + t
    if (i >= n) return;
    const long bp = i / T;
    const int t = (int)(i - bp * T);
    const long b = bp / P8;
    const int p = (int)(bp - b * P8);
    const float* s0 = src + ((b * 2 * P8 + 2 * p) * (long)T + t) * 4;
    const float4 lo = *reinterpret_cast<const float4*>(s0);
    const float4 hi = *reinterpret_cast<const float4*>(s0 + (long)T * 4);
    uint4 o;
    o.x = pack2(lo.x, lo.y);
    o.y = pack2(lo.z, lo.w);
    o.z = pack2(hi.x, hi.y);
    o.w = pack2(hi.z, hi.w);
    *reinterpret_cast<uint4*>(dst + i * 4) = o;
}
__global__ __launch_bounds__(256) void round_bf16_kernel(const float* __restrict__ src, float* __restrict__ dst, const int P8, const int T,
                                                         const long n) {
    round16_unit(src, dst, P8, T, n, [](float lo, float hi) { return (bf16_rne_bits(lo) >> 16) | bf16_rne_bits(hi); });
}
__global__ __launch_bounds__(256) void round_f16_kernel(const float* __restrict__ src, float* __restrict__ dst, const int P8, const int T,
                                                        const long n) {
    round16_unit(src, dst, P8, T, n, [](float lo, float hi) { return f16_rne_pair(lo, hi); });
}
template <class K>
static hipError_t launch_round16(K kernel, const float* src, float* dst, int NB, int Cp, int T, hipStream_t s) {
    if (NB < 1 || T < 1 || Cp < 8 || (Cp & 7)) return hipErrorInvalidValue;
    const long n = (long)NB * (Cp >> 3) * T;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, Cp >> 3, T, n);
    return hipGetLastError();
}
hipError_t launch_round_bf16(const float* src, float* dst, int NB, int Cp, int T, hipStream_t s) {
    return launch_round16(round_bf16_kernel, src, dst, NB, Cp, T, s);
}
hipError_t launch_round_f16(const float* src, float* dst, int NB, int Cp, int T, hipStream_t s) {
    return launch_round16(round_f16_kernel, src, dst, NB, Cp, T, s);
}

template <int NI, int KS>
static hipError_t launch_gemm_ni(const GemmArgs& a, int epi, hipStream_t s) {
    switch (epi) {
        case EPI_PLAIN: return launch_gemm_t<NI, KS, EPI_PLAIN, 0>(a, s);
        case EPI_RELU: return launch_gemm_t<NI, KS, EPI_RELU, 0>(a, s);
        case EPI_SILU: return launch_gemm_t<NI, KS, EPI_SILU, 0>(a, s);
        case EPI_GATE: return launch_gemm_t<NI, KS, EPI_GATE, 0>(a, s);
        case EPI_RES_SKIP: return launch_gemm_t<NI, KS, EPI_RES_SKIP, 0>(a, s);
        case EPI_POWER: return launch_gemm_t<NI, KS, EPI_POWER, 0>(a, s);
        case EPI_LOG: return launch_gemm_t<NI, KS, EPI_LOG, 0>(a, s);
    }
    return hipErrorInvalidValue;
}

// split-bf16, one-pass bf16 or one-pass f16 input: only the two hot kernels exist in these precisions
template <int PREC>
static hipError_t launch_gemm_lowp(const GemmArgs& a, int epi, int NI, hipStream_t s) {
    if (epi == EPI_GATE) return NI == 1 ? launch_gemm_t<1, 1, EPI_GATE, PREC>(a, s) : launch_gemm_t<2, 1, EPI_GATE, PREC>(a, s);
    if (epi == EPI_RES_SKIP && a.taps == 1)
        return a.kchunks % 4 == 0 ? launch_gemm_t<1, 4, EPI_RES_SKIP, PREC>(a, s) : launch_gemm_t<1, 1, EPI_RES_SKIP, PREC>(a, s);
    return hipErrorInvalidValue;
}

hipError_t launch_gemm(const GemmArgs& a, int epi, int NI, hipStream_t s, int prec) {
    if (a.kchunks < 1) return hipErrorInvalidValue;   // the X tile width is only bounded by LDS (checked per launch)
    if (prec == DR_PRECISION_F16) return launch_gemm_lowp<DR_PRECISION_F16>(a, epi, NI, s);
    if (prec == DR_PRECISION_BF16) return launch_gemm_lowp<DR_PRECISION_BF16>(a, epi, NI, s);
    if (prec == DR_PRECISION_BF16X3) return launch_gemm_lowp<DR_PRECISION_BF16X3>(a, epi, NI, s);
    if (prec != DR_PRECISION_F32) return hipErrorInvalidValue;
    const int KS = pick_one_ks(a.taps, a.kchunks, NI, epi, tuning().one_ks);      // channels per hand-over (launch_plan.h)
    if (NI == 1) {
        if (KS == 4) return launch_gemm_ni<1, 4>(a, epi, s);
        return KS == 2 ? launch_gemm_ni<1, 2>(a, epi, s) : launch_gemm_ni<1, 1>(a, epi, s);
    }
    if (NI == 2) {
        if (KS == 4) return launch_gemm_ni<2, 4>(a, epi, s);
        return KS == 2 ? launch_gemm_ni<2, 2>(a, epi, s) : launch_gemm_ni<2, 1>(a, epi, s);
    }
    if (NI == 5 && epi == EPI_GATE && KS == 1) return launch_gemm_t<5, 1, EPI_GATE, 0>(a, s);
    if (NI == 3 && epi == EPI_GATE && KS == 1) return launch_gemm_t<3, 1, EPI_GATE, 0>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace dr
