// The three GEMM bodies every contraction of the path is made of (device code, templates): gemm_body (LDS-staged X,
// 32x32x2 fp32 / 32x32x16 split-bf16 or one-pass bf16 / f16 MFMA), pw_body (1x1, both operands straight from L2) and gemm16_body (16x16x4 MFMA,
// 96 / 160-frame blocks).  Included by gemm.hip (one launch per phase), stack.hip and tail.hip (persistent kernels): the
// same device code everywhere, which is what makes the fused kernels bit-identical to the per-phase launches.
// What the bodies have in common is written once, in front of them: the epilogue arithmetic on register quads
// (residual_quad, skip_quad, gate_quad, hd_quad / store_y2 - pwk_kernel uses them too), where an output / skip quad lives and
// its plain store (y_quad_ptr, skip_quad_ptr, store_quad), the A-fragment loader (load_a4), the fp32 MFMA group (mma_f32x4),
// the B-fragment loader of the two direct 1x1 kernels (load_b4) and the producer waves of the two LDS-staged bodies (producer,
// with dma_tile for the read-modify-write tile - also used by stack_kernel for its resident tile).  Where a result goes stays
// with the body that computed it.  What was tried beyond that and changed the machine code: profiles/kstep_once_isa.txt.
#pragma once
#include "device_common.h"
#include "zero_taps.h"

namespace dr {

// ---------------------------------------------------------------------------------------------
// Epilogue arithmetic on one C/D register quad (4 consecutive packed rows of one frame = one float4 of the P4 layout).
// ---------------------------------------------------------------------------------------------
// h = (h + (acc + b)) / sqrt(2)   (model/diffwave.py:151)
DR_DEVINL void residual_quad(const float (&v)[4], const float4 bias, const float4 prev, float (&o)[4]) {
    float bb[4], pv[4];
    f4arr(bias, bb); f4arr(prev, pv);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = div_sqrt2(pv[e] + (v[e] + bb[e]));
}
// skip (+)= acc + b   (model/diffwave.py:680); the first layer starts the sum
DR_DEVINL void skip_quad(const float (&v)[4], const float4 bias, const float4 prev, const bool skip_init, float (&o)[4]) {
    float bb[4], pv[4];
    f4arr(bias, bb); f4arr(prev, pv);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = skip_init ? v[e] + bb[e] : (v[e] + bb[e]) + pv[e];
}
// The conditioner tensor conditional sample b of a launch reads (GemmArgs::c_b0 / c_n): once per (tile, sample), and the
// division only where a row lies past the clips (option "draws" > 1)
DR_DEVINL long cond_row(const GemmArgs& a, const int b) {
    int r = a.c_b0 + b;
    if (a.c_n > 0 && r >= a.c_n) r %= a.c_n;
    return r;
}
// y = conv + b_conv + (Wc spec + bc), gate = first half, filter = second   [model/diffwave.py:143-147]: v0 / v1 = the
// gate / filter rows of the same 4 channels; samples without a conditioner (has_c = false) carry the constant
// unconditional one inside their bias
DR_DEVINL void gate_quad(const float (&v0)[4], const float (&v1)[4], const float4 bias0, const float4 bias1,
                         const float4 cond0, const float4 cond1, const bool has_c, float (&o)[4]) {
    float b0[4], b1[4], c0[4], c1[4];
    f4arr(bias0, b0); f4arr(bias1, b1);
    f4arr(cond0, c0); f4arr(cond1, c1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a0 = has_c ? b0[e] + c0[e] : b0[e];
        const float a1 = has_c ? b1[e] + c1[e] : b1[e];
        o[e] = gatef_(v0[e] + a0, v1[e] + a1);
    }
}
// Where the P4 quad of rows p0 .. p0+3, frame t of sample b lives: in the output Y (p0 = the output's own row) and in the
// skip sum (p0 = the packed row of the residual / skip GEMM, >= y_rows: its skip half) - and its plain store
DR_DEVINL float* y_quad_ptr(const GemmArgs& a, const int b, const int p0, const int t) {
    return a.Y + (long)b * a.y_bs + (long)(p0 >> 2) * a.y_ps + (long)t * a.y_fs;
}
DR_DEVINL float* skip_quad_ptr(const GemmArgs& a, const int b, const int p0, const int t) {
    return a.skip + (long)b * a.s_bs + ((long)((p0 - a.y_rows) >> 2) * a.T + t) * 4;
}
DR_DEVINL void store_quad(float* dst, const float (&o)[4]) { *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]); }
// the second output hd = h + d: the next dilated conv's input (model/diffwave.py:139)
DR_DEVINL void hd_quad(const float (&h)[4], const float4 d, float (&o)[4]) {
    float dd[4];
    f4arr(d, dd);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = h[e] + dd[e];
}
// ... and its store for rows p0..p0+3, frame t of sample b: split-bf16 (a.out_s3 & 2) or fp32 P4.  COH3 / COH4: that
// flavour's store is write-through when a.wt_store says so (tensors handed to other workgroups of a fused launch), else plain.
// BF: the precision code of a one-plane 16-bit tensor (precisions "bf16" / "f16": the bodies with PREC = 2 / 4 write nothing
// else), 0 otherwise
template <int COH3, int COH4, int BF = 0>
DR_DEVINL void store_y2(const GemmArgs& a, const int b, const float (&o)[4], const float4 d, const int p0, const int t) {
    float o2[4];
    hd_quad(o, d, o2);
    if constexpr (BF) {
        store_quad_of<BF, COH3>(a.Y2 + (long)b * a.y2_bs, o2, p0, t, a.T, a.wt_store);
    } else if (a.out_s3 & 2) {
        store_s3_quad<COH3>(a.Y2 + (long)b * a.y2_bs, o2, p0, t, a.T, a.y_rows >> 3, a.wt_store);
    } else {
        float* dst2 = a.Y2 + (long)b * a.y2_bs + (long)(p0 >> 2) * a.y_ps + (long)t * a.y_fs;
        store_f4<COH4>(dst2, make_float4(o2[0], o2[1], o2[2], o2[3]), a.wt_store);
    }
}

// The 4 fp32 A fragments of K step `slab` of a weight panel (fragment-shaped packing: 16 KiB per 32-channel slab, 4 KiB
// per 8-channel group; wvo = this lane's byte offset inside a group)
DR_DEVINL AF4 load_a4(const __amdgpu_buffer_rsrc_t wrsrc, const int wvo, const int slab, const int NS, const int code) {
    AF4 o;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        DR_CHECK(slab >= 0 && wvo + slab * 16384 + g * 4096 + 16 <= NS * 16384, code, slab, NS);
        o.v[g] = buffer_load_f4(wrsrc, wvo, slab * 16384 + g * 4096);
    }
    return o;
}

// The fp32 MFMA group: 8 channels of K (one A fragment, one B fragment per tile) for the 32-frame tiles [LO, HI) of a
// wave's N, as 4 x v_mfma_f32_32x32x2_f32 per tile with the tile index innermost - consecutive MFMAs go to different
// accumulators (the pinned schedules keep program order inside their small groups: a chain of dependent back-to-back
// MFMAs costs ~8 cycles each).  FM: bit ni = tile ni starts a new chain here (C = 0 in its first MFMA).
template <int FM, int LO, int HI, int N>
DR_DEVINL void mma_f32x4(f32x16 (&acc)[N], const float4 af, const float4 (&bf)[N]) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ni = LO; ni < HI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf[ni].x, ((FM >> ni) & 1) ? zero16 : acc[ni], 0, 0, 0);
#pragma unroll
    for (int ni = LO; ni < HI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf[ni].y, acc[ni], 0, 0, 0);
#pragma unroll
    for (int ni = LO; ni < HI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf[ni].z, acc[ni], 0, 0, 0);
#pragma unroll
    for (int ni = LO; ni < HI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf[ni].w, acc[ni], 0, 0, 0);
}
// The B fragments of a K step of a 1x1 GEMM that reads them straight from L2 (pw_body, pwk_kernel), [8-channel group][32-frame
// tile]: xr = the sample's X tensor, xvo = this lane's fixed byte offsets of its frames, xps = bytes per plane.  (The two
// resources, wvo and xvo[] stay spelled out in both: as shared helpers they change pw_kernel's or pwk_kernel's digests.)
template <int NW> struct BF4 { float4 v[4][NW]; };
template <int NW>
DR_DEVINL BF4<NW> load_b4(const __amdgpu_buffer_rsrc_t xr, const int (&xvo)[NW], const int xps, const int slab) {
    BF4<NW> o;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ni = 0; ni < NW; ++ni)
            o.v[g][ni] = buffer_load_f4(xr, xvo[ni], (slab * 8 + g * 2) * xps);
    return o;
}

typedef __attribute__((address_space(3))) void* lds_ptr;

// LDS-DMA of a read-modify-write tile, global -> Rs = [32 planes (4 packed rows each)][BN frames] float4, frames t0.. of
// the planes plane_of(pl) (global address of frame 0; T frames of 16 B: frames >= T read 0), dealt over the waves
// first, first + stride, ...  AUX = 16: sc1 loads (the tile was written by this workgroup in an earlier phase of the same
// launch - bypass the L1).
template <int BN, int AUX, class PlaneOf>
DR_DEVINL void dma_tile(float4* Rs, PlaneOf plane_of, const int T, const int t0, const int first, const int stride, const int lane, const int code) {
    constexpr int RWL = (BN + 63) / 64;                 // 64-frame segments of a tile row
    for (int i = first; i < 32 * RWL; i += stride) {
        const int pl = i / RWL, seg = i - pl * RWL;
        const int f = seg * 64 + lane;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)plane_of(pl), 0, (unsigned)T * 16u, 0x00020000);
        if (BN % 64 == 0 || f < BN) {
            DR_CHECK_LDS(Rs + pl * BN + f, lds_off(Rs), lds_off(Rs) + 32u * BN * 16u, code);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(Rs + pl * BN + seg * 64), 16, (t0 + f) * 16, 0, 0, AUX);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The producer waves (pw = 0..3) of the LDS-staged bodies: they stage the X tile of chunks [c0, c1) of frame tile
// (b, t0) into Xs = [2 buffers][XP planes][FW frames] float4, one chunk ahead of the consumers, and first - RBN != 0,
// EPI_RES_SKIP - the block's read-modify-write tile (h rows of M tile mt below y_rows, skip rows above) into Rs.
//   Each X-tile plane row (FW float4 = frames t0-halo .. t0+BN+halo-1 of 4 channels) is copied
//   global -> LDS by ceil(FW/64) `buffer_load_dwordx4 ... lds` instructions (64 lanes x 16 B, LDS
//   destination = wave-uniform base + lane*16).  The buffer descriptor covers exactly frames
//   [0, T) of that plane, so frames outside the clip - the conv's zero padding and the tail of the
//   last tile - come back as 0 from the hardware bounds check: no VALU, no ds_write, no VGPR
//   staging.  Producers therefore issue a handful of instructions per chunk and no longer steal
//   issue slots from the consumers' MFMA stream (measured: 70.7 -> 66 ticks per MFMA when idle).
//   PREC = 1: the X tile rows are the split-bf16 planes [(sub*2 + g)*6 + piece*2 + kq] (see gemm_body).
//   PREC = 2 / 4 (one_plane16): the one-pass bf16 / f16 planes [(sub*2 + g)*2 + kq] = four consecutive plane8 units per 32
//   channels.
//   AUX = 16: sc1 loads (COH bodies: X was written by other workgroups of the same launch).
// ---------------------------------------------------------------------------------------------
template <int KS, int PREC, int AUX, int RBN>
DR_DEVINL void producer(const GemmArgs& a, float4* Xs, float4* Rs, const int pw, const int lane, const int mt, const int b, const int t0,
                        const int halo, const int FW, const int c0, const int c1, const int code_x, const int code_r) {
    constexpr int XP = x_tile_rows(PREC) * KS;            // 16-byte rows per X tile
    const int bx = a.x_bmod ? (b % a.x_bmod) : b;
    const float* Xg = a.X + (long)bx * a.x_bs;
    const int last_plane = a.x_planes - 1;
    const unsigned recs = ((unsigned)(a.T - 1) * (unsigned)a.x_fs + 4u) * 4u;   // bytes of one plane row
    const int wl = (FW + 63) >> 6;                  // wave-loads per plane row
    const int total = XP * wl;
    auto issue = [&](int chunk) {
        for (int i = pw; i < total; i += 4) {
            const int pl = i / wl, seg = i - pl * wl;
            const int f = seg * 64 + lane;
            // planes beyond Cin (K padding) re-read the last valid plane: finite data x zero weights
            const float* src;
            if constexpr (one_plane16(PREC)) {
                const int pc = min(chunk * (4 * KS) + pl, last_plane);                // plane8: rows are [(sub*2 + g)*2 + kq]
                src = Xg + (long)pc * a.x_ps;
            } else if constexpr (PREC) {
                const int sg = pl / 6, rem = pl - sg * 6, pce = rem >> 1, kq = rem & 1;
                const int pc = min(chunk * (4 * KS) + sg * 2 + kq, last_plane);       // plane8
                src = Xg + (long)pce * a.x_piece + (long)pc * a.x_ps;
            } else {
                src = Xg + (long)min(chunk * XP + pl, last_plane) * a.x_ps;
            }
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, recs, 0x00020000);
            const int voff = (t0 - halo + f) * (int)a.x_fs * 4;   // negative / past the end => reads 0
            float4* dst = Xs + (((chunk - c0) & 1) * XP + pl) * FW + seg * 64;
            if (f < FW) DR_CHECK_LDS(dst + lane, lds_off(Xs), lds_off(Xs) + 2u * XP * FW * 16u, code_x);
            if (f < FW) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)dst, 16, voff, 0, 0, AUX);
        }
    };
    if constexpr (RBN != 0) {
        auto plane_of = [&](int pl) -> const float* {
            const int row0 = mt * 128 + pl * 4;
            return (row0 < a.y_rows) ? a.Y + (long)b * a.y_bs + (long)(row0 >> 2) * a.y_ps
                                     : a.skip + (long)b * a.s_bs + (long)((row0 - a.y_rows) >> 2) * a.T * 4;
        };
        dma_tile<RBN, AUX>(Rs, plane_of, a.T, t0, pw, 4, lane, code_r);
    }
    issue(c0);
    for (int chunk = c0; chunk < c1; ++chunk) {
        // hand-over #chunk: this wave's DMA of tile #chunk must have LANDED before the barrier releases the
        // consumers - barriers do not drain VMEM, and hipcc does not reliably insert the wait for a
        // __syncthreads() behind LDS-DMA builtins (it did in the stand-alone kernels and did NOT in the fused
        // ones: tools/isa_audit.py; the consumers then read the previous occupant of the buffer whenever the tile
        // was slower than their own first weight fragments - observed with cross-XCD hand-offs).  Hence explicit.
        // The consumers' matching barrier opens their chunk; only then may the OTHER buffer be refilled (the
        // consumers finished reading it before they arrived here).
#if DR_FAULT != 1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#else                       // litmus build 1: the hand-over WITHOUT the wait - a bare s_barrier, so that hipcc's own fence
        __builtin_amdgcn_s_barrier();       // handling cannot put it back (which kernels of rounds 1-2 had it was luck)
#endif
        if (chunk + 1 < c1) issue(chunk + 1);
    }
}

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM kernel.
//   block = 512 threads = 8 waves, SPECIALISED (measured with the s_memtime hook: with one wave per
//   SIMD every non-MFMA instruction cluster in the consumer's in-order stream is exposed - X loads,
//   select/add VALU, ds_write and the barrier cost 6.7 of 74.6 ticks per MFMA - while instructions of
//   ANOTHER wave on the same SIMD overlap the 64-cycle MFMAs):
//     waves 0-3  consumers, one per SIMD, 4 (M) x 1 (N): wave tile 32 rows x 64*NI frames (for the paired
//                epilogues the 32 rows are 16 gate/cos + 16 filter/sin rows of the SAME channels, so
//                pairing is register-local).  They only issue MFMAs, the A-fragment loads and the
//                B-fragment ds_reads.
//     waves 4-7  producers: stage the X tile of the NEXT chunk with LDS-DMA (hardware zero padding)
//                while the consumers compute the current one.
//   One s_barrier per chunk hands a staged buffer over (double buffered).
//
//   A operand (weights): NEVER staged through LDS.  The packed layout is fragment-shaped, so every
//   consumer wave loads the 4 float4 A-fragments of a K step (4 channel groups x its 32 rows) straight
//   from L2 into VGPRs - buffer loads off the M tile's weight panel (resource in SGPRs, fixed per-lane
//   offset, scalar per-step offset: no vector address arithmetic), two fully coalesced 512-B segments per
//   instruction, one step ahead of use, spread through the first group's MFMAs.  The 128-row weight panel
//   of an M tile is L2-resident: blockIdx % MT pins a panel to an XCD.
//   B operand (activations): X tile [KS*8 planes][FW = BN + 2*halo frames][float4] in LDS; all taps of
//   the dilated conv read it at shifted frame offsets with conflict-free ds_read_b128.
//   K loop: for chunk (32*KS input channels) for tap for sub-chunk: 64*NI MFMAs per consumer wave.
// ---------------------------------------------------------------------------------------------
//   PREC = 1 ("S3"): the X input and the weights are split-bf16 (see above): X tile rows are
//   [(sub*2 + g)*6 + piece*2 + kq] (16 channels per group g, 8 per kq half), the consumers run 6
//   v_mfma_f32_32x32x16_bf16 per (group, row tile, frame tile) instead of 8 fp32 MFMAs per 16 channels.
//   PREC = 2 ("bf16"): the X input and the weights are piece 0 of that split alone - each value rounded once to bf16 - in one
//   plane set: X tile rows [(sub*2 + g)*2 + kq], ONE v_mfma_f32_32x32x16_bf16 per (group, row tile, frame tile) and K step;
//   the EPI_GATE output and the second output Y2 are written in the same form (store_bf16_quad).
//   PREC = 4 ("f16"): PREC = 2 with IEEE binary16 in place of bf16 - the same planes, tiles, slabs and K loop; only the
//   conversion (store_f16_quad) and the MFMA (v_mfma_f32_32x32x16_f16) differ (device_common.h: store_quad_of, mma_of).
//   COH = 1 (the fused residual-stack kernel only): the tensors this body exchanges with OTHER workgroups of the
//   same launch - its X input (hd) and its EPI_GATE output (g) - are read with sc1 loads and written with sc1
//   (write-through) stores, the placement-independent hand-off form of MI355X_MICROARCH.md "inter-workgroup
//   visibility"; everything else (weights, biases, conditioner: written before the launch) stays plain.
//
//   Accumulation order (the contraction's numerics): every 32*KS-channel chunk (x all taps: 288 terms of the k = 9
//   conv) is contracted as one k-ordered fp32 MFMA chain starting from ZERO, and the chunk sums are added up in chunk
//   order in a second set of registers ("outer") - blocked accumulation, as the CPU libraries' K-blocked GEMMs do it.
//   One 4608-term chain per output (rounds 1-3) had 3-3.9x the rounding error of the CPU fp32 reference against
//   float64 in the trained-weight regime (profiles/r03_parity_margins.txt); with 288-term blocks a CPU emulation
//   gives 2.1e-5 rms on unit-variance data against 8.3e-5 for the single chain and 2.1e-5 for torch's own matmul.
//   The fold (NW x 16 adds per chunk) sits behind the hand-over barrier, under the latency of the chunk's first
//   fragment reads; the chunk's first MFMAs take a zero C operand, so nothing is cleared.
//
//   FOLDP: blocked accumulation wanted.  It applies to the gated conv (EPI_GATE: the K = taps x C contraction; every other
//   GEMM of the path has K <= 1056 and keeps one chain, bit-identical to pw_body).  Cost, with the fold pinned behind the
//   hand-over barrier (see fold()): +0.6 % per config-3 chain on 64-frame blocks, +0.2-0.6 % per config-2 chain on 128-row x
//   128-frame blocks (208 registers with the in-place fragment refresh below) - on by default in both (engine option
//   "blocked_accumulation": 1 = 128-frame blocks keep one chain).  profiles/r04_conv_flavour_ab.txt.
template <int NI, int KS, int EPI, int PREC, int COH, int FOLDP = (NI == 1)>
DR_DEVINL void gemm_body(const GemmArgs& a, char* smem, const int mt, const int nt, const int ks) {
    // NI = 1 / 2: 64 / 128-frame blocks (2 / 4 32-frame MFMA tiles per consumer wave); NI = 3 / 5: THREE / FIVE tiles = 96 /
    // 160-frame blocks, the dilated conv only (640-frame geometries: 4 x 160-frame blocks per clip, 8 evaluations x 4 x 8 M
    // tiles = 256 blocks; ragged lengths: 96) - fp32 with blocked accumulation, in place of the 16x16-MFMA kernels of those
    // widths, which have no blocked form
    constexpr int NW = (NI == 3 || NI == 5) ? NI : 2 * NI;    // 32-frame MFMA tiles per wave
    constexpr int BN = 32 * NW;
    static_assert(NI == 1 || NI == 2 || ((NI == 3 || NI == 5) && EPI == EPI_GATE && PREC == 0 && KS == 1 && FOLDP == 1),
                  "block widths: 64, 128; 96, 160 (conv)");
    constexpr int XP = x_tile_rows(PREC) * KS;      // 16-byte rows per X tile
    // Consumer wave arrangement: 4 (M) x 1 (N) - every wave owns 32 distinct rows x all 64*NI frames of the
    // block, so no two waves issue the same A-fragment loads (a CU's vector-memory path is the stressed
    // resource: with 2 x 2 the two N-waves fetched identical fragments); the X tile is shared through LDS.
    // Paired epilogues (gate / |.|^2) find both members of a pair inside one 32-row MFMA tile: packed rows
    // of a wave are [16 gate (cos) channels, 16 filter (sin) channels], i.e. C/D register quads q and q+2
    // of the same lane.
    constexpr bool PAIRED = (EPI == EPI_GATE || EPI == EPI_POWER);
    int tid = threadIdx.x;
    // COH (the persistent kernels call this body once per phase inside a loop): everything this call derives from the lane
    // index must be computed INSIDE the call.  Without the opaque barrier the compiler hoists the per-lane address
    // arithmetic of every phase body out of the phase loop - dozens of registers that then live through the K loops of the
    // other phases (stack_kernel<2> with blocked accumulation: 256 VGPRs + 232 B of scratch before).
    if constexpr (COH) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long tick0 = a.dbg ? clock64() : 0;   // measurement hook (null in production launches)

    const int halo = ((a.taps - 1) >> 1) * a.dil;
    const int FW = BN + 2 * halo;
    float4* Xs = reinterpret_cast<float4*>(smem);   // [2 buffers][XP][FW]
    // EPI_RES_SKIP: the tile of h (residual rows) / skip (skip rows) this block read-modify-writes,
    // [32 planes][BN frames] float4, DMA'd by the producers at kernel start and read by the epilogue.
    // (Holding it in 64 prefetch VGPRs instead cost the compiler the B-fragment software pipelining.)
    float4* Rs = Xs + 2 * XP * FW;
#ifdef DR_BOUNDS
    const unsigned xs0 = lds_off(Xs), xs1 = xs0 + 2u * XP * FW * 16u, rs1 = xs1 + (EPI == EPI_RES_SKIP ? 32u * BN * 16u : 0u);
    if (tid == 0 && !COH) DR_CHECK(rs1 <= (unsigned)a.lds_bytes, 100, rs1, a.lds_bytes);      // the regions fit the launch's LDS
#endif

    // (mt, nt, ks) = this block's M tile, frame tile and K split: chosen by the caller (gemm_kernel below)
    const int tps = (a.T + BN - 1) / BN;
    const int b = nt / tps;
    const int t0 = (nt % tps) * BN;
    const int NS = a.kchunks * a.taps;              // K steps (32 channels x 1 tap each)
    const int cps = a.kchunks / KS / a.ksplit;      // chunks (hand-overs) of this block: [c0, c1)
    const int c0 = ks * cps, c1 = c0 + cps;

    if (wave >= 4) {      // producers (LDS-DMA)
        producer<KS, PREC, COH ? 16 : 0, EPI == EPI_RES_SKIP ? BN : 0>(a, Xs, Rs, wave - 4, lane, mt, b, t0, halo, FW, c0, c1, 101, 102);
        return;
    }

    // ---------------------------------------------------------------------- consumers (wave = its 32 rows of the M tile)
    const int r = lane & 31, hi = lane >> 5;
    // this lane's A fragments inside a slab: fp32 [g][hi][row][4] (16 KiB); S3 [g16][piece][kq][row][8 bf16] (24 KiB)

    f32x16 acc[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
    // blocked accumulation (see the header): acc = the running chunk's chain, outer = the sum of the finished chunks
    f32x16 outer[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) outer[ni][e] = 0.f;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr bool FOLD = FOLDP && EPI == EPI_GATE;
    auto fold = [&]() {
        if constexpr (FOLD) {
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) outer[ni] = outer[ni] + acc[ni];
            // The adds happen HERE.  Their results are only needed after the K loop, and left alone the compiler sinks
            // them to the bottom of the chunk - which keeps the previous chain alive through the whole chunk in a THIRD
            // register set (16*NW copies per chunk behind the last MFMAs; at NW = 4 also what pushed the kernel into
            // scratch).  An opaque use pins them in front of the chunk's first MFMAs, which then reuse acc's registers.
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) asm volatile("" : "+v"(outer[ni]));
        }
    };

    // Epilogue operands are NOT prefetched into VGPRs: bias / d2 / conditioner are L2-resident and are
    // loaded as unconditional batches at the start of the epilogue (a conditional load there compiles to
    // a branch + s_waitcnt vmcnt(0) per quad), the EPI_RES_SKIP read-modify-write tile waits in LDS (Rs).
    float4 eop[NW][4];

    if constexpr (one_plane16(PREC)) {
        // One-pass bf16: both operands rounded once to bf16 (piece 0 of the split), ONE v_mfma_f32_32x32x16_bf16 per
        // (group, row tile, frame tile) and K step.  A slab = 8 KiB, [g16 2][kq 2][row 128][8 bf16]; X tile rows
        // [(sub*2 + g)*2 + kq].  A K step is only 2*NW MFMAs of 32 cycles, shorter than an L2 round trip: the A fragments
        // are refreshed in place TWO steps ahead (two register sets, roles alternate statically), each load right behind
        // the MFMAs that consumed its registers; every MFMA has one B-fragment read (the wave tile is 32 rows: a
        // fragment is used once), issued one group ahead in the shadow of the previous MFMA.
        const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.Wp + (long)mt * NS * 2048), 0, (unsigned)NS * 8192u, 0x00020000);
        const int wvo = (hi * 128 + wave * 32 + r) * 16;
        auto load_ag = [&](int slab, int g) -> uint4 {
            DR_CHECK(slab >= 0 && wvo + slab * 8192 + g * 4096 + 16 <= NS * 8192, 113, slab, NS);
            return buffer_load_u4(wrsrc, wvo, slab * 8192 + g * 4096);
        };
        const int s0 = c0 * KS * a.taps;
        AF2 wA, wB;
        wA.v[0] = load_ag(s0, 0); wA.v[1] = load_ag(s0, 1);
        wB.v[0] = load_ag(min(s0 + 1, NS - 1), 0); wB.v[1] = load_ag(min(s0 + 1, NS - 1), 1);
        const int cen = (a.taps - 1) >> 1;
        const int per_chunk = a.taps * KS;
        const uint4* Xsb = reinterpret_cast<const uint4*>(Xs);
        struct BF1 { uint4 v[NW]; };              // B fragments of one 16-channel group: NW 32-frame tiles
        BF1 b0, b1;
        auto xaddr = [&](int chunk, int q) -> const uint4* {
            const int j = q / KS, sub = q - j * KS;
            return Xsb + (((chunk - c0) & 1) * XP + sub * 4 + hi) * FW + halo + (j - cen) * a.dil + r;
        };
        auto rd1 = [&](const uint4* Xb, int g) -> BF1 {
            BF1 o;
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) {
                DR_CHECK_LDS(Xb + g * 2 * FW + ni * 32, xs0, xs1, 114);
                o.v[ni] = Xb[g * 2 * FW + ni * 32];
            }
            return o;
        };
        auto mma1 = [&](auto FIRST, const uint4 af, const BF1& bf) {
            constexpr bool kFirst = FOLD && decltype(FIRST)::value;      // the chunk's first products: C = 0 (a new chain)
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_of<PREC>(af, bf.v[ni], kFirst ? zero16 : acc[ni]);
        };
        auto step = [&](auto ROLE, auto FIRST, int slab, int chunk, int q) {
            constexpr bool kB = decltype(ROLE)::value;
            const uint4* Xb = xaddr(chunk, q);
            const int nx = min(slab + 2, NS - 1);
            b1 = rd1(Xb, 1);
            mma1(FIRST, kB ? wB.v[0] : wA.v[0], b0);
            if constexpr (kB) wB.v[0] = load_ag(nx, 0);
            else wA.v[0] = load_ag(nx, 0);
            b0 = rd1(xaddr(chunk, min(q + 1, per_chunk - 1)), 0);
            mma1(std::false_type{}, kB ? wB.v[1] : wA.v[1], b1);
            if constexpr (kB) wB.v[1] = load_ag(nx, 1);
            else wA.v[1] = load_ag(nx, 1);
            sgb<0x100, 1>();
            sgb_mix1<NW - 1, 0>(); sgb<0x8, 1>(); sgb<0x20, 1>();
            sgb<0x100, 1>();
            sgb_mix1<NW - 1, 0>(); sgb<0x8, 1>(); sgb<0x20, 1>();
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        for (int chunk = c0; chunk < c1; ++chunk) {
            auto at = [&](auto R, auto FIRST, int q) {
                const int j = q / KS, sub = q - j * KS;
                step(R, FIRST, (chunk * KS + sub) * a.taps + j, chunk, q);
            };
            __syncthreads();              // X tile #chunk staged by the producers (matches their hand-over barrier)
            b0 = rd1(xaddr(chunk, 0), 0);
            fold();                       // the previous chunk's chain joins the outer sum (zeros the first time)
            at(F_{}, T_{}, 0);
            int q = 1;
            for (; q + 2 <= per_chunk; q += 2) {
                at(T_{}, F_{}, q);
                at(F_{}, F_{}, q + 1);
            }
            if (q < per_chunk) at(T_{}, F_{}, q);
            else { const AF2 t = wA; wA = wB; wB = t; }      // (an odd number of steps: the next step's fragments sit in set B)
        }
    } else if constexpr (PREC == 1) {
        // A fragments through buffer loads with scalar per-step offsets (see the fp32 path): slab = 24 KiB,
        // [g16 2][piece 3][kq 2][row 128][8 bf16]
        const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.Wp + (long)mt * NS * 6144), 0, (unsigned)NS * 24576u, 0x00020000);
        const int wvo = (hi * 128 + wave * 32 + r) * 16;
        auto load_a3 = [&](int slab) -> AF6 {
            AF6 o;
#pragma unroll
            for (int gp = 0; gp < 6; ++gp) {
                DR_CHECK(slab >= 0 && wvo + slab * 24576 + gp * 4096 + 16 <= NS * 24576, 103, slab, NS);
                o.v[gp] = buffer_load_u4(wrsrc, wvo, slab * 24576 + gp * 4096);
            }
            return o;
        };
        AF6 wA = load_a3(c0 * KS * a.taps), wB;
        const int cen = (a.taps - 1) >> 1;
        const int per_chunk = a.taps * KS;
        const uint4* Xs3 = reinterpret_cast<const uint4*>(Xs);
        // B fragments of one 16-channel group: 3 pieces x NW 32-frame tiles
        struct BF3 { uint4 v[3][NW]; };
        BF3 b0, b1;
        auto xaddr = [&](int chunk, int q) -> const uint4* {
            const int j = q / KS, sub = q - j * KS;
            return Xs3 + (((chunk - c0) & 1) * XP + sub * 12 + hi) * FW + halo + (j - cen) * a.dil + r;
        };
        auto rd3 = [&](const uint4* Xb, int g) -> BF3 {
            BF3 o;
#pragma unroll
            for (int pz = 0; pz < 3; ++pz)
#pragma unroll
                for (int ni = 0; ni < NW; ++ni) {
                    DR_CHECK_LDS(Xb + (g * 6 + pz * 2) * FW + ni * 32, xs0, xs1, 104);
                    o.v[pz][ni] = Xb[(g * 6 + pz * 2) * FW + ni * 32];
                }
            return o;
        };
        // six piece products per accumulator, smallest terms first; consecutive MFMAs go to different
        // accumulators (the pinned schedule keeps program order: no dependent back-to-back pairs)
        auto mma6 = [&](auto FIRST, const uint4 a0, const uint4 a1, const uint4 a2, const BF3& bf) {
            constexpr bool kFirst = FOLD && decltype(FIRST)::value;      // the chunk's first products: C = 0 (a new chain)
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a2, bf.v[0][ni], kFirst ? zero16 : acc[ni]);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a0, bf.v[2][ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a1, bf.v[1][ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a1, bf.v[0][ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a0, bf.v[1][ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[ni] = mma_bf16(a0, bf.v[0][ni], acc[ni]);
        };
        // One K step (32 channels x 1 tap): 2 groups x 6 piece products x NW tiles = 12*NW MFMAs per wave.
        // A 32x32x16 bf16 MFMA is 32 cycles, so a step is only 384*NW cycles: every non-MFMA instruction
        // that is not issued in the shadow of a running MFMA shows.  Pipeline (pinned): the reads of group 1
        // are interleaved 1:2 with group 0's MFMAs, the reads of the NEXT step's group 0 with group 1's;
        // only the chunk's first step reads its own group 0 (after the hand-over barrier).
        auto step = [&](auto ROLE, auto FIRST, int slab, int chunk, int q) {
            constexpr bool kB = decltype(ROLE)::value;
            const uint4* Xb = xaddr(chunk, q);
            if constexpr (kB) wA = load_a3(min(slab + 1, NS - 1));
            else wB = load_a3(min(slab + 1, NS - 1));
            b1 = rd3(Xb, 1);
            mma6(FIRST, kB ? wB.v[0] : wA.v[0], kB ? wB.v[1] : wA.v[1], kB ? wB.v[2] : wA.v[2], b0);
            b0 = rd3(xaddr(chunk, min(q + 1, per_chunk - 1)), 0);
            mma6(std::false_type{}, kB ? wB.v[3] : wA.v[3], kB ? wB.v[4] : wA.v[4], kB ? wB.v[5] : wA.v[5], b1);
            sgb_mix<3 * NW, 6>();           // + the 6 A-fragment loads of the next step, one per MFMA pair
            sgb_mix<3 * NW, 0>();
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        for (int chunk = c0; chunk < c1; ++chunk) {
            auto at = [&](auto R, auto FIRST, int q) {
                const int j = q / KS, sub = q - j * KS;
                step(R, FIRST, (chunk * KS + sub) * a.taps + j, chunk, q);
            };
            __syncthreads();
            b0 = rd3(xaddr(chunk, 0), 0);
            fold();                       // the previous chunk's chain joins the outer sum (zeros the first time)
            at(F_{}, T_{}, 0);
            int q = 1;
            for (; q + 2 <= per_chunk; q += 2) {
                at(T_{}, F_{}, q);
                at(F_{}, F_{}, q + 1);
            }
            if (q < per_chunk) at(T_{}, F_{}, q);
            else wA = wB;
        }
    } else {
    // A fragments through buffer loads: the M tile's weight panel is the resource (SGPRs), the per-lane
    // byte offset is fixed for the whole kernel and the per-step offset is scalar - no vector address
    // arithmetic in the K loop (with flat 64-bit addresses it was ~12 exposed VALU instructions per step).
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.Wp + (long)mt * NS * 4096), 0, (unsigned)NS * 16384u, 0x00020000);
    const int wvo = (hi * 128 + wave * 32 + r) * 16;
    auto load_a = [&](int slab) { return load_a4(wrsrc, wvo, slab, NS, 105); };

    AF4 wA = load_a(c0 * KS * a.taps), wB;
    const int cen = (a.taps - 1) >> 1;

    // B fragments of one 8-channel group: NW float4 (one per 32-frame MFMA tile), conflict-free ds_read_b128
    struct BF { float4 v[NW]; };
    BF b0, b1;                                   // groups 0/2 and 1/3 of the step in flight
    auto xaddr = [&](int chunk, int q) -> const float4* {     // X tile address of step q of a chunk
        const int j = q / KS, sub = q - j * KS;
        return Xs + (((chunk - c0) & 1) * XP + sub * 8 + hi) * FW + halo + (j - cen) * a.dil + r;
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    using I0 = std::integral_constant<int, 0>;
    using IN = std::integral_constant<int, NW>;
    using IA = std::integral_constant<int, (1 << NW) - 1>;       // chain-start mask: every tile
    // group g of the step at Xb, tiles [LO, HI) (I0, IN: all)   (DR_BOUNDS: one code, 106; the edge-tap steps' 115 is retired)
    auto rdx = [&](auto LO_, auto HI_, const float4* Xb, int g, BF& o) {
#pragma unroll
        for (int ni = decltype(LO_)::value; ni < decltype(HI_)::value; ++ni) {
            DR_CHECK_LDS(Xb + g * 2 * FW + ni * 32, xs0, xs1, 106);
            o.v[ni] = Xb[g * 2 * FW + ni * 32];
        }
    };
    // mma_f32x4 on every tile; FIRST = the chunk's first MFMAs, which start a new chain where the accumulation is blocked (FOLD)
    auto mma4 = [&](auto FIRST, const float4 af, const BF& bf) {
        constexpr bool kFirst = FOLD && decltype(FIRST)::value;
        mma_f32x4<kFirst ? (1 << NW) - 1 : 0, 0, NW>(acc, af, bf.v);
    };

    // One K step (32 channels x 1 tap): 16*NW MFMAs per wave in 4 groups of 8 channels.  Software pipeline,
    // pinned with sched_group_barrier: the fragment reads of group g+1 are issued before group g's MFMAs,
    // and the reads of the NEXT step's group 0 before this step's group 3 - so inside a chunk no MFMA ever
    // waits for LDS; only the chunk's first step reads its own group 0, right after the hand-over barrier
    // (the last step of a chunk prefetches a valid but unused address: the next tile is not staged yet).
    // ROLE (compile time) selects which of the two A-fragment register sets is consumed; the other receives
    // the next step's fragments (prefetch distance one step), requested at the top of the step.  Roles
    // alternate statically: no per-step register copies.
    const int per_chunk = a.taps * KS;
    auto step = [&](auto ROLE, auto FIRST, int slab, int chunk, int q) {
        constexpr bool kB = decltype(ROLE)::value;
        const float4* Xb = xaddr(chunk, q);
        if constexpr (kB) wA = load_a(min(slab + 1, NS - 1));
        else wB = load_a(min(slab + 1, NS - 1));
        rdx(I0{}, IN{}, Xb, 1, b1);
        mma4(FIRST, kB ? wB.v[0] : wA.v[0], b0);
        rdx(I0{}, IN{}, Xb, 2, b0);
        mma4(std::false_type{}, kB ? wB.v[1] : wA.v[1], b1);
        rdx(I0{}, IN{}, Xb, 3, b1);
        mma4(std::false_type{}, kB ? wB.v[2] : wA.v[2], b0);
        rdx(I0{}, IN{}, xaddr(chunk, min(q + 1, per_chunk - 1)), 0, b0);
        mma4(std::false_type{}, kB ? wB.v[3] : wA.v[3], b1);
        // pinned schedule: the 4 A-fragment loads ride inside group 0's MFMAs (one per NW MFMAs: issued in the
        // shadow of a running MFMA instead of as a burst with the matrix pipe idle; hipcc on its own sinks them
        // to their first use and exposes the whole L2 latency once per step)
        sgb<0x100, NW>(); sgb_spread<4, NW>();
        sgb<0x100, NW>(); sgb<0x8, 4 * NW>();
        sgb<0x100, NW>(); sgb<0x8, 4 * NW>();
        sgb<0x100, NW>(); sgb<0x8, 4 * NW>();
    };
    // 128-frame blocks (NI = 2) refresh the A fragments IN PLACE instead: group g's fragment register quad receives the
    // next step's group g right behind the group's last MFMA (one buffer load per group: prefetch distance three
    // groups = 48 MFMAs) - ONE fragment set instead of two, which is what lets the second accumulator set of the
    // blocked accumulation (64 registers at NW = 4) live in the K loop without spilling; no roles, no per-chunk copy.
    // That step is stepx below on every tile: stepx(IA, I0, IN) starts the chunk's chains (C = 0), stepx(I0, I0, IN) goes on.
    constexpr bool AINP = (NI == 2 || NI == 5) && FOLD;
    auto load_ag = [&](int slab, int g) -> float4 {
        DR_CHECK(slab >= 0 && wvo + slab * 16384 + g * 4096 + 16 <= NS * 16384, 112, slab, NS);
        return buffer_load_f4(wrsrc, wvo, slab * 16384 + g * 4096);
    };
    // Edge taps (zero_taps.h; option "zero_taps", fp32 128-frame blocks with blocked accumulation only - ZT): where the dilation
    // is a whole MFMA tile (d = 8 at k = 9: the outer taps sit at -+32 frames), tap 0 of the block's first tile and the last
    // tap of its last tile read nothing but zero padding, and their 16 MFMAs each add w * (+0) to a chain that starts from +0.
    // stepx is the in-place step on the tiles [LO, HI) alone - FM: the tiles whose chain starts (C = 0) in this step - with the
    // sched groups scaled to HI - LO tiles; the prefetch of the next step's group 0 stays NW wide.  The K loop is pure MFMA issue,
    // so the MFMAs left out are cycles left out: 2 of 36 tile-taps of a chunk.  One tap per edge (the kernel clamps edge_taps
    // to 1): the general form - counts, loops over them - spills in the merged kernel (256 VGPRs + 92 B of scratch; this one
    // 224 and none), and so does either form at NW = 5.  Bit-identical; resources and timing: profiles/zero_taps_ab.txt.
    constexpr bool ZT = NI == 2 && FOLD && EPI == EPI_GATE && KS == 1 && PREC == 0;
    auto stepx = [&](auto FM_, auto LO_, auto HI_, int slab, int chunk, int q) {
        constexpr int FM = decltype(FM_)::value, LO = decltype(LO_)::value, HI = decltype(HI_)::value, NX = HI - LO;
        const float4* Xb = xaddr(chunk, q);
        const int nx = min(slab + 1, NS - 1);
        rdx(LO_, HI_, Xb, 1, b1);
        mma_f32x4<FM, LO, HI>(acc, wA.v[0], b0.v);
        wA.v[0] = load_ag(nx, 0);
        rdx(LO_, HI_, Xb, 2, b0);
        mma_f32x4<0, LO, HI>(acc, wA.v[1], b1.v);
        wA.v[1] = load_ag(nx, 1);
        rdx(LO_, HI_, Xb, 3, b1);
        mma_f32x4<0, LO, HI>(acc, wA.v[2], b0.v);
        wA.v[2] = load_ag(nx, 2);
        rdx(I0{}, IN{}, xaddr(chunk, min(q + 1, per_chunk - 1)), 0, b0);
        mma_f32x4<0, LO, HI>(acc, wA.v[3], b1.v);
        wA.v[3] = load_ag(nx, 3);
        sgb<0x100, NX>(); sgb<0x8, 4 * NX>(); sgb<0x20, 1>();
        sgb<0x100, NX>(); sgb<0x8, 4 * NX>(); sgb<0x20, 1>();
        sgb<0x100, NX>(); sgb<0x8, 4 * NX>(); sgb<0x20, 1>();
        sgb<0x100, NW>(); sgb<0x8, 4 * NX>(); sgb<0x20, 1>();
    };
    bool zlo = false, zhi = false;              // block-uniform: one leading / trailing tap of this block is left out
    if constexpr (ZT) {
        if (a.zero_taps) {
            const EdgeTaps et = edge_taps(a.T, t0, a.dil, a.taps, NW);
            zlo = __builtin_amdgcn_readfirstlane(et.nlo) > 0;
            zhi = __builtin_amdgcn_readfirstlane(et.nhi) > 0;
        }
    }

    // The edge-tap K loop (ZT only; a generic lambda: no other instantiation compiles it), one copy per combination of edges.
    // The WHOLE loop is specialised, not a chunk or a step: where the variants of a step meet again inside the loop the
    // compiler reconciles their register assignments with copies of the A fragments just requested - a wait for the L2 per
    // chunk, measured at +0.6 % per chain - while separate loops meet once, behind the last chunk.
    auto edge_loop = [&](auto ZLO_, auto ZHI_) {
        constexpr bool ZLO = decltype(ZLO_)::value, ZHI = decltype(ZHI_)::value;
        using I1 = std::integral_constant<int, 1>;
        using IM = std::integral_constant<int, NW - 1>;
        using FA = std::integral_constant<int, (1 << NW) - 2>;
        for (int chunk = c0; chunk < c1; ++chunk) {
            auto slab_of = [&](int q) { return chunk * a.taps + q; };      // (KS == 1)
            __syncthreads();   // as below: the hand-over, the chunk mark, group 0 of step 0, the fold, the fence
            if (a.dbg && blockIdx.x == 0 && tid == 0 && chunk < 14) a.dbg[2 + chunk] = clock64() - tick0;
            rdx(I0{}, IN{}, xaddr(chunk, 0), 0, b0);
            fold();
            __builtin_amdgcn_sched_barrier(0);
            const int qe = per_chunk - (ZHI ? 1 : 0);
            int q = 1;
            if constexpr (ZLO) {
                stepx(FA{}, I1{}, IN{}, slab_of(0), chunk, 0);      // tiles 1 .. NW-1 start their chains; tile 0 has nothing yet
                __builtin_amdgcn_sched_barrier(0);
                stepx(I1{}, I0{}, IN{}, slab_of(1), chunk, 1);      // ... and starts here
                __builtin_amdgcn_sched_barrier(0);
                q = 2;
            } else {
                stepx(IA{}, I0{}, IN{}, slab_of(0), chunk, 0);
            }
            for (; q + 2 <= qe; q += 2) {
                stepx(I0{}, I0{}, IN{}, slab_of(q), chunk, q);
                stepx(I0{}, I0{}, IN{}, slab_of(q + 1), chunk, q + 1);
            }
            if (q < qe) { stepx(I0{}, I0{}, IN{}, slab_of(q), chunk, q); ++q; }
            if constexpr (ZHI) {
                __builtin_amdgcn_sched_barrier(0);
                stepx(I0{}, I0{}, IM{}, slab_of(q), chunk, q);      // the last tap: tiles 0 .. NW-2
            }
        }
    };
    bool edge = false;          // the edge-tap loop ran in place of the one below (ZT only: everywhere else a constant)
    if constexpr (ZT) {
        if (zlo || zhi) {
            if (zlo && zhi) edge_loop(T_{}, T_{});
            else if (zlo) edge_loop(T_{}, F_{});
            else edge_loop(F_{}, T_{});
            edge = true;
        }
    }

    // Steps of a chunk, q = 0 .. per_chunk-1, in memory order of the slabs ([32-channel kchunk][tap]):
    // tap-major, sub-chunk minor.  Roles alternate A,B,A,...; a chunk always starts in role A (one
    // register copy per chunk when per_chunk is odd).
    if (!edge)
    for (int chunk = c0; chunk < c1; ++chunk) {
        auto slab_of = [&](int q) {
            const int j = q / KS, sub = q - j * KS;
            return (chunk * KS + sub) * a.taps + j;
        };
        auto at = [&](auto R, auto FIRST, int q) { step(R, FIRST, slab_of(q), chunk, q); };
        __syncthreads();   // X tile #chunk staged by the producers (matches their hand-over barrier)
        if (a.dbg && blockIdx.x == 0 && tid == 0 && chunk < 14) a.dbg[2 + chunk] = clock64() - tick0;
        rdx(I0{}, IN{}, xaddr(chunk, 0), 0, b0);
        fold();                           // the previous chunk's chain joins the outer sum (zeros the first time)
        // (the first step's pinned schedule starts HERE: without the fence its first sched group adopts the reads of b0
        // above, and every fragment read of the step is issued one group late - right in front of the MFMAs that wait for it)
        if constexpr (FOLD) __builtin_amdgcn_sched_barrier(0);
        if constexpr (AINP) {
            stepx(IA{}, I0{}, IN{}, slab_of(0), chunk, 0);      // C = 0: a new chain
            int q = 1;
            for (; q + 2 <= per_chunk; q += 2) {
                stepx(I0{}, I0{}, IN{}, slab_of(q), chunk, q);
                stepx(I0{}, I0{}, IN{}, slab_of(q + 1), chunk, q + 1);
            }
            if (q < per_chunk) stepx(I0{}, I0{}, IN{}, slab_of(q), chunk, q);
        } else {
            at(F_{}, T_{}, 0);                // C = 0: a new chain
            int q = 1;
            for (; q + 2 <= per_chunk; q += 2) {
                at(T_{}, F_{}, q);
                at(F_{}, F_{}, q + 1);
            }
            if (q < per_chunk) at(T_{}, F_{}, q);
            else wA = wB;                     // (an odd number of steps ends in role A: the next fragments sit in set B.
                                              // Swapping the roles across chunks instead - two copies of the chunk body -
                                              // was measured: 505 vs 483 ms per config-3 chain, spills at 128 frames)
        }
    }

    }
    // the last chunk's chain; from here on acc holds the block's (partial) sums
    if constexpr (FOLD) {
#pragma unroll
        for (int ni = 0; ni < NW; ++ni) acc[ni] = outer[ni] + acc[ni];
    }

    const long long tick1 = a.dbg ? clock64() : 0;
    // ----------------------------------------------------------------------------------------
    // split-K reduction, per consumer wave (no block-level synchronisation): every wave parks its partial
    // accumulators in the workspace (fragment order: 1 KiB per store instruction), then takes a ticket on
    // the counter of its (tile, wave) region.  The wave that draws the last ticket re-reads ALL ksplit
    // partials in split order - so the sum does not depend on arrival order: results are deterministic -
    // and runs the epilogue; the others are done.  It also re-arms the counter for the next launch.
    // The XCDs' L2s are not coherent with each other, so the partials travel with agent-coherent cache
    // policy (sc0 sc1: write-through stores, L2-bypassing loads) and the ordering is
    // stores -> s_waitcnt vmcnt(0) -> ticket (agent-scope atomic) -> loads; a full __threadfence() here
    // costs an L2-wide write-back + invalidate per wave (measured: 25 us per launch).
    // ----------------------------------------------------------------------------------------
    if (a.ksplit > 1) {
        constexpr int WQ = NW * 4;                                   // float4 per lane per wave region
        constexpr int WSCOH = 17;                                    // buffer cache policy: sc0 | sc1
        const int tile = nt * a.MT + mt;
        const __amdgpu_buffer_rsrc_t wsr =
            __builtin_amdgcn_make_buffer_rsrc((void*)a.ws, 0, (unsigned)(a.ws_floats * 4), 0x00020000);
        const int sstride = 4 * WQ * 64 * 16;                        // bytes between consecutive splits
        const int base = ((tile * a.ksplit * 4 + wave) * (WQ * 64) + lane) * 16;
#pragma unroll
        for (int ni = 0; ni < NW; ++ni)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 v = {__float_as_uint(acc[ni][4 * q]), __float_as_uint(acc[ni][4 * q + 1]),
                                 __float_as_uint(acc[ni][4 * q + 2]), __float_as_uint(acc[ni][4 * q + 3])};
                DR_CHECK((size_t)(base + ks * sstride + (ni * 4 + q) * 1024) + 16 <= a.ws_floats * 4, 107, base + ks * sstride, a.ws_floats);
                __builtin_amdgcn_raw_buffer_store_b128(v, wsr, base + ks * sstride + (ni * 4 + q) * 1024, 0, WSCOH);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // partials are out before the ticket is drawn
        unsigned ticket = 0;
        DR_CHECK((size_t)(tile * 4 + wave) < a.ws_cnt_n, 108, tile * 4 + wave, a.ws_cnt_n);
        if (lane == 0) ticket = __hip_atomic_fetch_add(a.ws_cnt + tile * 4 + wave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket != (unsigned)(a.ksplit - 1)) return;
        if (lane == 0) __hip_atomic_store(a.ws_cnt + tile * 4 + wave, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int ni = 0; ni < NW; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
        // U splits in flight per wait (the loads are pure latency: ~1.5 us each when taken one by one);
        // the adds stay in split order whatever U is
        auto reduce = [&](auto UU, int sp0) {
            constexpr int U = decltype(UU)::value;
            u32x4 v[U][WQ];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < WQ; ++i) {
                    DR_CHECK((size_t)(base + (sp0 + u) * sstride + i * 1024) + 16 <= a.ws_floats * 4, 109, base + (sp0 + u) * sstride, a.ws_floats);
                    v[u][i] = __builtin_amdgcn_raw_buffer_load_b128(wsr, base + (sp0 + u) * sstride + i * 1024, 0, WSCOH);
                }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int ni = 0; ni < NW; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[ni][4 * q + e] += __uint_as_float(v[u][ni * 4 + q][e]);
        };
        constexpr int UMAX = (NW == 2) ? 4 : 2;
        if (a.ksplit % UMAX == 0) {
            for (int sp = 0; sp < a.ksplit; sp += UMAX) reduce(std::integral_constant<int, UMAX>{}, sp);
        } else {
            for (int sp = 0; sp < a.ksplit; sp += 2) reduce(std::integral_constant<int, 2>{}, sp);
        }
    }
    // ----------------------------------------------------------------------------------------
    // epilogue.  C/D fragment of 32x32: column = lane&31 (frame), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    // => per register quad q a lane owns 4 consecutive rows 8q+4hi..+3 = one float4 of the P4 layout.
    // ----------------------------------------------------------------------------------------
    // Dual-output mode (EPI_GATE, a.dual = B > 0): classifier-free guidance feeds the SAME x_t to the conditional
    // and the unconditional evaluation, so in the first residual layer the dilated conv of sample b and of
    // sample b + B is the same contraction - it is done once, and the epilogue runs twice (conditioner of
    // sample b / constant unconditional bias) writing both samples' gated outputs.
    const int npass = (EPI == EPI_GATE && a.dual > 0) ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        const int be = b + pass * a.dual;
        // conditioner tensor of this (tile, sample), frame 0: the sample's clip (cond_row), or for samples >= n_cond the
        // shared learned unconditional conditioner (condition='trainable_spec') when there is one, else clip 0's tensor
        // as a readable dummy
        const float* cbase = nullptr;
        if constexpr (EPI == EPI_GATE)
            cbase = (be < a.n_cond || !a.cond2) ? a.cond + (be < a.n_cond ? cond_row(a, be) : 0L) * a.c_bs : a.cond2;
        float4 ebias[4];                            // [q]
        float4 ed2[4];                              // second-output offset (step embedding of the next conv)
        {
            const float* bsrc = a.bias;
            if constexpr (EPI == EPI_GATE) bsrc = (be < a.n_cond) ? a.bias : a.bias2;
    #pragma unroll
            for (int q = 0; q < 4; ++q) ebias[q] = *reinterpret_cast<const float4*>(bsrc + mt * 128 + wave * 32 + 8 * q + 4 * hi);
            if constexpr (EPI == EPI_RELU || EPI == EPI_RES_SKIP) {
    #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // residual rows only exist below y_rows; the clamp keeps the (unused) skip-row loads in range
                    const int p0 = min(mt * 128 + wave * 32 + 8 * q + 4 * hi, a.y_rows - 4);
                    ed2[q] = *reinterpret_cast<const float4*>(a.d2 + (a.tsel ? (long)a.tsel[be] * a.d2_ts : 0) + p0);
                }
            }
        }
    #pragma unroll
        for (int ni = 0; ni < NW; ++ni) {
            const int t = t0 + ni * 32 + r;
            if constexpr (EPI == EPI_RES_SKIP) {
    #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    DR_CHECK_LDS(Rs + (wave * 8 + 2 * q + hi) * BN + ni * 32 + r, xs1, rs1, 110);
                    eop[ni][q] = Rs[(wave * 8 + 2 * q + hi) * BN + ni * 32 + r];
                }
            }
            if constexpr (EPI == EPI_GATE) {
                // conditioner quads of this frame column: one unconditional batch (unconditional samples read
                // sample 0's tensor - valid memory - and ignore it)
                const int tc = min(t, a.T - 1);
                const float* cb = cbase + (long)tc * 4;
    #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p0 = mt * 128 + wave * 32 + 8 * q + 4 * hi;
                    eop[ni][q] = *reinterpret_cast<const float4*>(cb + (long)(p0 >> 2) * a.T * 4);
                }
            }
            if (t >= a.T) continue;
    #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rq = 8 * q + 4 * hi;   // row offset inside the wave's 32-row MFMA tile
                if constexpr (PAIRED) {
                    if (q >= 2) continue;                     // quads 0,1 = gate / cos rows, quads 2,3 = their partners
                    const int c0 = mt * 64 + wave * 16 + rq;  // output channel of the quad (rq = 8q + 4hi < 16)
                    if (c0 >= a.y_rows) continue;
                    float v0[4], v1[4], o[4];
    #pragma unroll
                    for (int e = 0; e < 4; ++e) { v0[e] = acc[ni][4 * q + e]; v1[e] = acc[ni][4 * (q + 2) + e]; }
                    if constexpr (EPI == EPI_GATE) {
                        gate_quad(v0, v1, ebias[q], ebias[q + 2], eop[ni][q], eop[ni][q + 2], be < a.n_cond || a.cond2 != nullptr, o);
                    } else {
    #pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = v0[e] * v0[e] + v1[e] * v1[e];
                    }
                    if constexpr (one_plane16(PREC)) {   // g for the one-pass bf16 / f16 1x1 kernel
                        store_quad_of<PREC, COH>(a.Y + (long)be * a.y_bs, o, c0, t, a.T, a.wt_store);
                    } else if (a.out_s3 & 1) {   // g for the split-bf16 1x1 kernel
                        store_s3_quad<COH>(a.Y + (long)be * a.y_bs, o, c0, t, a.T, a.y_rows >> 3, a.wt_store);
                    } else {
                        float* dst = y_quad_ptr(a, be, c0, t);
                        store_f4<COH>(dst, make_float4(o[0], o[1], o[2], o[3]), a.wt_store);
                    }
                } else {
                    const int p0 = mt * 128 + wave * 32 + rq;
                    float v[4], o[4];
    #pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[ni][4 * q + e];
                    if constexpr (EPI == EPI_RES_SKIP) {
                        // packed rows [0, y_rows) are the residual half, [y_rows, 2*y_rows) the skip half
                        // (y_rows is a multiple of 64, so the branch is wave-uniform)
                        if (p0 < a.y_rows) {   // h, in place
                            float* dst = y_quad_ptr(a, be, p0, t);
                            residual_quad(v, ebias[q], eop[ni][q], o);
                            store_quad(dst, o);
                            if (a.Y2) store_y2<COH, 0, one_plane16(PREC) ? PREC : 0>(a, be, o, ed2[q], p0, t);
                        } else {
                            float* dst = skip_quad_ptr(a, be, p0, t);
                            skip_quad(v, ebias[q], eop[ni][q], a.skip_init, o);
                            store_quad(dst, o);
                        }
                    } else {
                        if (p0 >= a.y_rows) continue;
                        float bb[4];
                        f4arr(ebias[q], bb);
    #pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if constexpr (EPI == EPI_PLAIN) o[e] = a.alpha * v[e] + bb[e];
                            else if constexpr (EPI == EPI_RELU) o[e] = fmaxf(a.alpha * v[e] + bb[e], 0.f);
                            else if constexpr (EPI == EPI_SILU) { const float z = v[e] + bb[e]; o[e] = z * sigmoidf_(z); }
                            else o[e] = logf(v[e] + 1e-6f);
                        }
                        store_quad(y_quad_ptr(a, be, p0, t), o);
                        if constexpr (EPI == EPI_RELU) {
                            if (a.Y2) store_y2<COH, 0>(a, be, o, ed2[q], p0, t);    // hd = h + d_0 for the first dilated conv
                        }
                    }
                }
            }
        }
    }
    if (a.dbg && blockIdx.x == 0 && tid == 0) {
        a.dbg[0] = tick1 - tick0;           // main loop
        a.dbg[1] = clock64() - tick0;       // whole block
    }
}

// ---------------------------------------------------------------------------------------------
// Pointwise (1x1) GEMM with BOTH operands straight from L2: the 1x1 output projection + residual / skip
// update (model/diffwave.py:149-151, :680).  A 1x1 GEMM has no tap reuse, so staging X through LDS buys
// nothing - and costs a hand-over barrier per chunk plus the LDS-DMA traffic, during which the consumers of
// gemm_kernel were measured to run ~30 % slower (87 vs 66.7 ticks per MFMA).  Here a block is just four
// consumer waves, 4 (M) x 1 (N), wave tile 32 rows x 32*NW frames: per 32-channel K step a wave loads its
// 4 A fragments (packed weights, fragment order) and 4*NW B fragments (P4 activations: one float4 = the 4
// K values of a lane for 4 consecutive MFMAs) one step ahead into the alternate register set, then
// issues 16*NW MFMAs.  No LDS, no barriers, no producers.  Frames beyond T are clamped (their columns are
// never written).
// ---------------------------------------------------------------------------------------------
//   COH = 1 (fused residual-stack kernel): the second output Y2 (hd, read by other workgroups of the same launch)
//   is stored write-through (sc1) unless a.wt_store == 0; X (g, written by other workgroups) is read with plain
//   loads AFTER an agent-scope acquire in the preceding group barrier; the read-modify-write tiles h and skip
//   belong to this workgroup alone for the whole launch.
//   Run by waves 0-3 of the block (wave = wave index); mt / nt = M tile and frame tile.
//   RLDS = 1 (fused kernel; Rs = the tile): the block's read-modify-write tile (its 128 rows of h / skip x BN frames,
//   [32 planes][BN] float4) is RESIDENT IN LDS for the whole launch instead of being re-read from and re-written
//   to global memory by every layer: the epilogue reads and updates it there (no operand registers are held
//   across the last K steps - with them the fused kernel spilled), only hd goes to global.
//   TBN / foff (fused kernel, 160-frame tiles): the block's frame tile is TBN frames wide and this call covers its
//   32*NW frames starting at foff - the 160-frame 1x1 runs as a 96-frame and a 64-frame pass, because one pass
//   with 5 frame tiles per wave does not fit the fused kernel's register budget without spilling in the K loop.
//   EPI (default EPI_RES_SKIP; the tail kernel also runs EPI_RELU / EPI_PLAIN): the plain epilogues y = [relu](alpha acc
//   + bias) of the skip / output projection (model/diffwave.py:682-685) with the output strides of GemmArgs (the
//   output projection writes the (B, T, 88) roll layout); their output is stored write-through under COH.
template <int NW, int COH, int RLDS, int TBN = 32 * NW, int EPI = EPI_RES_SKIP>     // 32-frame MFMA tiles per wave: 128 rows x 32*NW frames per call
DR_DEVINL void pw_body(const GemmArgs& a, const int mt, const int nt, const int wave, float4* Rs = nullptr, const int foff = 0) {
    static_assert(EPI == EPI_RES_SKIP || EPI == EPI_RELU || EPI == EPI_PLAIN, "pw_body epilogues");
    static_assert(EPI == EPI_RES_SKIP || !RLDS, "the LDS-resident tile belongs to the residual / skip epilogue");
    constexpr int BN = TBN;
    int lane = threadIdx.x & 63;
    if constexpr (COH) asm volatile("" : "+v"(lane));      // (as gemm_body: no per-lane value of this call may be hoisted out of a phase loop)
    const int r = lane & 31, hi = lane >> 5;
    const long long tick0 = a.dbg ? clock64() : 0;

    const int tps = (a.T + BN - 1) / BN;
    const int b = nt / tps;
    const int t0 = (nt % tps) * BN + foff;
    const int NS = a.kchunks;

    // Both operands through buffer loads: resource = (this M tile's weight panel | this sample's X tensor) in
    // SGPRs, per-lane byte offset fixed for the whole kernel (1 + NW VGPRs), per-step offset scalar - so a
    // K step costs no vector address arithmetic (flat 64-bit addressing cost ~70 VALU ops per step, i.e.
    // ~12 of 76 ticks per MFMA, all exposed: nothing else runs on the SIMD).  Out-of-range reads (K padding
    // planes) return 0 from the bounds check; frames past T read the next plane's data (finite, never used).
    // X loads are PLAIN also in the fused kernel: the four waves of a block read the same B fragments, and only
    // the CU's L1 turns that into one L2 request instead of four (measured: with L1-bypassing sc1 loads the phase
    // ran 2x slower) - the fused kernel therefore invalidates the L1 once, in the barrier before this phase.
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.Wp + (long)mt * NS * 4096), 0, (unsigned)NS * 16384u, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.X + (long)b * a.x_bs), 0, (unsigned)(a.x_planes * a.x_ps * 4), 0x00020000);
    const int wvo = (hi * 128 + wave * 32 + r) * 16;
    const int xps = (int)a.x_ps * 4;                          // bytes per plane
    int xvo[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni) xvo[ni] = hi * xps + min(t0 + ni * 32 + r, a.T - 1) * 16;
    using BF = BF4<NW>;
    auto load_a = [&](int slab) { return load_a4(wr, wvo, slab, NS, 120); };
    auto load_b = [&](int slab) { return load_b4(xr, xvo, xps, slab); };

    f32x16 acc[NW];
#pragma unroll
    for (int ni = 0; ni < NW; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;

    AF4 aA = load_a(0), aB;
    BF bA = load_b(0), bB;
    auto step = [&](auto ROLE, int slab) {
        constexpr bool kB = decltype(ROLE)::value;
        const int nxt = min(slab + 1, NS - 1);
        if constexpr (kB) { aA = load_a(nxt); bA = load_b(nxt); }
        else { aB = load_a(nxt); bB = load_b(nxt); }
#pragma unroll
        for (int g = 0; g < 4; ++g) mma_f32x4<0, 0, NW>(acc, kB ? aB.v[g] : aA.v[g], (kB ? bB : bA).v[g]);
        // pinned schedule: the 4 + 4*NW prefetch loads are spread through the MFMA stream (one per PER MFMAs),
        // so each is issued in the shadow of a running MFMA; issued as one burst at the top of the step they
        // cost 16 TA cycles each with the matrix pipe idle (71.8 vs 67.6 ticks per MFMA)
        constexpr int NLD = 4 + 4 * NW, PER = (16 * NW) / NLD;
        sgb_spread<NLD, PER>();
        sgb<0x8, 16 * NW - NLD * PER>();
    };
    // epilogue operands (EPI_RES_SKIP): rows [0, y_rows) h = (h + acc + b) / sqrt(2) in place (+ hd = h + d_next),
    // rows [y_rows, 2 y_rows) skip (+)= acc + b.  The read-modify-write tile comes straight from global and is
    // requested BEFORE the last two K steps, so its latency hides behind their MFMAs.
    const int rowb = mt * 128 + wave * 32 + 4 * hi;           // + 8q
    const bool res_rows = rowb < a.y_rows;                     // wave-uniform (y_rows is a multiple of 64)
    float4 ebias[4], ed2[4], eop[RLDS ? 1 : NW][4];
    auto load_epilogue = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ebias[q] = *reinterpret_cast<const float4*>(a.bias + rowb + 8 * q);
            if constexpr (EPI == EPI_RES_SKIP)
                ed2[q] = *reinterpret_cast<const float4*>(a.d2 + (a.tsel ? (long)a.tsel[b] * a.d2_ts : 0) + min(rowb + 8 * q, a.y_rows - 4));
        }
        if constexpr (RLDS || EPI != EPI_RES_SKIP) return;              // the tile waits in LDS / there is none
        const float* base = res_rows ? a.Y + (long)b * a.y_bs + (long)(rowb >> 2) * a.y_ps
                                     : a.skip + (long)b * a.s_bs + (long)((rowb - a.y_rows) >> 2) * a.T * 4;
        const long qs = res_rows ? 2 * a.y_ps : (long)2 * a.T * 4;      // 8 rows = 2 planes further
        const long fs = res_rows ? a.y_fs : 4;
#pragma unroll
        for (int ni = 0; ni < NW; ++ni) {
            const int tc = min(t0 + ni * 32 + r, a.T - 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) eop[ni][q] = *reinterpret_cast<const float4*>(base + q * qs + tc * fs);
        }
    };
    int slab = 0;
    const int pre = max(NS - 2, 0) & ~1;                      // even number of steps before the prefetch point
    for (; slab < pre; slab += 2) {
        step(std::false_type{}, slab);
        step(std::true_type{}, slab + 1);
        if (a.dbg && slab == 0 && blockIdx.x == 0 && threadIdx.x == 0) a.dbg[2] = clock64() - tick0;   // first two steps done
    }
    if (a.dbg && blockIdx.x == 0 && threadIdx.x == 0) a.dbg[3] = clock64() - tick0;                    // before the RMW-tile request
    // (RLDS: only the bias / step-embedding rows are left to load - 8 L2-hot float4 per lane, requested after the
    // loop: holding them across the last K steps is what pushed the fused kernel over its register budget)
    if constexpr (!RLDS) load_epilogue();
    __builtin_amdgcn_sched_barrier(0);
    for (; slab + 2 <= NS; slab += 2) {
        step(std::false_type{}, slab);
        step(std::true_type{}, slab + 1);
    }
    if (slab < NS) step(std::false_type{}, slab);
    const long long tick1 = a.dbg ? clock64() : 0;
    if constexpr (RLDS) load_epilogue();

#pragma unroll
    for (int ni = 0; ni < NW; ++ni) {
        const int t = t0 + ni * 32 + r;
        if (t >= a.T) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p0 = rowb + 8 * q;
            float v[4], o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[ni][4 * q + e];
            if constexpr (EPI != EPI_RES_SKIP) {
                if (p0 >= a.y_rows) continue;
                float bb[4];
                f4arr(ebias[q], bb);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = a.alpha * v[e] + bb[e];
                    if constexpr (EPI == EPI_RELU) o[e] = fmaxf(o[e], 0.f);
                }
                float* dst = y_quad_ptr(a, b, p0, t);
                store_f4<COH>(dst, make_float4(o[0], o[1], o[2], o[3]), a.wt_store);
                continue;
            }
            float4* rs = nullptr;                                                   // this quad in the LDS tile (RLDS)
            if constexpr (RLDS) rs = Rs + (wave * 8 + 2 * q + hi) * BN + foff + ni * 32 + r;
#ifdef DR_BOUNDS
            if constexpr (RLDS) DR_CHECK_LDS(rs, lds_off(Rs), lds_off(Rs) + 32u * BN * 16u, 121);
#endif
            float4 pv;
            if constexpr (RLDS) pv = *rs;
            else pv = eop[ni][q];
            if (res_rows) {
                float* dst = a.Y + (long)b * a.y_bs + (long)(p0 >> 2) * a.y_ps + (long)t * a.y_fs;       // (= y_quad_ptr; spelled out: profiles/kstep_once_isa.txt)
                residual_quad(v, ebias[q], pv, o);
                if constexpr (RLDS) *rs = make_float4(o[0], o[1], o[2], o[3]);
                else store_quad(dst, o);
                if (a.Y2) store_y2<0, COH>(a, b, o, ed2[q], p0, t);
            } else {
                float* dst = skip_quad_ptr(a, b, p0, t);
                skip_quad(v, ebias[q], pv, a.skip_init, o);
                if constexpr (RLDS) *rs = make_float4(o[0], o[1], o[2], o[3]);
                else store_quad(dst, o);
            }
        }
    }
    if (a.dbg && blockIdx.x == 0 && threadIdx.x == 0) {
        a.dbg[0] = tick1 - tick0;
        a.dbg[1] = clock64() - tick0;
    }
}

// ---------------------------------------------------------------------------------------------
// Flexible-width variant on v_mfma_f32_16x16x4_f32 (exact fp32, 32-cycle issue): 16-frame column tiles,
// so a block covers BN = 32*NJ frames (96, 160).  Used when 64/128-frame tiles
// quantise badly over the 256 CUs (config 5: 8 x 640 frames -> 4 x 160-frame tiles per clip = exactly
// 256 blocks instead of 2.5 rounds of 64-frame blocks).  Same packed weights (the slab is
// [channel/4][row][4], which serves both MFMA shapes), same LDS-DMA producers, same P4 layouts.
//   consumers 4 (M) x 1 (N): wave tile = 2 row tiles (paired epilogue: gate 16 / filter 16 of the same
//   channels) x 2*NJ column tiles = 20 accumulators x 4 registers at NJ = 5.
// ---------------------------------------------------------------------------------------------
template <int NJ, int KS, int EPI>
DR_DEVINL void gemm16_body(const GemmArgs& a, char* smem, const int mt, const int nt) {
    static_assert(EPI == EPI_GATE || EPI == EPI_RES_SKIP, "16x16 variant: hot kernels only");
    constexpr int BN = 32 * NJ;
    constexpr int XP = 8 * KS;
    // 4 (M) x 1 (N) consumers, as in gemm_kernel: wave = its 32 rows of the M tile
    constexpr int RT = 2;                           // 16-row tiles per wave (paired: tile 0 gate, tile 1 filter)
    constexpr int CT = 2 * NJ;                      // 16-frame tiles per wave

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = ((a.taps - 1) >> 1) * a.dil;
    const int FW = BN + 2 * halo;
    float4* Xs = reinterpret_cast<float4*>(smem);   // [2][XP][FW]
    float4* Rs = Xs + 2 * XP * FW;                  // EPI_RES_SKIP: [32 planes][BN]
#ifdef DR_BOUNDS
    const unsigned xs0 = lds_off(Xs), xs1 = xs0 + 2u * XP * FW * 16u, rs1 = xs1 + (EPI == EPI_RES_SKIP ? 32u * BN * 16u : 0u);
    if (tid == 0) DR_CHECK(rs1 <= (unsigned)a.lds_bytes, 140, rs1, a.lds_bytes);
#endif

    const int tps = (a.T + BN - 1) / BN;
    const int b = nt / tps;
    const int t0 = (nt % tps) * BN;
    const int NS = a.kchunks * a.taps;
    const int nchunks = a.kchunks / KS;

    if (wave >= 4) {   // producers (LDS-DMA, hardware zero padding)
        producer<KS, 0, 0, EPI == EPI_RES_SKIP ? BN : 0>(a, Xs, Rs, wave - 4, lane, mt, b, t0, halo, FW, 0, nchunks, 141, 142);
        return;
    }

    // consumers.  16x16x4: A lane (i = l&15, kq = l>>4) holds W[row i][4 channels kq*4..+3 of a 16-channel
    // group] (one per MFMA), B lane (j = l&15, kq) the matching X values; C/D: column = l&15,
    // rows (l>>4)*4 + reg -> one float4 of the P4 layout per tile.
    const int li = lane & 15, kq = lane >> 4;
    float4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f4zero();

    // A fragments through buffer loads with scalar per-step offsets (as in gemm_kernel)
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.Wp + (long)mt * NS * 4096), 0, (unsigned)NS * 16384u, 0x00020000);
    const int wvo = (kq * 128 + wave * 32 + li) * 16;
    auto load_a = [&](int slab) -> AF4 {     // [g16][rt]
        AF4 o;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                DR_CHECK(slab >= 0 && wvo + slab * 16384 + g * 8192 + rt * 256 + 16 <= NS * 16384, 143, slab, NS);
                o.v[g * RT + rt] = buffer_load_f4(wrsrc, wvo, slab * 16384 + g * 8192 + rt * 256);
            }
        return o;
    };
    AF4 wA = load_a(0), wB;
    const int cen = (a.taps - 1) >> 1;
    const int per_chunk = a.taps * KS;
    typedef float v4f __attribute__((ext_vector_type(4)));

    // B fragments of one 16-channel group: CT float4 (one per 16-frame column tile)
    struct BF { float4 v[CT]; };
    BF b0, b1;
    auto xaddr = [&](int chunk, int q) -> const float4* {
        const int j = q / KS, sub = q - j * KS;
        return Xs + ((chunk & 1) * XP + sub * 8 + kq) * FW + halo + (j - cen) * a.dil + li;
    };
    auto rd = [&](const float4* Xb, int g) -> BF {
        BF o;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            DR_CHECK_LDS(Xb + g * 4 * FW + ct * 16, xs0, xs1, 144);
            o.v[ct] = Xb[g * 4 * FW + ct * 16];
        }
        return o;
    };
    auto mma = [&](const float4 af, const BF& bf, int rt) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            v4f c = {acc[rt][ct].x, acc[rt][ct].y, acc[rt][ct].z, acc[rt][ct].w};
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bf.v[ct].x, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bf.v[ct].y, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bf.v[ct].z, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bf.v[ct].w, c, 0, 0, 0);
            acc[rt][ct] = make_float4(c[0], c[1], c[2], c[3]);
        }
    };
    // K step = 2 groups of 16 channels; group 1's fragments are read before group 0's MFMAs, the NEXT step's
    // group 0 before group 1's MFMAs (cross-step prefetch inside a chunk, as in gemm_kernel)
    auto step = [&](auto ROLE, int slab, int chunk, int q) {
        constexpr bool kB = decltype(ROLE)::value;
        const float4* Xb = xaddr(chunk, q);
        if constexpr (kB) wA = load_a(min(slab + 1, NS - 1));
        else wB = load_a(min(slab + 1, NS - 1));
        b1 = rd(Xb, 1);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) mma(kB ? wB.v[rt] : wA.v[rt], b0, rt);
        b0 = rd(xaddr(chunk, min(q + 1, per_chunk - 1)), 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) mma(kB ? wB.v[RT + rt] : wA.v[RT + rt], b1, rt);
        // the 2*RT A-fragment loads of the next step ride inside group 0's MFMAs
        sgb<0x100, CT>(); sgb_spread<2 * RT, (4 * RT * CT) / (2 * RT)>();
        sgb<0x100, CT>(); sgb<0x8, 4 * RT * CT>();
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        auto at = [&](auto R, int q) {
            const int j = q / KS, sub = q - j * KS;
            step(R, (chunk * KS + sub) * a.taps + j, chunk, q);
        };
        __syncthreads();
        b0 = rd(xaddr(chunk, 0), 0);
        int q = 0;
        for (; q + 2 <= per_chunk; q += 2) {
            at(F_{}, q);
            at(T_{}, q + 1);
        }
        if (q < per_chunk) {
            at(F_{}, q);
            wA = wB;
        }
    }

    // epilogue: per (row tile, column tile) a lane owns rows rowbase + kq*4 .. +3 of frame column li
    const int rowb = mt * 128 + wave * 32 + kq * 4;     // + rt*16
    float4 ebias[RT], ed2[RT];
    const float* cbase = nullptr;           // EPI_GATE: the sample's conditioner tensor, frame 0 (as in gemm_body)
    if constexpr (EPI == EPI_GATE)
        cbase = (b < a.n_cond || !a.cond2) ? a.cond + (b < a.n_cond ? cond_row(a, b) : 0L) * a.c_bs : a.cond2;
    {
        const float* bsrc = a.bias;
        if constexpr (EPI == EPI_GATE) bsrc = (b < a.n_cond) ? a.bias : a.bias2;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            ebias[rt] = *reinterpret_cast<const float4*>(bsrc + rowb + rt * 16);
            if constexpr (EPI == EPI_RES_SKIP)
                ed2[rt] = *reinterpret_cast<const float4*>(a.d2 + (a.tsel ? (long)a.tsel[b] * a.d2_ts : 0) + min(rowb + rt * 16, a.y_rows - 4));
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int t = t0 + ct * 16 + li;
        if constexpr (EPI == EPI_GATE) {
            float4 cnd[RT];
            const int tc = min(t, a.T - 1);
            const float* cb = cbase + (long)tc * 4;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) cnd[rt] = *reinterpret_cast<const float4*>(cb + (long)((rowb + rt * 16) >> 2) * a.T * 4);
            if (t >= a.T) continue;
            const bool has_c = b < a.n_cond || a.cond2 != nullptr;
            {                                    // tile 0 = gate rows, tile 1 = filter rows of the same 16 channels
                const int c0 = mt * 64 + wave * 16 + kq * 4;
                if (c0 >= a.y_rows) continue;
                float v0[4], v1[4], o[4];
                f4arr(acc[0][ct], v0); f4arr(acc[1][ct], v1);
                gate_quad(v0, v1, ebias[0], ebias[1], cnd[0], cnd[1], has_c, o);
                if (a.out_s3 & 1) {
                    store_s3_quad(a.Y + (long)b * a.y_bs, o, c0, t, a.T, a.y_rows >> 3);
                } else {
                    store_quad(y_quad_ptr(a, b, c0, t), o);
                }
            }
        } else {
            float4 pv4[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                DR_CHECK_LDS(Rs + ((wave * 32 + rt * 16) / 4 + kq) * BN + ct * 16 + li, xs1, rs1, 145);
                pv4[rt] = Rs[((wave * 32 + rt * 16) / 4 + kq) * BN + ct * 16 + li];
            }
            if (t >= a.T) continue;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int p0 = rowb + rt * 16;
                float v[4], o[4];
                f4arr(acc[rt][ct], v);
                if (p0 < a.y_rows) {
                    float* dst = y_quad_ptr(a, b, p0, t);
                    residual_quad(v, ebias[rt], pv4[rt], o);
                    store_quad(dst, o);
                    if (a.Y2) store_y2<0, 0>(a, b, o, ed2[rt], p0, t);
                } else {
                    float* dst = skip_quad_ptr(a, b, p0, t);
                    skip_quad(v, ebias[rt], pv4[rt], a.skip_init, o);
                    store_quad(dst, o);
                }
            }
        }
    }
}

}  // namespace dr
