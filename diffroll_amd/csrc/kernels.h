// Internal launch interface between the host translation units (pack / plan / abi / debug_abi .hip: host logic, C-ABI) and the kernel translation units gemm / stack / tail / update / frontend .hip (gfx950 kernels).
// Not part of the public ABI (that is include/diffroll_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "chain_tables.h"     // window_entry / window_rec / window_idx, WindowTable
#include "launch_plan.h"      // Epilogue, tile / split-K / fused-stack planning

namespace dr {

// ---------------------------------------------------------------------------------------------
// Data layouts in HBM
//
//  "P4" activation layout: a (batch, channels, frames) tensor is stored as
//        [batch][plane = channel/4][frame][4]        (fp32; one float4 per (plane, frame))
//  so that (a) a wavefront's 64 lanes reading consecutive frames of a plane move 1 KiB
//  contiguously, (b) the float4 is exactly the 4 consecutive K-values an MFMA lane consumes
//  over 4 consecutive v_mfma_f32_32x32x2_f32 issues, and (c) the MFMA C/D fragment (4 consecutive
//  rows per lane per register quad) is written back as one float4 with no shuffles.
//  The roll (B, T, 88) is addressed with the same (batch, plane, frame) strides
//  (plane stride 4, frame stride 88), so no transposed copy is ever made.
//
//  Packed weights: for a GEMM  Y[M][N] = W[M][K] X[K][N]  with K = taps x Cin,
//        Wp[mtile][kchunk][tap][g = 0..3][hi = 0..1][row = 0..127][4]
//  = W[orig_row(mtile,row)][channel = kchunk*32 + g*8 + hi*4 + i][tap]; one (mtile,kchunk,tap)
//  slab is 16 KiB, contiguous, and is the exact LDS image the kernel reads (linear copy).
// ---------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------
// A/B knobs of the planners and launchers (process-wide; defaults = what ships).  They are set through
// dr_set_option(e, "tune.<field>", value) by tools/ and tests - the library reads no environment variable.
// ---------------------------------------------------------------------------------------------
// Fields are atomics (relaxed loads / stores are all that is needed: independent integers): dr_debug_set_option may run on
// one host thread while another engine's planner reads them.  Every change bumps tuning_epoch(), which is part of the key
// of every engine's captured chain: dr_sample does not replay a chain captured under older values.
struct Tuning {
    std::atomic<int> pack_threads{16};   // host threads packing the layers at dr_commit (1 = serial)
    std::atomic<int> tile{0};            // force a conv / LDS-staged 1x1 tile: 3201 / 3202 / 3203 / 3205 (32x32 MFMA, NI) or 1603 / 1605 (16x16, NJ); 0 = cost model
    std::atomic<int> pw{1};              // 1x1 residual/skip GEMM: 1 = operands direct from L2 (pw_kernel), 0 = the LDS-staged kernels
    std::atomic<int> pw_nw{0};           // force 32 * pw_nw frames per pw_kernel block (2..5); 0 = cost model; under pwk = 2: 1 / 2 = pwk_kernel's width
    std::atomic<int> pwk{1};             // under-filled 1x1 launches: K split over the block's waves (pwk_kernel); 0 = never; 2 = at every fill,
                                         // wherever the kernel exists (fp32, K slabs a multiple of 4): tests
    std::atomic<int> ksplit_max{16};     // largest split-K factor of gemm_kernel launches (1 = never split)
    std::atomic<long> ksplit_blocks{0};  // cap on tiles x ksplit (0 = 2048 fp32 / 256 split-bf16)
    std::atomic<int> one_ks{0};          // force the 1x1 GEMMs' channels-per-hand-over (KS = 1 / 2 / 4) where it divides the K slabs and fits the LDS;
                                         // 0 = by divisibility (launch_plan.h: pick_one_ks)
    std::atomic<int> stack3{1};          // the split-bf16 flavour of the fused residual stack
    std::atomic<int> stack_fl{0};        // force the fused stack's block flavour (1 / 2 / 5 = 64 / 128 / 160-frame blocks); -5 = never the 160-frame one; 0 = cost model
    std::atomic<int> tail_t4{0};         // force the item width of the tail kernel's first-layer conv (1 = 64, 3 = 96 frames); 0 = by rounds x width
    std::atomic<int> xcd_n{-1};          // force the block -> XCD mapping of per-phase GEMM launches (0 / 1) where mapping 1 exists (more than one
                                         // M tile, frame tiles a multiple of 8); -1 = traffic model (launch_plan.h: pick_xcd_mapping)
    std::atomic<int> xcd_model{1};       // 0 = the rounds 1-2 rule (activation bytes > weight bytes)
    std::atomic<int> s3_eager{0};        // build the split-bf16 packings at every dr_commit (rounds 1-3 behaviour)
    std::atomic<int> debug_chunks{0};    // dr_debug_ticks prints the chunk-start tick marks
};
Tuning& tuning();            // gemm.hip
std::atomic<unsigned>& tuning_epoch();
PlanKnobs plan_knobs();      // what the planners read of tuning(), now

struct GemmArgs {
    // A operand
    const float* Wp;      // packed weights
    const float* bias;    // [MT*128] in packed-row order; never null (pass a zero vector: loads are unconditional)
    const float* bias2;   // EPI_GATE: bias for samples >= n_cond (unconditional: conv bias + cond const)
    // B operand
    const float* X;
    long x_bs, x_ps, x_fs;   // batch / plane / frame strides in floats
    long x_piece;            // S3 input only: stride between the three bf16 pieces (4-byte units)
    int x_planes;            // valid planes (Cin/4); planes beyond re-read the last one (their weights are zero)
    int x_bmod;              // sample index is taken modulo this (0 = no modulo)
    int NB, T;               // samples, frames per sample
    int taps, dil;           // conv taps (odd) and dilation; halo = (taps-1)/2*dil
    int kchunks;             // ceil(Cin/32)
    int MT;                  // M tiles of 128 packed rows
    int mt0;                 // pw_kernel only: first M tile of the launch (tiles mt0 .. mt0 + MT - 1 are computed)
    // output
    float* Y;
    long y_bs, y_ps, y_fs;
    long y2_bs;              // batch stride of Y2 (4-byte units)
    int out_s3;              // bit 0: Y (EPI_GATE) is written in S3 split-bf16 layout; bit 1: Y2 is
    float* Y2;               // EPI_RELU / residual rows of EPI_RES_SKIP: optional second output Y2 = Y + d2[row]
                             // (same strides): the (h + step embedding) tensor the next dilated conv reads
    const float* d2;         // [>= y_rows] never null (zero vector when unused)
    const int* tsel;         // optional per-sample row selector of d2: sample b adds d2[tsel[b] * d2_ts + row] (per-sample
    long d2_ts;              // diffusion steps of forward(); null in the samplers: one step for the whole batch)
    int y_rows;              // valid output rows (quads starting at >= y_rows are not written)
    // epilogue extras
    const float* cond;       // EPI_GATE: [n_cond][MT*32 planes][T][4] in packed-row order; must point at valid memory
                             // of at least one sample even when n_cond == 0 (prefetched unconditionally, then ignored)
    long c_bs;
    int c_b0, c_n;           // EPI_GATE: conditional sample b reads conditioner tensor c_b0 + b, taken modulo c_n when c_n > 0:
                             // the launch's first row in the roll batch and the clips of the last dr_frontend (option "draws":
                             // row b of the batch is draw b / n of clip b % n; a sample chunk may start inside a draw and wrap)
    const float* cond2;      // EPI_GATE, optional: one conditioner tensor [MT*32 planes][T][4] shared by all samples >= n_cond
                             // (the learned unconditional spectrogram of condition='trainable_spec'); null: they use bias2 only
    int n_cond;
    int dual;                // EPI_GATE, gemm_kernel only: > 0 = also write sample b + dual from the same accumulators
                             // with the unconditional bias (first layer under classifier-free guidance); NB counts b only
    float* skip;             // EPI_RES_SKIP: P4 [NB][MT/2*32 planes][T][4]
    long s_bs;
    int skip_init;           // 1: skip = value, 0: skip += value
    float alpha;
    int xcd_n;               // set by the launcher: block -> (M tile, frame tile) mapping, see gemm_kernel
    // split-K (gemm_kernel only; optional): partial-accumulator workspace + zero-initialised ticket counters.
    // The launcher picks ksplit (1 when ws is null or the launch already fills the chip).
    float* ws;               // >= tiles * ksplit * 128 * BN floats
    unsigned* ws_cnt;        // >= tiles * 4 counters, all zero between launches
    size_t ws_floats, ws_cnt_n;
    int ksplit;              // set by the launcher
    long long* dbg;          // measurement hook: block 0 writes {main-loop ticks, block ticks} (s_memtime); null normally
    int lds_bytes;           // set by the launcher: dynamic LDS of the launch (read by DR_BOUNDS checker builds only)
    int fold128;             // EPI_GATE on 128-frame blocks (NI = 2, fp32): 1 = the blocked-accumulation instantiation
    int nofold64;            // EPI_GATE on 64-frame blocks (NI = 1, fp32, no split-K): 1 = ONE chain per output instead of the blocked
                             // accumulation every other 64-frame launch uses - the shared first-layer conv of an engine whose fused
                             // 128-frame stack runs single-chain (blocked_accumulation = 1), so that the per-phase launch and the
                             // tail kernel's copy of that conv (TailArgs::fold = 0) produce the same bits
    int wt_store;            // fused residual stack only (COH bodies): 1 = the tensors handed to other workgroups are
                             // stored write-through (sc1), 0 = plain stores (every workgroup of the group shares one
                             // XCD's L2, verified at run time)
    int zero_taps;           // EPI_GATE on 128-frame blocks (NI = 2, fp32, blocked accumulation): 1 = a block leaves out the edge tap
                             // whose window of its first / last 32-frame tile is all zero padding (zero_taps.h; lab option
                             // "zero_taps", default 1; 0 = every tap of every tile, the same bits)
};

// gemm_kernel: block tile = 128 packed rows x 64*NI frames (NI in {1, 2}), 512 threads (4 consumer + 4 producer
// waves); call init_kernels() once per process before any launch.
hipError_t init_kernels();
// DR_BOUNDS checker builds: {code of the first violated check, detail, detail, number of violations} / reset;
// hipErrorNotSupported in production builds
hipError_t read_bounds(unsigned long long* out4);
hipError_t reset_bounds();
// prec = 0: fp32 X / weights; 1: split-bf16 ("S3") X / weights (EPI_GATE and 1x1 EPI_RES_SKIP only); 2: one-pass bf16 X /
// weights (the same two GEMMs; X, the EPI_GATE output and Y2 are [batch][channel/8][frame][8 bf16], out_s3 is not read);
// 4: one-pass f16 - as 2 with IEEE binary16 in place of bf16.  The codes are the DR_PRECISION_* values; 3 is refused.
hipError_t launch_gemm(const GemmArgs& a, int epi, int NI, hipStream_t s, int prec = 0);
// flexible-width variant (16x16x4 MFMA): block = 128 rows x 32*NJ frames, NJ in {3,5}; fp32, EPI_GATE / 1x1 EPI_RES_SKIP
hipError_t launch_gemm16(const GemmArgs& a, int epi, int NJ, hipStream_t s);
// 1x1 EPI_RES_SKIP GEMM with both operands direct from L2 (no LDS): block = 128 rows x 32*NW frames
// (NW in {2,3,4,5}), 256 threads
hipError_t launch_pointwise(const GemmArgs& a, int NW, hipStream_t s);
// precision "bf16": src = P4 fp32 [NB][Cp/4][T][4] -> dst = [NB][Cp/8][T][8 bf16], each value rounded to nearest even
// (the first dilated conv's input, which the fp32 input projection leaves in P4)
hipError_t launch_round_bf16(const float* src, float* dst, int NB, int Cp, int T, hipStream_t s);
// precision "f16": the same with 8 IEEE binary16 per unit (round to nearest even, subnormals kept)
hipError_t launch_round_f16(const float* src, float* dst, int NB, int Cp, int T, hipStream_t s);
hipError_t launch_pointwise_ksplit(const GemmArgs& a, int NW, hipStream_t s);   // under-filled launches: 32-row tiles, K split over the block's waves

// ---------------------------------------------------------------------------------------------
// Fused residual stack: ONE persistent launch runs a range of the 2L phases of the residual layers
// (phase 2l = dilated conv + conditioner + gate of layer l, phase 2l+1 = its 1x1 + residual / skip), instead of
// one launch per phase.  grid = (samples x frame tiles x M tiles) <= the number of CUs, every block owns the same
// (M tile, frame tile) in every phase; the blocks of one sample (= one clip evaluation: M tiles x its frame tiles)
// form a GROUP that synchronises on a device counter between phases - nothing is exchanged between groups, so
// there is no grid-wide barrier.  See stack_kernel in stack.hip.
// ---------------------------------------------------------------------------------------------
struct StackLayer {
    const float *conv_w, *conv_b, *conv_b2;   // packed dilated-conv weights; bias of samples < n_cond / >= n_cond
    const float *cond, *cond2;                // conditioner tensors of this layer (see GemmArgs)
    const float *out_w, *out_b;               // packed 1x1 weights / bias
    int dil, pad_;
};
struct StackArgs {
    float *h, *hd, *g, *skip;                 // P4 activations [NB][Cp/4][T][4]
    const float* d2;                          // step-embedding rows: layer l+1's row is d2 + (l + 1) * Cp (+ tsel[b] * d2_ts)
    const int* tsel;
    long d2_ts;
    const float* zero;                        // device zero vector (never-null operands)
    int NB, T, Cp, taps, n_cond, L;
    long c_bs;
    int c_b0, c_n;                            // first row of this chunk in the roll batch / clips of the conditioner (GemmArgs)
    int p0, p1;                               // phases [p0, p1)
    int xcd_n;                                // block -> (M tile, frame tile) mapping, as in gemm_kernel
    int rs_off;                               // set by the launcher: LDS byte offset of the resident h / skip tile
    int lds_bytes;                            // set by the launcher: dynamic LDS of the launch (DR_BOUNDS checker builds)
    int fault;                                // test hook: barriers wait for one arrival too many (exercises the spin bound)
    int fold128;                              // FL = 2: 1 = the instantiation with blocked accumulation in its conv phases
    int warm;                                 // idle waves warm the L2 with the next phase's weights / conditioner tile
    int zero_taps;                            // conv phases: GemmArgs::zero_taps
    unsigned* xid;                            // [grid] scratch: the XCC each block runs on (rewritten by every launch)
    unsigned* bar;                            // [groups][4] {arrivals, departures, generation, -}; the first two are zero
                                              // between launches, the generation advances by one per launch
    unsigned* err;                            // host-mapped: set to 1 if a barrier wait ran into its spin bound (never in a
                                              // healthy run)
    unsigned* derr;                           // device copy of that flag: polled by the waits, and a launch that finds it set
                                              // returns at once (cleared by the host together with *err)
    long long* dbg;                           // optional: block 0 writes s_memtime at every phase start (dbg[p - p0]) and at the end
    StackLayer layer[DR_STACK_MAX_LAYERS];
};
// FL = block flavour: 1 / 2 = 128 packed rows x 64 / 128 frames.  The caller guarantees
// NB * stack_group_blocks(FL, Cp, T) <= #CUs and stack_lds_bytes(..) <= 160 KiB.
// prec = 1: the split-bf16 flavour (s.hd / s.g = the S3 tensors; Cp % 128 == 0; LDS: stack3_lds_bytes)
// prec = 2 / 4: the one-pass bf16 / f16 flavour (s.hd / s.g = the one-plane-set 16-bit tensors; same restriction and LDS function)
hipError_t launch_stack(const StackArgs& s, int FL, int max_dil, hipStream_t st, int prec = 0);

// Per-call scalars of the update that must not be baked into a captured graph: the chain graph reads them from
// this device block, which a one-thread kernel rewrites (stream-ordered) before every graph launch - a new
// seed / batch offset / guidance weight re-uses the instantiated graph.
struct DynParams {
    unsigned long long seed;
    int first_sample;
    float w, onepw;
    unsigned epoch;        // long-form windows: the tail launches of this chain publish epoch + TailArgs::epoch (see tail_kernel)
};
hipError_t launch_set_dyn(DynParams* d, unsigned long long seed, int first_sample, float w, float onepw, unsigned epoch,
                          hipStream_t s);

struct UpdateArgs {
    float* x;              // (B, T, 88) in/out
    const float* x0c;      // (B, T, 88) conditional (or the only) prediction
    const float* x0u;      // unconditional prediction or null
    const float* noise;    // (B, T, 88) or null -> philox
    const float* coef;     // device pointer to this step's 5 coefficients
    int t;                 // step index
    int mode;              // coefficient family (DR_COEF_*): 0/1 x0 update, 2 eps ddpm, 3 eps ddim, 4 eps ddim2ddpm;
                           // 5 = option "solver_order": the multistep solver update (update_quad.h: solver_quad)
    long n;                // B*T*88
    long per_sample;       // T*88
    float w, onepw;
    uint64_t seed;
    int first_sample;
    const DynParams* dyn;  // non-null: w / onepw / seed / first_sample are read from here instead
    // Long-form windows (option "window_overlap" = O > 0; 0 = off): the B rolls are B consecutive windows of ONE
    // recording on a canvas of (B - 1) * win_H + T frames, window b starting at canvas frame b * win_H, win_H = T - O,
    // 2 O <= T.  A frame shared by windows b and b + 1 (frames [win_H, T) of b = frames [0, O) of b + 1) uses the mean
    // 0.5 (y_b + y_b+1) of the two windows' guided predictions, and Philox is keyed by (seed, first_sample = the
    // recording, t, canvas element / 4): both windows compute the same x_{t-1} there, bit for bit.
    // Option "window_blend" travels in the same word: win = win_H | blend << 28 (win_H < 2^28; read them with win_H() /
    // win_blend() below) - how a shared frame combines the two predictions: 0 the mean above, 1 the linear cross-fade, 2 the
    // hand-over at the middle of the overlap (update_quad.h: blend_quad).  Spare bits of this word and not a word of its
    // own: the argument block does not grow, and tail_kernel parks no more scalars than it did
    // (profiles/blend_kernel_resources.txt).  A zero-initialised block is off in both.
    int win;
    // Recording boundaries inside the window batch (option "window_break"): null = one recording (the definition above);
    // else the engine's per-window table, win_tab[b] = window_entry(r, i): window b is window i of recording r of the batch.
    // Windows b and b + 1 share frames only when b + 1 is not the first window of a recording (i(b + 1) > 0), the canvas
    // above is recording r's own ((n_r - 1) * win_H + T frames, window b at frame i * win_H) and Philox is keyed
    // (seed, first_sample + r, t, canvas element of recording r / 4).
    const unsigned* win_tab;
    // Option "draws" (D > 1; draw_n = 0: off): roll b is draw b / draw_n of clip b % draw_n and its Philox sample key is
    // first_sample + b % draw_n + (b / draw_n) * draw_G (draw_G = draw_n unless option "draw_stride" says otherwise).  Windows
    // (win_H > 0) carry the draw in their table word instead: win_tab is then always set.
    int draw_n, draw_G;
    // Mode 5, order 2 (null: first order): the history - ONE engine buffer of two (B, T, 88) halves, n floats apart, used
    // ping-pong.  Half hist_par holds the guided prediction (after the shared-frame mean) of the previous step, read only
    // where this step's row has c != 0; this step's goes into the other half while t > 0 (a step follows) - never the same
    // one: the tail kernel's row tiles recompute a quad in different blocks.  One pointer and one parity word instead of two
    // pointers: under option "solver_noise" mode 5 reads `noise` and `seed` too, so the history can no longer share their
    // storage, and the argument block - SGPRs the tail kernel is short of (profiles/solver_noise_kernel_resources.txt) -
    // grows by three words instead of four.
    float* hist;
    int hist_par;
    // Option "x0_clip" (0 = off): the prediction the update consumes - guided, after the shared-frame mean - is clamped to
    // [clamp_lo, clamp_hi] in front of everything that reads it (update_quad.h: clamp_quad); x0 samplers only (mode 0 / 1 / 5).
    // On where clamp_lo < clamp_hi: a zero-initialised block is off.  The bounds themselves, not the option's code: of the forms
    // tried this one parks the fewest scalars of the tail kernel in VGPR lanes (profiles/clip_kernel_resources.txt).
    float clamp_lo, clamp_hi;
};
// (mode 5) the half the step reads / the half it writes, null where it stores nothing
__host__ __device__ inline const float* hist_prev(const UpdateArgs& a) { return a.hist + (a.hist_par ? a.n : 0); }
__host__ __device__ inline float* hist_next(const UpdateArgs& a) { return a.hist && a.t > 0 ? a.hist + (a.hist_par ? 0 : a.n) : nullptr; }
// the two fields of UpdateArgs::win: the windows' stride H = T - O (0: independent clips) and the mode of option "window_blend"
constexpr int WIN_BLEND_SHIFT = 28;
__host__ __device__ inline int win_H(const UpdateArgs& a) { return a.win & ((1 << WIN_BLEND_SHIFT) - 1); }
__host__ __device__ inline int win_blend(const UpdateArgs& a) { return a.win >> WIN_BLEND_SHIFT; }
// (the words of the per-window table and the table itself: chain_tables.h)
hipError_t launch_set_windows(unsigned* d_tab, const WindowTable& tab, int n, hipStream_t s);
hipError_t launch_update(const UpdateArgs& a, hipStream_t s);
// option "start_noise": x = (coef[2] * x) + (coef[3] * z) in place (update.hip: diffuse_kernel).  Of UpdateArgs it reads x,
// noise (z, or null: Philox), coef, t (the Philox counter word: timesteps + the start step), n, per_sample, seed /
// first_sample (or dyn), win (its win_H), win_tab, draw_n, draw_G
hipError_t launch_diffuse(const UpdateArgs& a, hipStream_t s);

// Option "x0_threshold" (include/diffroll_amd.h): dynamic thresholding of the prediction the update consumes.  One q - the
// exact v / 10000 quantile of |y - m| - is taken over each GROUP of the batch: a clip's roll, or under "window_overlap" a
// recording's canvas, every canvas frame counted once (a window that is not its recording's first contributes frames [O, T)).
// The threshold launches (threshold.hip) leave {q, s = max(q, r)} of a group in the record of the group's FIRST row; the
// update's thresholding form reads s from there.
// The engine's work buffer: [0] the ticket of the multi-launch form (zero between launches), then one record of
// THRESH_ROW_WORDS words per row of the batch at THRESH_HEAD + row * THRESH_ROW_WORDS:
//   [0, 256) the digit counts of the running pass (zero between launches), [256] the pattern bits selected so far,
//   [257] the rank still sought among the elements that carry them, [258] elements in the selected bin, [259] ~(the smallest
//   pattern above a[k]) (zero between launches: armed), [260] rem, [264] q, [265] s.
// The words that must be zero sit at the same offsets whatever B a call has, so one buffer serves every batch that fits.
constexpr int THRESH_HEAD = 4, THRESH_ROW_WORDS = 272, THRESH_SEL = 256, THRESH_QS = 264;
inline size_t thresh_work_words(int B) { return (size_t)THRESH_HEAD + (size_t)B * THRESH_ROW_WORDS; }
struct ThreshArgs {
    UpdateArgs u;          // read: x0c, x0u, w / onepw (or dyn), n, per_sample, win, win_tab - what forms y (threshold_quad.h: pred_quad)
    float m, r;            // centre and half-width of the range "x0_clip" names
    int v;                 // the percentile, 1 / 10000
    int pass;              // multi-launch form: 0-3 the radix passes (8, 8, 8, 7 bits from the top), 4 the successor pass
    unsigned* work;        // the buffer above, thresh_work_words(B) words
};
// What the update's thresholding form needs beside UpdateArgs (a second kernel argument: UpdateArgs, embedded in TailArgs,
// does not grow): the q / s pair of row 0's record - row b's is THRESH_ROW_WORDS floats further per row - and m, r.
struct ThreshUpd {
    const float* qs;
    float m, r;
};
// every launch of one step's selection: one launch of one workgroup per roll (clips of at most THRESH_ROLL_MAX elements), or
// five launches over all rows (windows, longer clips)
constexpr long THRESH_ROLL_MAX = 65536;
hipError_t launch_threshold(ThreshArgs a, int B, hipStream_t s);
// update_kernel's thresholding form (update.hip: update_thresh_kernel)
hipError_t launch_update_thresh(const UpdateArgs& a, const ThreshUpd& th, hipStream_t s);
// (dr_debug_threshold) out (G, 2) = {q, s} of the batch's groups in row / recording order
hipError_t launch_thresh_gather(const ThreshArgs& a, int B, float* out, hipStream_t s);

// The work buffer of a statistics launch over the GROUPS above ("cfg_rescale", "cfg_project" / "cfg_norm", "cfg_momentum";
// group_sums.h has the launch) - one layout, stated here alone:
//   [0] the ticket of the grid form (zero between launches);
//   then one record of GS_ROW_WORDS words per row of the batch at GS_HEAD + row * GS_ROW_WORDS - a group's result, in the
//   record of its FIRST row;
//   then - grid form - one slot of K doubles per (row, block of GS_BLOCK frames), row-major: the block's K sums.  Every slot
//   a launch adds up was written by that launch: the slots need no re-arming, and one buffer serves every batch that fits -
//   and every one of the options: the engine holds ONE, of gs_work_words(B, T, GS_SUMS_MAX) words (below), a step runs one launch.
constexpr int GS_HEAD = 4, GS_ROW_WORDS = 2, GS_BLOCK = 64;
inline size_t gs_blocks(int T) { return ((size_t)T + GS_BLOCK - 1) / GS_BLOCK; }
inline size_t gs_work_words(int B, int T, int K) { return (size_t)GS_HEAD + (size_t)B * GS_ROW_WORDS + (size_t)B * gs_blocks(T) * K * 2; }
inline const float* gs_records(const unsigned* work) { return reinterpret_cast<const float*>(work + GS_HEAD); }
// (dr_debug_rescale / dr_debug_project / dr_debug_momentum) out (G, words) = the first `words` words of the records of the
// batch's groups, in row / recording order; u = the Args' UpdateArgs, work = their buffer
hipError_t launch_group_gather(const UpdateArgs& u, const unsigned* work, int words, int B, float* out, hipStream_t s);

// Option "cfg_rescale" (include/diffroll_amd.h): the guidance rescale of Lin et al. 2024.  At a step that guides, one factor
//   g = (float)(1 + phi (sqrt(Vc / Vy) - 1))
// per GROUP - the group of "x0_threshold" above - scales the guided prediction y towards the spread of the conditional
// prediction c (both after the shared-frame mean / blend); the update consumes g y.  The statistics launches (rescale.hip)
// leave g in the record of the group's FIRST row; the update's rescaling form reads it from there.
// The engine's work buffer is the one above: a record is [0] g, a slot the four doubles {S1c, S2c, S1y, S2y}.
constexpr int RESCALE_SUMS = 4;
struct RescaleArgs {
    UpdateArgs u;          // read: what pred_quad reads (ThreshArgs::u); x0u is set - the step guides
    int phi;               // the option's value, 1 .. 10000
    unsigned* work;        // the buffer above, at least gs_work_words(B, T, RESCALE_SUMS) words
};
// What the update's rescaling form needs beside UpdateArgs (the second kernel argument, as ThreshUpd is): g of row 0's
// record (gs_records) - row b's is GS_ROW_WORDS floats further per row - and what follows the product: th.qs set = the
// thresholding of "x0_threshold" with th, else the clamp UpdateArgs names, or nothing.
struct RescaleUpd {
    const float* g;
    ThreshUpd th;
};
// a step's statistics: one launch of one workgroup per roll (clips of at most THRESH_ROLL_MAX elements), or one launch of
// (blocks, rows) workgroups whose last arriver sums the slots (windows, longer clips)
hipError_t launch_rescale(const RescaleArgs& a, int B, hipStream_t s);
// a step's threshold launches ranking |g y - m| (threshold.hip: the kernels' rescaled forms); g as in RescaleUpd
hipError_t launch_threshold_rescaled(ThreshArgs a, const float* g, int B, hipStream_t s);
// update_kernel's rescaling form (update.hip: update_rescale_kernel)
hipError_t launch_update_rescale(const UpdateArgs& a, const RescaleUpd& rs, hipStream_t s);

// Options "cfg_project" / "cfg_norm" (include/diffroll_amd.h): adaptive projected guidance (Sadat et al. 2024) without its
// momentum - that part needs a roll-sized state with validity rules like the solver history's and is option "cfg_momentum" below;
// the combined form with "cfg_rescale" (which would need the spread of y') and with "x0_threshold" (a third text form of
// threshold.hip) are refused (abi.hip: check_options).  At a step that guides, one pair
//   a = (float)((1 - s) - s (rho k)),   b = (float)s
// per GROUP - the group of "x0_threshold" above - turns the guided prediction y into y' = (a c) + (b y), c the conditional
// prediction (both after the shared-frame mean / blend): the update c - u bounded in rms, its component parallel to c reduced
// by rho.  The statistics launches (project.hip) leave (a, b) in the record of the group's FIRST row; the update's projecting
// form reads them from there.
// The engine's work buffer is the one above (the same one): a record is [0] a, [1] b, a slot the three doubles {Scc, Scd, Sdd}.
constexpr int PROJECT_SUMS = 3;
constexpr int GS_SUMS_MAX = RESCALE_SUMS > PROJECT_SUMS ? RESCALE_SUMS : PROJECT_SUMS;      // the K the engine's one buffer is sized for
struct ProjectArgs {
    UpdateArgs u;          // read: what pred_quad reads (ThreshArgs::u); x0u is set - the step guides
    int rho;               // "cfg_project", 0 .. 10000
    int norm;              // "cfg_norm", 0 .. 100000 (0: no bound); one of the two is not 0
    unsigned* work;        // the buffer above, at least gs_work_words(B, T, PROJECT_SUMS) words
};
// What the update's projecting form needs beside UpdateArgs (the second kernel argument, as ThreshUpd is): (a, b) of row 0's
// record (gs_records) - row b's is GS_ROW_WORDS floats further per row.  What follows is the clamp UpdateArgs names, or nothing.
struct ProjectUpd {
    const float* ab;
};
// a step's statistics: one launch of one workgroup per roll (clips of at most THRESH_ROLL_MAX elements), or one launch of
// (blocks, rows) workgroups whose last arriver sums the slots (windows, longer clips)
hipError_t launch_project(const ProjectArgs& a, int B, hipStream_t s);
// update_kernel's projecting form (update.hip: update_project_kernel)
hipError_t launch_update_project(const UpdateArgs& a, const ProjectUpd& pj, hipStream_t s);

// Option "cfg_momentum" (include/diffroll_amd.h): the momentum of adaptive projected guidance - the third part of the method,
// beside "cfg_project" / "cfg_norm".  At a step that guides, per element and in fp32 (each operation rounded once),
//   d = y - c,   m = d at the step that STARTS the state, else m = d + (bf * m_prev),   yb = c + m
// and everything the two options above define happens with yb in place of y.  m is the engine's state: one float per roll
// element (the layout of the roll, B x T x 88), updated IN PLACE by the update - an element's thread is its word's only
// reader and writer; neighbouring windows read each other's predictions, never each other's state (a frame two windows
// share holds the same m in both rows: d is bit-identical there).  The statistics launch reads m_prev and forms m and yb on
// the fly (momentum.hip: the two launch forms, slots and ticket of project.hip, on the same work buffer - a step runs one of
// the two); "starts" is a fact of the step, baked per node in a captured chain (chain_tables.h: momentum_step for dr_step).
struct MomentumArgs {
    ProjectArgs p;         // what the statistics of "cfg_project" / "cfg_norm" read and write
    const float* m_prev;   // the state the step reads; null: the step STARTS the state (nothing is read)
    float bf;              // (float)((double)cfg_momentum / 10000.0)
};
// What the update's momentum form needs beside UpdateArgs (its second kernel argument, in ProjectUpd's place)
struct MomentumUpd {
    const float* ab;       // ProjectUpd::ab
    float* m;              // the state: read unless `start`, then written, by the element's own thread
    float bf;
    int start;             // 1: the step starts the state
};
// a step's statistics in their momentum form: launch_project's two forms over yb
hipError_t launch_momentum(const MomentumArgs& a, int B, hipStream_t s);
// update_kernel's momentum form (momentum.hip: update_momentum_kernel)
hipError_t launch_update_momentum(const UpdateArgs& a, const MomentumUpd& mo, hipStream_t s);
// (dr_debug_momentum) m_next = m of every element, by the device function the update uses; m_prev null: starts
hipError_t launch_momentum_state(const UpdateArgs& a, const float* m_prev, float bf, float* m_next, hipStream_t s);

// Option "guidance_stride" (include/diffroll_amd.h): the guidance update d = y - c of a step that REFRESHES - y the guided
// prediction, c the conditional one, both after the shared-frame mean / blend, fp32, one rounding - is the engine's state, one
// float per roll element (the layout of the roll, B x T x 88), stored by the element's own thread and left as it is by the
// steps that REUSE it: those run the conditional evaluation alone and consume y = c + d.  Neighbouring windows read each
// other's predictions, never each other's state (a frame two windows share holds the same d in both rows).  Refresh or reuse
// is a fact of the step, baked per node in a captured chain (chain_tables.h: stride_step for dr_step).  What the update's
// stride form needs beside UpdateArgs - its second kernel argument, StrideUpd - and its form_quad: stride_quad.h.
struct StrideUpd;
// update_kernel's stride form (stride.hip: update_stride_kernel); a refresh step has a.x0u set, a reuse step has it null
hipError_t launch_update_stride(const UpdateArgs& a, const StrideUpd& su, hipStream_t s);

// Tail of a reverse step as one persistent launch (tail_kernel in tail.hip): skip projection -> output projection ->
// classifier-free combine + posterior update -> input projection of the next step.  Same grid / grouping as the
// stack_kernel launch it follows: NB samples (first `dual` conditional, next `dual` unconditional when dual > 0) x
// ceil(T / BN) frame tiles x Cp / 64 blocks, all resident at once.
struct TailArgs {
    int NB, T, Cp, BN;                        // BN = frames per block of the preceding stack launch (64 / 128 / 160): grouping only
    int dual;                                 // B > 0: classifier-free pairs (sample b, sample b + B) NOW - how x0 is combined and who
                                              // meets at the pair barriers; 0: every sample on its own
    int dual_next;                            // B > 0: the NEXT step is guided - h / hd are written for rows b and b + B and conv_w
                                              // may be set; 0: rows b only, no conv.  Differs from `dual` at the two ends of a
                                              // guidance interval (options "guidance_t_min" / "guidance_t_max")
    int u_B;                                  // rolls to update (B)
    int xcd_n, fault;
    float alpha;                              // 1 / sqrt(residual_layers)
    const float* skip;                        // P4 [NB][Cp/4][T][4]
    float* tmp;                               // P4 workspace, same shape
    float* x0;                                // (NB, T, 88): network outputs (u.x0c / u.x0u point into it)
    const float *skip_w, *skip_b, *outp_w, *outp_b, *zero;
    UpdateArgs u;                             // the update of this step; u.x = x_t is only READ here
    float* x_out;                             // x_{t-1} is written here (never u.x: other blocks still read x_t)
    const float *in_w, *in_b, *d2_next;       // input projection of the NEXT step (in_w null: the chain ends here / single step)
    float *h, *hd;                            // its outputs, P4 [NB][Cp/4][T][4]
    // the next step's shared first-layer conv (dual_next > 0 and in_w set; conv_w null: none): layer 0 as in StackLayer
    const float *conv_w, *conv_b, *conv_b2, *cond, *cond2;
    long c_bs;
    int c_n;                                  // clips of the conditioner (GemmArgs::c_n)
    int taps, dil;
    int fold;                                 // blocked accumulation in that conv (gemm_body.h), as the stack launch that follows
    int t4_ni;                                // in: 0 = the launcher chooses T4's item width, 1 / 3 = force 64 / 96 frames; the launcher sets 1 or 3
    float* g;                                 // its output, P4 [NB][Cp/4][T][4]
    int lds_bytes;                            // set by the launcher
    long long* dbg;                           // optional: block 0 writes s_memtime at the start and after T1, its barrier, T2, its
                                              // barrier, T3, its barrier, T4 (8 marks)
    unsigned *bar, *pbar, *err, *derr;        // counters as in StackArgs (own arrays), time-out flags (shared with the stack)
    // long-form windows (win_H(u) > 0): T3 of window b reads the x0 that windows b - 1 / b + 1 wrote in their T2.  After
    // its pair barrier, window b publishes ready[b] = epoch and waits for its neighbours' words to reach it.  The words
    // only ever grow (epoch = (u.dyn ? u.dyn->epoch : 0) + this launch's epoch, a per-engine count of tail launches):
    // a replayed graph and a neighbour that has already left the launch are both seen correctly.
    unsigned* ready;                          // [STACK_GROUPS] one word per window, zero after a time-out's re-arm
    unsigned epoch;
};
hipError_t launch_tail(const TailArgs& s, hipStream_t st);

hipError_t launch_reflect_pad(const float* wav, float* out, int B, int L, int pad, hipStream_t s);
// STFT power by FFT (N a power of two): wav_pad (B, Lp) -> power (B, TF, bins_p) row-major; win (N) the window,
// tw (N complex) = exp(-2 pi i k / N), norm = sqrt(sum win^2) (the spectrum is divided by it)
hipError_t launch_stft_power(const float* wav_pad, const float* win, const float* tw, float* power, int B, int Lp, int TF,
                             int N, int hop, int bins_p, float norm, hipStream_t s);
// per-sample min/max of logmel P4 [B][planes][TF][4] over rows < n_rows -> mm[B][2]; scratch = minmax_scratch_floats(B)
// floats of device memory, zero before its first use (partials + one ticket word per sample, left zero by the kernel)
hipError_t launch_minmax(const float* logmel, float* mm, float* scratch, int B, int planes, int TF, int n_rows, hipStream_t s);
size_t minmax_scratch_floats(int B);
// normalise, mask, trim -> spec P4 [B][planes_out][T][4] (rows >= n_rows zero) and optional plain (B, n_rows, T)
// framewise = 1: mm holds one (min, max) per (sample, frame) [B][TF][2] (launch_minmax_frame) instead of per sample
hipError_t launch_minmax_frame(const float* logmel, float* mm, int B, int planes, int TF, int n_rows, hipStream_t s);
hipError_t launch_normalize(const float* logmel, const float* mm, float* specP4, float* spec_plain,
                            int B, int planes_in, int planes_out, int TF, int T, int n_rows,
                            int mt0, int mt1, int mf0, int mf1, hipStream_t s, int framewise = 0);
hipError_t launch_fill(float* p, float v, long n, hipStream_t s);
// q_sample / extract_x0 of task/diffusion.py:31-64 (mode 0 / 1): per-sample schedule lookup by t[b], elementwise
hipError_t launch_noise_mix(int mode, const float* x, const float* y, const int64_t* t, const float* sac,
                            const float* s1m, int n_steps, int B, long per_sample, float* out, hipStream_t s);
// note_end[b][t][p] = offset frame (exclusive) of the note that STARTS at frame t on pitch p, else 0:
// roll (B, T, 88) thresholded at thr; a note = maximal run of frames above the threshold (rule1 with
// onsets == frames, task/diffusion.py:1185-1233)
hipError_t launch_note_runs(const float* roll, int* note_end, int B, int T, float thr, hipStream_t s);
// work[0..2] = {TP, FP, FN} of (pred > thr) against (label > 0.5) over n elements (exact integers); work = device
// scratch of frame_counts_work_words() 64-bit words, zero before its first use (the kernel leaves its ticket word zero)
hipError_t launch_frame_counts(const float* pred, const float* label, float thr, long n,
                               unsigned long long* work, hipStream_t s);
size_t frame_counts_work_words();
hipError_t init_update_kernels();

}  // namespace dr
