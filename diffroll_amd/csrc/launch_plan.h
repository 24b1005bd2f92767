// Launch planning: which tile flavour and split-K factor a per-phase GEMM launch gets, and whether a network evaluation
// runs its residual layers as fused persistent launches (stack_kernel<FL>, how many sample chunks, the tail kernel).
// Every decision is a pure function of the launch shape and a PlanKnobs snapshot of the A/B knobs (kernels.h: Tuning);
// run_network (plan.hip) takes one plan per evaluation and only carries it out.  Host code; plain C++
// (tests/test_launch_plan_cpu.py compiles it without HIP).
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/diffroll_amd.h"      // DR_MODE_*

namespace dr {

enum Epilogue : int {
    EPI_PLAIN = 0,     // y = alpha*acc + bias
    EPI_RELU = 1,      // y = relu(alpha*acc + bias)
    EPI_SILU = 2,      // y = silu(acc + bias)
    EPI_GATE = 3,      // rows paired (gate, filter): y = sigmoid(a0 + c0) * tanh(a1 + c1)
    EPI_RES_SKIP = 4,  // first half of M: h = (h + acc + b)/sqrt(2) in place; second half: skip (+)= acc + b
    EPI_POWER = 5,     // rows paired (cos, sin): y = a0^2 + a1^2
    EPI_LOG = 6        // y = log(acc + 1e-6)
};

constexpr int DR_STACK_MAX_LAYERS = 30;          // residual layers a fused stack launch carries (StackArgs::layer)
constexpr int STACK_GROUPS = 512;                // barrier groups (samples) of one fused launch: the engine's counter arrays
constexpr size_t SK_WS_FLOATS = (size_t)16 << 20, SK_CNT_N = 4096;     // split-K workspace of an engine, 64 MiB: up to
                                                                      // 1024 partial tiles of 128 x 128, and its tickets

// The A/B knobs the planners read (kernels.h: Tuning, which documents them), as plain values: plan_knobs() (gemm.hip)
// takes a snapshot.  The defaults are the shipping values.
struct PlanKnobs {
    int tile = 0, pw = 1, pw_nw = 0, pwk = 1, ksplit_max = 16;
    long ksplit_blocks = 0;
    int stack3 = 1, stack_fl = 0;
    int xcd_n = -1, xcd_model = 1, tail_t4 = 0, one_ks = 0;
};

// The precision codes are the DR_PRECISION_* values (3 is reserved and never reaches the planners or the kernels).
// THE one-plane 16-bit modes: each operand of the two hot contractions rounded once to a 16-bit format - bf16 (2) or IEEE
// binary16 (4) - and carried as ONE plane set [batch][channel/8][frame][8 x 16 bit].  The two share every layout, LDS
// size and planner decision; they differ in the conversion and in the MFMA (device_common.h: Half16<PREC>).
constexpr bool one_plane16(int prec) { return prec == DR_PRECISION_BF16 || prec == DR_PRECISION_F16; }
// Option "exact_below" (include/diffroll_amd.h): THE rule of a reverse step's precision.  A step at diffusion step t <
// exact_below runs in exact fp32 whatever mode the engine has selected (prec); every other step runs in that mode.  Keyed
// by the real diffusion step, so it means the same under "sampling_steps"; 0 = off, timesteps = every step exact.  The
// visited t decrease along a chain, so all exact steps lie behind all reduced ones.  Network evaluations that are not
// chain steps (dr_forward, dr_forward_steps) do not ask: they keep the engine's mode.
constexpr int step_precision(int prec, int exact_below, int t) { return t < exact_below ? (int)DR_PRECISION_F32 : prec; }
// what dr_set_option accepts for the name (S = timesteps)
constexpr bool exact_below_ok(int v, int S) { return v >= 0 && v <= S; }
// 16-byte rows of an X tile per 32 input channels: fp32 P4 planes, the three split-bf16 pieces, or one 16-bit plane set
constexpr int x_tile_rows(int prec) { return one_plane16(prec) ? 4 : prec ? 12 : 8; }
// bytes of one packed weight slab (128 rows x 32 channels of one tap)
constexpr size_t weight_slab_bytes(int prec) { return one_plane16(prec) ? 8192 : prec ? 24576 : 16384; }

// frames per block of gemm_kernel<NI, ...>: 64 / 128 (NI = 1 / 2), 96 / 160 (NI = 3 / 5: that many 32-frame MFMA tiles per
// consumer wave, the gated conv only)
inline int gemm_block_frames(int NI) { return (NI == 3 || NI == 5) ? 32 * NI : 64 * NI; }
inline size_t gemm_lds_bytes(int NI, int KS, int taps, int dil, int prec, int epi) {
    const int halo = ((taps - 1) / 2) * dil;
    const int BN = gemm_block_frames(NI);
    const int FW = BN + 2 * halo;
    return (size_t)2 * x_tile_rows(prec) * KS * FW * 16 + (epi == EPI_RES_SKIP ? (size_t)32 * BN * 16 : 0);
}

// Block -> XCD mapping of a per-phase GEMM launch (gemm.hip: block_tile) of MT row tiles x NT frame tiles of BN frames:
// 0 = one weight panel (M tile) per XCD, 1 = the M tiles of a frame tile share an XCD (needs NT % 8 == 0 and more than one
// M tile; a forced tune.xcd_n is ignored elsewhere).  Chosen by the bytes each choice pulls through the XCDs' L2s (what the
// FETCH counters see): with mapping 0 every XCD streams ITS panel once (L2-resident if it fits) and all of X; with mapping 1
// every XCD streams its share of X once and ALL panels - once if the whole weight matrix fits its L2, else once per
// round of concurrently resident frame tiles.  (Until round 3 the rule was "xbytes > wbytes" - tune.xcd_model = 0 - which
// picked mapping 1 for 5-round launches of big convs - 640-frame generation batches - and paid 13.9x the algorithmic traffic.)
inline int pick_xcd_mapping(const PlanKnobs& k, int MT, int NT, int BN, int kchunks, int taps) {
    // weights: MT*128 rows x 32*kchunks*taps floats; activations: NT frame tiles of BN frames x 32*kchunks floats
    const double wbytes = 4.0 * 128.0 * MT * 32.0 * kchunks * taps, xbytes = 4.0 * (double)NT * BN * 32.0 * kchunks;
    if (MT <= 1 || NT % 8 != 0) return 0;
    if (k.xcd_n >= 0) return k.xcd_n;      // A/B experiments
    if (!k.xcd_model) return xbytes > wbytes ? 1 : 0;
    const double l2 = 4.0 * 1024 * 1024, cus_per_xcd = 32.0;
    const double conc = cus_per_xcd / MT < 1.0 ? 1.0 : cus_per_xcd / MT;               // frame tiles resident per XCD (mapping 1)
    const double rounds1 = wbytes <= l2 ? 1.0 : ((NT / 8.0) / conc < 1.0 ? 1.0 : (NT / 8.0) / conc);
    const double cost1 = 8.0 * rounds1 * wbytes + xbytes;
    const double panel = wbytes / MT;
    const double rounds0 = panel <= l2 ? 1.0 : (double)((long)MT * NT + 255) / 256;    // a panel that does not fit is re-streamed per round
    const double cost0 = rounds0 * wbytes + 8.0 * xbytes;
    return cost1 < cost0 ? 1 : 0;
}

// Channels per hand-over of an fp32 gemm_kernel launch, in 32-channel slabs (KS = 1 / 2 / 4).  1x1 GEMMs restage X every
// step: take up to 128 channels per chunk there (fewer hand-overs); EPI_RES_SKIP also keeps its read-modify-write tile in
// LDS, which leaves room for 64 channels at NI = 2.  A forced value (tune.one_ks) is taken where it divides the slabs and
// its X tiles fit the 160 KiB of LDS; elsewhere the unforced choice stands.
inline int pick_one_ks(int taps, int kchunks, int NI, int epi, int forced) {
    int KS = taps != 1 ? 1 : (kchunks % 4 == 0 ? 4 : (kchunks % 2 == 0 ? 2 : 1));
    if (epi == EPI_RES_SKIP && NI == 2 && KS == 4) KS = 2;
    if ((forced == 1 || forced == 2 || forced == 4) && taps == 1 && kchunks % forced == 0 &&
        gemm_lds_bytes(NI, forced, 1, 1, 0, epi) <= 160 * 1024)
        KS = forced;
    return KS;
}

// Item width of the tail kernel's copy of the next step's first-layer conv (its part T4), as gemm_kernel's NI: 1 = 64-frame
// items, 3 = 96.  Rounds over the pair's 2 * gsize blocks (gsize where this step is not guided: dual = 0; gsize = MT x the
// BN-frame tiles of a clip) x frames per item: 64 unless 96 is strictly cheaper or forced (tune.tail_t4 = 3; 1 forces 64).
// The 96-frame body exists with blocked accumulation only (fold).
inline int tail_t4_width(bool fold, int forced, bool dual, int MT, int T, int BN) {
    const long pair_blocks = (dual ? 2L : 1L) * MT * ((T + BN - 1) / BN);
    const long n64 = (long)MT * ((T + 63) / 64), n96 = (long)MT * ((T + 95) / 96);
    const long c64 = (n64 + pair_blocks - 1) / pair_blocks * 64, c96 = (n96 + pair_blocks - 1) / pair_blocks * 96;
    return (fold && forced != 1 && (c96 < c64 || forced == 3)) ? 3 : 1;
}

// THE split-K decision of gemm_kernel launches (the launcher takes it; the engine's tile choice prices a launch with it,
// so the estimate and the launch cannot disagree): for `tiles` output tiles of 128 rows x 64 NI frames, `nchunks` hand-over
// chunks of K (kchunks / KS), a workspace of ws_floats / ws_cnt_n: the number of K slices and the modelled time.
// Model (fp32, fitted to 3..8 guided clips of 125 frames, tools/lab/small_batch_ab.py): equal blocks run in lockstep rounds
// over the 256 CUs - rounds x t_full / ks + exchange, t_full = a full-K tile (MFMA count x 69 cycles at 2.4 GHz), the
// exchange (store, ticket, the last arriver's ordered re-read) ~(4 + ks) us.  Inside one resident round more slices are
// always taken; beyond it a split must win by 3 %.
struct KSplitPlan { int ks; double us; double us_unsplit; };
inline KSplitPlan plan_ksplit(const PlanKnobs& k, long tiles, int nchunks, int kchunks, int taps, int NI, int prec,
                              size_t ws_floats, size_t ws_cnt_n) {
    const int ks_max = k.ksplit_max;
    const long forced_blocks = k.ksplit_blocks;
    const long max_blocks = forced_blocks ? forced_blocks : (prec ? 256 : 2048);
    const int BN = gemm_block_frames(NI);
    const double t_full = (double)kchunks * taps * 16.0 * (BN / 32) * 69.0 / 2400.0;
    auto cost = [&](int ks) {
        return (double)((tiles * ks + 255) / 256) * t_full / ks + (ks > 1 ? 4.0 + ks : 0.0);
    };
    KSplitPlan p{1, cost(1), cost(1)};
    for (int ks = 2; ks <= ks_max && ks <= 16; ks *= 2) {
        if (tiles * ks > max_blocks || nchunks % ks != 0) break;
        if ((size_t)tiles * ks * 128 * BN > ws_floats || (size_t)tiles * 4 > ws_cnt_n) break;
        const double c = cost(ks);
        if (tiles * ks <= 256 || c < 0.97 * p.us) { p.us = std::min(p.us, c); p.ks = ks; }
    }
    return p;
}

// Fused residual stack (stack_kernel<FL>, kernels.h: StackArgs).  FL = block flavour: 1 / 2 / 5 = 128 packed rows x
// 64 / 128 / 160 frames.
inline int stack_tile_frames(int FL) { return FL == 5 ? 160 : 64 * FL; }
// split-bf16 flavour: max over its two phase bodies (conv: S3 X tiles; 1x1: 128-channel S3 X tiles + the 64-frame h / skip tile)
// (the one-plane 16-bit flavours, prec = 2 / 4: the same two bodies on X tiles of a third the rows)
inline size_t stack3_lds_bytes(int FL, int taps, int max_dil, int prec = 1) {
    return std::max(gemm_lds_bytes(FL, 1, taps, max_dil, prec, EPI_GATE), gemm_lds_bytes(1, 4, 1, 1, prec, EPI_RES_SKIP)) + 16;
}
// blocks of one clip evaluation (= one barrier group): M tiles x frame tiles
inline int stack_group_blocks(int FL, int Cp, int T) {
    const int BN = stack_tile_frames(FL);
    return (Cp >> 6) * ((T + BN - 1) / BN);
}
// the conv's double-buffered X tiles + the resident h / skip tile
inline size_t stack_lds_bytes(int FL, int taps, int max_dil) {
    const int BN = stack_tile_frames(FL), halo = ((taps - 1) / 2) * max_dil;
    return (size_t)2 * 8 * (BN + 2 * halo) * 16 + (size_t)32 * BN * 16 + 16;     // + one flag word (16-byte slot)
}

// Tile of a per-phase GEMM launch (launch_tiled, plan.hip).  flavor 0: gemm_kernel (32x32 MFMA) with NI = n (64*n frames
// per block; 96 / 160 for n = 3 / 5); 1: gemm16_kernel (16x16 MFMA) with NJ = n (32*n frames per block, fp32 hot kernels
// only); 2: pw_kernel with NW = n; 3: pwk_kernel with NW = n.
struct Tile { int flavor, n; };

// Frame-tile choice for a GEMM of MT row tiles over NB samples of T frames.  Cost = (block rounds over the 256 CUs, one
// block per CU: LDS / 512-thread blocks) x (frames per block); 16x16 tiles carry a small penalty (more operand reads per
// MFMA), 128-frame 32x32 tiles win ties (half the weight traffic per MFMA).
// The 32x32 conv kernels may be cut in K into more blocks than CUs (launch_gemm's split-K cost model: equal blocks run
// in lockstep rounds, the exchange costs ~(4 + ks) us): a width whose tile count fills the chip unevenly can still win
// that way - 2 guided 640-frame clips: 320 64-frame tiles cut 4x, 3209 vs 3592 us per step on 224 96-frame tiles of
// the 16x16 kernel, which has no split.  Cost in the units of pick_tile (block rounds x frames per block x penalty) of
// the best split that needs MORE than one resident round, with a 5 % handicap; 1e30 if there is none.
inline double split_cost(const PlanKnobs& k, long blocks, int bn, double pen, int MT, int taps) {
    const int nchunks = 2 * MT;                                                  // 32-channel chunks of K (convs: KS = 1)
    // the launcher's own decision and price (plan_ksplit): what it WILL do with this launch
    const KSplitPlan p = plan_ksplit(k, blocks, nchunks, nchunks, taps, bn / 64, 0, SK_WS_FLOATS, SK_CNT_N);
    if (p.ks <= 1 || blocks * p.ks <= 256) return 1e30;                          // (one resident round: priced by the caller)
    const double us_per_frame = p.us_unsplit / ((double)((blocks + 255) / 256) * bn);      // us of one frame column of a full-K tile
    return 1.05 * pen * p.us / us_per_frame;
}
// wide32: the 96 / 160-frame flavours of the 32x32 conv kernel (n = 3 / 5; fp32 gated conv with blocked accumulation) may be
// used - they take the place of the 16x16 kernels of those widths, which have no blocked form (option blocked_accumulation = 2)
inline Tile pick_tile(const PlanKnobs& k, int MT, int NB, int T, int taps, int dil, int prec, int epi, bool allow16,
                      bool wide32 = false) {
    const int forced = k.tile;                          // A/B experiments: 3202, 1605, ... (if it fits)
    const int halo = ((taps - 1) / 2) * dil;
    struct Cand { int flavor, n, bn; double pen; };
    const Cand cands[] = {{0, 2, 128, 1.0}, {0, 5, 160, 1.04}, {1, 5, 160, 1.04}, {0, 3, 96, 1.04}, {1, 3, 96, 1.04}, {0, 1, 64, 1.0}};
    auto feasible = [&](const Cand& c) {
        if (c.flavor == 1 && (!allow16 || prec != 0)) return false;
        if (c.flavor == 0 && (c.n == 3 || c.n == 5) && (!wide32 || prec != 0 || epi != EPI_GATE || taps == 1)) return false;
        const int ks = (taps == 1) ? 2 : 1;
        const size_t lds = (c.flavor == 0)
            ? gemm_lds_bytes(c.n, (taps == 1 && c.n == 1) ? 4 : ks, taps, dil, prec, epi)
            : (size_t)2 * 8 * ks * (c.bn + 2 * halo) * 16 + (epi == EPI_RES_SKIP ? (size_t)32 * c.bn * 16 : 0);
        return lds <= 160 * 1024;
    };
    if (forced) {
        const int ff = forced / 100 == 16 ? 1 : 0, fn = forced % 100;
        for (const Cand& c : cands)
            if (c.flavor == ff && c.n == fn && feasible(c)) return Tile{ff, fn};
    }
    Tile best{0, 1};
    double best_cost = 1e30;
    for (const Cand& c : cands) {
        if (!feasible(c)) continue;
        const long blocks = (long)MT * NB * ((T + c.bn - 1) / c.bn);
        double cost = (double)((blocks + 255) / 256) * c.bn * c.pen;
        if (c.flavor == 0 && c.n <= 2 && prec == 0 && epi == EPI_GATE && taps > 1 && allow16)
            cost = std::min(cost, split_cost(k, blocks, c.bn, c.pen, MT, taps));
        if (cost < best_cost - 1e-9) { best_cost = cost; best = Tile{c.flavor, c.n}; }
    }
    return best;
}
inline int pick_ni(const PlanKnobs& k, int MT, int NB, int T, int taps, int dil, int prec = 0) {
    return pick_tile(k, MT, NB, T, taps, dil, prec, EPI_GATE, false).n;
}
// tile of the 1x1 residual/skip GEMM: flavor 2 = operands direct from L2 (pw_kernel), fp32 only
// (kchunks: 32-channel slabs of K; 0 = MT tiles cover all rows); flavor 3 = pwk_kernel, the K loop split over the block's waves
inline Tile pick_pointwise_tile(const PlanKnobs& k, int MT, int NB, int T, int prec, int kchunks = 0) {
    if (prec) return Tile{0, 1};
    const int pw = k.pw, pw_ni = k.pw_nw;      // A/B experiments: 0 = LDS-staged kernels / force 32*NW-frame blocks
    if (!pw) return pick_tile(k, MT, NB, T, 1, 1, 0, EPI_RES_SKIP, true);
    // tune.pwk = 2 (tests): pwk_kernel wherever it exists (K slabs a multiple of 4), whatever the fill; tune.pw_nw = 1 / 2
    // then names ITS width
    const bool pwk_ok = (kchunks ? kchunks : 2 * MT) % 4 == 0;
    const int pwk_nw = (long)4 * MT * NB * ((T + 31) / 32) <= 512 ? 1 : 2;
    if (k.pwk == 2 && pwk_ok && pw_ni <= 2) return Tile{3, pw_ni ? pw_ni : pwk_nw};
    if (pw_ni) return Tile{2, pw_ni};
    // launches that cannot fill half the chip even with 64-frame blocks (single clips): 32-row x 32-frame tiles whose
    // four waves split K in-block (flavor 3, pwk_kernel: 256 blocks at config 1, 13.9 -> 8 us per launch); without it
    // (tune.pwk = 0, K splitting pinned off, a channel count that is not a multiple of 128) the LDS-staged kernel with
    // split-K through the workspace.  (Measured and rejected in round 3: 32-frame blocks of the direct kernel instead -
    // 64 blocks at config 1 - 35.2 vs 34.0 ms per chain.)
    if ((long)MT * NB * ((T + 63) / 64) <= 128) {
        if (k.pwk && k.ksplit_max > 1 && pwk_ok) return Tile{3, pwk_nw};
        return pick_tile(k, MT, NB, T, 1, 1, 0, EPI_RES_SKIP, true);
    }
    // cost = block rounds over the 256 CUs x frames per block; 64-frame blocks carry a measured 7 % penalty
    // (twice the operand loads per MFMA)
    struct Cand { int nw; double pen; };
    const Cand cands[] = {{4, 1.0}, {5, 1.0}, {3, 1.02}, {2, 1.07}};
    Tile best{2, 4};
    double best_cost = 1e30;
    for (const Cand& c : cands) {
        const int bn = 32 * c.nw;
        const long blocks = (long)MT * NB * ((T + bn - 1) / bn);
        const double cost = (double)((blocks + 255) / 256) * bn * c.pen;
        if (cost < best_cost - 1e-9) { best_cost = cost; best = Tile{2, c.nw}; }
    }
    return best;
}

// One network evaluation as run_network sees it: NB samples (the first n_cond conditional) of T frames, inputs taken
// modulo bmod, and the engine's geometry and options.
struct NetShape {
    int NB, n_cond, bmod, T;
    int Cp, L, K, max_dil;      // padded channels, residual layers, kernel size, largest dilation
    int prec;                   // 0 exact fp32, 1 split-bf16, 2 one-pass bf16, 4 one-pass f16 (DR_PRECISION_*)
    int n_cus;                  // CUs of the device (0: unknown - never fused)
    int fuse;                   // FusedMode::active(): 0 one launch per phase, 1 fused where the cost model likes it, 2 fused regardless
    int opt_blocked, opt_tail;  // options "blocked_accumulation" and "fused_tail"
    bool has_tsel;              // per-sample diffusion steps (dr_forward_steps)
    bool tail_offered;          // run_step offered the fused step (TailPlan)
};
struct NetPlan {
    int stack_fl = 0;           // fused residual stack flavour (1 / 2 / 5); 0 = one launch per phase
    int stack_chunks = 1;       // sample chunks the evaluation is launched in (one fused launch each)
    int stack_from = -1;        // first phase run by the fused kernel (-1: none; 1: layer 0's conv is a launch of its own)
    bool dual0 = false;         // classifier-free pairs (sample b, b + bmod): layer 0's conv is contracted once per pair
    bool fold = false;          // blocked accumulation in the fused conv phases (and the tail kernel's copy of layer 0's conv)
    bool fused_step = false;    // the evaluation is ONE fused launch that the tail kernel may follow
    bool use_tail = false;      // ... and run_step offered it: the rest of the step is the tail kernel
    int mode = DR_MODE_PER_PHASE;
};
inline NetPlan plan_network(const NetShape& s, const PlanKnobs& k) {
    const int NB = s.NB, T = s.T, Cp = s.Cp, L = s.L, prec = s.prec;
    const bool dual0 = (s.bmod > 0 && NB == 2 * s.bmod && s.n_cond == s.bmod);
    // ---- fused residual stack: the layers as ONE persistent launch when all its blocks are resident at once ----
    // (exact fp32 only; the first layer's conv stays a launch of its own under classifier-free guidance, where it
    // is contracted once per (conditional, unconditional) pair)
    int stack_from = -1;                   // first phase run by the fused kernel (-1: none)
    int stack_ni = 0, stack_chunks = 1;    // flavour, and how many sample chunks the evaluation is launched in
    bool fused_step = false;
    // (the split-bf16 and one-pass bf16 / f16 precisions have their own flavours of the kernel: 128-channel chunks in the 1x1 phases
    // need Cp % 128 == 0)
    const int stack3 = k.stack3;
    const int fuse = s.fuse;
    if (fuse && (prec == 0 || (stack3 && Cp % 128 == 0)) && L <= DR_STACK_MAX_LAYERS && s.n_cus > 0) {
        // Flavours 1 / 2 / 5 (128 packed rows x 64 / 128 / 160 frames per block) are chosen automatically; tune.stack_fl = n
        // pins one (tests / measurements); tune.stack_fl = -5 excludes the 160-frame flavour (its A/B).  Flavour 5 exists in
        // exact fp32 with blocked accumulation only (its per-phase twin is gemm_kernel<5>, which has no other form).
        const int fl_force = k.stack_fl;
        // A launch must be ONE resident round (groups spin on each other), so an evaluation with more samples than
        // fit is launched in balanced CHUNKS of samples, one fused launch after the other (samples are independent).
        // Cost model per frame-tile width, as pick_tile's: (block rounds over the CUs) x (frames per block) x a
        // per-width penalty (64-frame blocks load twice the weight fragments per MFMA; 16x16 tiles more operands) -
        // for the fused kernel rounds = chunks, minus what fusing was measured to save; fused wins if its best width
        // costs no more than the per-phase launches' best width.
        const int MT = Cp / 64;
        auto per_phase_cost = [&]() {
            double best = 1e30;
            const struct { int bn; double pen; } cands[] = {{64, 1.0 / 0.93}, {96, 1.04}, {128, 1.0}, {160, 1.04}};
            for (const auto& c : cands) {
                const long blocks = (long)MT * NB * ((T + c.bn - 1) / c.bn);
                best = std::min(best, (double)((blocks + s.n_cus - 1) / s.n_cus) * c.bn * c.pen);
                // (the 32x32 widths may split K beyond one round: 20 guided clips, 640 64-frame tiles cut 2x, 6166 us
                // per step against 7074 as three fused launches of 13-14 evaluations)
                if (c.bn == 64 || c.bn == 128) best = std::min(best, split_cost(k, blocks, c.bn, c.pen, MT, s.K));
            }
            return best;
        };
        double best = 1e30;
        for (int fl : {1, 2, 5}) {
            if (fl_force > 0 && fl != fl_force) continue;
            if (fl == 5 && (fl_force == -5 || prec != 0 || s.opt_blocked < 2)) continue;
            const int bn = stack_tile_frames(fl);
            const long gsize = stack_group_blocks(fl, Cp, T);                           // blocks per sample
            const long cap = std::min<long>(s.n_cus, 1024) / gsize;                     // samples per launch
            if (cap < 1 || (prec ? stack3_lds_bytes(fl, s.K, s.max_dil, prec) : stack_lds_bytes(fl, s.K, s.max_dil)) > 160 * 1024) continue;
            const long chunks = (NB + cap - 1) / cap;
            if ((NB + chunks - 1) / chunks > STACK_GROUPS) continue;
            // (what fusing saves is per-launch overhead, which the per-phase launches amortise over their rounds:
            // measured +2.5 % at one round, +1.1 % at two (B = 32 guided clips per GPU), nothing at four)
            const double cost = (1.0 - 0.025 / chunks) * chunks * bn * (fl == 1 ? 1.0 / 0.93 : fl == 5 ? 1.04 : 1.0);
            // (a single launch that leaves more than a fifth of the CUs idle is better served by the per-phase kernels'
            // split-K, which this cost model does not see: they cut the same work into many short blocks that balance
            // over all CUs - 8 evaluations x 125 frames (half the chip): 1365 vs 2422 us per step, 10 / 12 evaluations
            // (62 / 75 %): 1994 / 2022 vs 2425, 14 (87 %): 2526 vs 2424; fuse == 2 fuses regardless: tests)
            const bool ok = fuse == 2 || (chunks == 1 ? 5 * NB * gsize > 4 * (long)s.n_cus : true);
            if (ok && cost < best) { best = cost; stack_ni = fl; stack_chunks = (int)chunks; }
        }
        if (stack_ni && fuse != 2 && best > per_phase_cost()) stack_ni = 0;
        if (stack_ni) stack_from = dual0 ? 1 : 0;
        // fused step (option "fused_tail"): everything behind the stack launch - skip / output projection, update, and
        // for a chain the next step's input projection and (guided) shared first-layer conv - is one tail launch,
        // when the evaluation is ONE fused launch of the 32x32-MFMA flavours
        fused_step = stack_ni && stack_chunks == 1 && s.opt_tail && !s.has_tsel && prec == 0;      // (the tail kernel is fp32 only)
    }
    const bool use_tail = fused_step && s.tail_offered;
    const int mode = use_tail ? DR_MODE_FUSED_STACK_TAIL : (stack_from >= 0 ? DR_MODE_FUSED_STACK : DR_MODE_PER_PHASE);
    // (the 128-frame flavour keeps one fp32 chain per output under blocked_accumulation = 1; every other one folds)
    const bool fold = stack_ni != 2 || s.opt_blocked >= 2;
    return NetPlan{stack_ni, stack_chunks, stack_from, dual0, fold, fused_step, use_tail, mode};
}

// Guidance interval (options "guidance_t_min" / "guidance_t_max", include/diffroll_amd.h): a reverse step of a guiding
// sampler at diffusion step t runs both evaluations and combines them with the caller's w iff lo <= t <= hi; every other
// step is the w = 0 step - the conditional evaluation alone, consumed unchanged.  w == 0 is the empty interval.
struct GuidanceInterval {
    int lo = 0, hi = -1;        // as set; hi = -1: timesteps - 1
    int hi_eff(int S) const { return hi < 0 ? S - 1 : hi; }
    bool empty(int S) const { return lo > hi_eff(S); }
};
// what dr_set_option accepts for the two names (S = timesteps)
inline bool guidance_value_ok(bool is_max, int v, int S) { return v < S && v >= (is_max ? -1 : 0); }
inline bool step_guided(const GuidanceInterval& g, int S, bool w_zero, int t) {
    return !w_zero && t >= 0 && g.lo <= t && t <= g.hi_eff(S);
}
// The evaluation batch of one reverse step: NB network evaluations of B rolls, the first n_cond conditional; dual = the
// step is guided (rows b and b + B evaluate the same x_t: NB = 2 B).
struct StepEval { int NB = 0, n_cond = 0; bool dual = false; };
// (NB, n_cond: the sampler's own shape - sampler_shape, plan.hip; a sampler that does not guide keeps it at every step)
inline StepEval step_eval(int NB, int n_cond, int B, bool guided) {
    if (NB != 2 * B) return StepEval{NB, n_cond, false};
    return guided ? StepEval{NB, n_cond, true} : StepEval{B, B, false};
}
// Guidance stride (option "guidance_stride", include/diffroll_amd.h): of the steps that guide, numbered k = 0, 1, 2, ... in
// the order the chain visits them from its start position, the one with k % n == 0 and step t == 0 REFRESH - both
// evaluations, as without the option - and every other one REUSES the guidance update the last refresh stored: the
// conditional evaluation alone, the shape of a step outside the interval.  n <= 1: off, every guided step refreshes.
inline bool stride_refreshes(int n, int k, int t) { return n <= 1 || k % n == 0 || t == 0; }
// this step's shape and its successor's in the chain (next_t < 0: the chain ends here, `next` is all zero); reuse_now /
// reuse_next: the step guides and reuses under "guidance_stride" (the caller counts k: chain_tables.h, guided_ordinal)
struct StepShapes { StepEval now, next; };
inline StepShapes plan_step(int NB, int n_cond, int B, const GuidanceInterval& g, int S, bool w_zero, int t, int next_t,
                            bool reuse_now = false, bool reuse_next = false) {
    StepShapes p;
    p.now = step_eval(NB, n_cond, B, step_guided(g, S, w_zero, t) && !reuse_now);
    if (next_t >= 0) p.next = step_eval(NB, n_cond, B, step_guided(g, S, w_zero, next_t) && !reuse_next);
    return p;
}

}  // namespace dr
