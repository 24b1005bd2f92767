// Host side of the DiffRoll sampling engine, shared declarations: the engine object behind the C-ABI handle and the
// helpers the four host translation units use -
//   pack.hip       weight packing, staged uploads, dr_set_param / dr_set_tables / dr_commit (+ the split-bf16 packings)
//   plan.hip       the launch sequences of one evaluation and one reverse step (their planning: launch_plan.h)
//   abi.hip        the C-ABI of include/diffroll_amd.h: life cycle, front-end, forward / step / sample (hipGraph), time-outs
//                  (the chain's steps, coefficient rows, start position, history rule and window table: chain_tables.h;
//                  the owner of the captured chain - graph, executable, key, capture stream: captured_chain.h)
//   debug_abi.hip  measurement and checker entry points (dr_bench_*, dr_debug_*, dr_profile_*)
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/diffroll_amd_debug.h"      // (includes the boundary, diffroll_amd.h)
#include "captured_chain.h"
#include "chain_tables.h"
#include "device_buffer.h"
#include "fused_mode.h"
#include "kernels.h"

namespace drh {
using namespace dr;

extern thread_local std::string g_create_error;      // dr_last_error(NULL): errors of calls that have no engine

struct LayerW {
    float* conv_w = nullptr;     // packed (paired rows) [MTc][kch][k] slabs
    float* conv_b = nullptr;     // packed-row bias (conditional samples; cond tensor carries bc)
    float* conv_b_u = nullptr;   // packed-row bias for unconditional samples: b_conv + (bc - sum_m Wc)
    float* conv_b_z = nullptr;   // ... for spec == 0 samples (cfdg_ddim_x0's second branch): b_conv + bc
    float* conv_w3 = nullptr;    // split-bf16 ("S3") packing of conv_w  [MTc][kch][k] slabs of 24 KiB
    float* out_w3 = nullptr;     // split-bf16 packing of out_w
    float* conv_wb = nullptr;    // one-pass bf16 packing of conv_w  [MTc][kch][k] slabs of 8 KiB
    float* out_wb = nullptr;     // one-pass bf16 packing of out_w
    float* conv_wh = nullptr;    // one-pass f16 packing of conv_w: bf16's slabs and index order, IEEE binary16 values
    float* out_wh = nullptr;     // one-pass f16 packing of out_w
    // the packing of the two hot GEMMs that precision `prec` (DR_PRECISION_*) contracts
    const float* conv_w_of(int prec) const { return prec == DR_PRECISION_F16 ? conv_wh : prec == DR_PRECISION_BF16 ? conv_wb : prec ? conv_w3 : conv_w; }
    const float* out_w_of(int prec) const { return prec == DR_PRECISION_F16 ? out_wh : prec == DR_PRECISION_BF16 ? out_wb : prec ? out_w3 : out_w; }
    float* out_w = nullptr;      // packed (natural halves) 1x1
    float* out_b = nullptr;
    float* cond_w = nullptr;     // packed (paired rows) conditioner 1x1
    float* cond_b = nullptr;
    int dil = 1;
};

// The value options a chain is run under (dr_set_option; each name's accepted values and what setting it drops or rebuilds:
// abi.hip, set_option).  dr_engine::opt holds them as set; a captured chain's key holds effective() of them.
struct ChainOptions {
    int steps = 0;                      // option "sampling_steps": n of a respaced chain; 0 (and S) = every step
    int win_O = 0;                      // option "window_overlap": > 0 = the B rolls of dr_step / dr_sample are consecutive windows of
                                        // one recording sharing that many frames (UpdateArgs::win); 0 = independent clips
    int win_blend = 0;                  // option "window_blend": what a frame shared by two windows takes of their predictions - 0 the mean,
                                        // 1 the linear cross-fade, 2 the hand-over (update_quad.h: blend_quad); read only while win_O > 0
    int draws = 1;                      // option "draws": D > 1 = the B rolls are D draws of the B / D clips of the last dr_frontend, draw-major
    int draw_G = 0;                     // option "draw_stride": Philox key distance between two draws of a clip; 0 = the clips of the batch
    dr::GuidanceInterval guid;          // options "guidance_t_min" / "guidance_t_max": the steps a guiding sampler guides (launch_plan.h)
    // option "solver_order": 0 = the sampler's own update; 1 / 2 = the x0-prediction samplers integrate their prediction
    // with the first-order exponential integrator in lambda / DPM-Solver++ (2M) (update_quad.h: solver_quad)
    int solver = 0;
    // option "solver_noise": 1 = the solver's stochastic form (SDE-DPM-Solver++): other rows 0 / 1 / 4, and mode 5 adds c4 z.
    // Stored always, read only while solver != 0
    int solver_noise = 0;
    // option "start_step": the visited step a chain begins at (d_x on entry is x at that step); -1 = the chain's first
    // visited step.  option "start_noise": 1 = d_x on entry to dr_sample is a clean roll, diffused to that step by the
    // chain's first node (update.hip: diffuse_kernel)
    int start = -1, start_noise = 0;
    // option "x0_clip": 0 = off; 1 / 2 = the x0-prediction samplers clamp the prediction their update consumes to [0, 1] /
    // [-1, 1] (update_quad.h: clamp_quad); the epsilon samplers refuse a non-zero value (abi.hip: check_options)
    int x0_clamp = 0;
    // option "x0_threshold": 0 = off; 5000 .. 10000 = the percentile (1 / 10000) of dynamic thresholding, a refinement of
    // "x0_clip" (refused without it: abi.hip: check_options).  A thresholded step offers no tail plan: the stack launch, the
    // head projections, the threshold launches (threshold.hip) and update_thresh_kernel (plan.hip: run_step)
    int x0_thresh = 0;
    // option "cfg_rescale": 0 = off; 1 .. 10000 = phi (1 / 10000) of the guidance rescale.  A step that guides under it offers
    // no tail plan either: the statistics launch (rescale.hip) behind the head projections, then the threshold launches'
    // rescaled forms where "x0_threshold" is set, then update_rescale_kernel (plan.hip: run_step).  A step that does not
    // guide - another sampler, w = 0, outside the guidance interval - does not read it
    int cfg_rescale = 0;
    // options "cfg_project" / "cfg_norm": 0 = off; rho = cfg_project / 10000 of the update's component parallel to the
    // conditional prediction is removed, r = cfg_norm / 10000 bounds the rms of c - u (adaptive projected guidance without
    // momentum).  A step that guides under either offers no tail plan: the statistics launch (project.hip) behind the head
    // projections, then update_project_kernel (plan.hip: run_step).  Refused beside "x0_threshold" and "cfg_rescale"
    // (abi.hip: check_options); a step that does not guide reads neither
    int cfg_project = 0, cfg_norm = 0;
    // option "cfg_momentum": 0 = off; beta = cfg_momentum / 10000, -9999 .. 9999, the momentum of adaptive projected guidance:
    // a guided step under "cfg_project" / "cfg_norm" runs the statistics in their momentum form and update_momentum_kernel
    // (momentum.hip) over the engine's state (dr_engine::momentum).  Refused while both partners are 0 (abi.hip: check_options)
    int cfg_momentum = 0;
    // option "guidance_stride": 0 / 1 = off; n = 2 .. 64: of the steps that guide, numbered in chain order from the chain's
    // start position, every n-th one and step 0 refresh - both evaluations, and d = y - c stored per element into the engine's
    // state (dr_engine::stride_d) - and the others reuse: the conditional evaluation alone, y = c + d (launch_plan.h:
    // stride_refreshes; stride.hip: update_stride_kernel).  A guided step under it offers no tail plan.  Refused beside
    // "x0_threshold", "cfg_rescale", "cfg_project", "cfg_norm" and "cfg_momentum", and by a sampler that does not guide
    // (abi.hip: check_options)
    int guid_stride = 0;
    // option "exact_below": 0 = off; v = 1 .. timesteps: a reverse step at diffusion step t < v runs in exact fp32 whatever
    // dr_set_precision selected (launch_plan.h: step_precision; plan.hip: run_step asks once per step).  Inert under
    // DR_PRECISION_F32 (abi.hip: chain_key takes it out of the key there)
    int exact_below = 0;
    bool operator==(const ChainOptions& o) const {
        return steps == o.steps && win_O == o.win_O && win_blend == o.win_blend && draws == o.draws && draw_G == o.draw_G && guid.lo == o.guid.lo &&
               guid.hi == o.guid.hi && solver == o.solver && solver_noise == o.solver_noise && start == o.start &&
               start_noise == o.start_noise && x0_clamp == o.x0_clamp && x0_thresh == o.x0_thresh && cfg_rescale == o.cfg_rescale &&
               cfg_project == o.cfg_project && cfg_norm == o.cfg_norm && cfg_momentum == o.cfg_momentum && guid_stride == o.guid_stride &&
               exact_below == o.exact_below;
    }
};
// Which stages between the network and the update run - the one statement of it, for a step and for a chain: the threshold
// launches of "x0_threshold" (the x0-prediction samplers, under the range "x0_clip" names), the statistics launch of
// "cfg_rescale", that of "cfg_project" / "cfg_norm", and its momentum form under "cfg_momentum".  guides: asked about a step,
// the step runs the unconditional evaluation; asked about a chain, a step of it can - a guiding sampler, w != 0.
// stride: the step guides under "guidance_stride" - a refresh or a reuse (`guides` then says that the step is one of those
// that guide: a reuse runs no unconditional evaluation, and check_options has refused every other stage beside it).
struct Stages { bool thresh, rescale, project, momentum, stride; };
inline Stages stages_of(const ChainOptions& o, bool x0_sampler, bool guides) {
    Stages s{};
    s.thresh = o.x0_thresh != 0 && o.x0_clamp != 0 && x0_sampler;
    s.rescale = o.cfg_rescale != 0 && guides;
    s.project = (o.cfg_project != 0 || o.cfg_norm != 0) && guides;
    s.momentum = s.project && o.cfg_momentum != 0;
    s.stride = o.guid_stride > 1 && guides;
    return s;
}
// The options as a chain sees them - what its captured graph bakes in, so what its key compares.  A value that is inert
// under the others does not make another chain: "draw_stride" counts only under "draws" > 1, "solver_noise" only under
// a solver order, "window_blend" only under "window_overlap", the interval only for a sampler that guides (hi resolved); start_t is "start_step" resolved to the
// step the chain visits first (chain_tables.h: start_position); "cfg_rescale", "cfg_project", "cfg_norm", "cfg_momentum" and "guidance_stride" (whose 0 and 1 are one value) count only for the stages a step of the
// chain can run (stages_of) - a sampler that guides, at a weight that is not 0 (w_zero: GraphKey::w_zero, a chain of conditional evaluations alone).
// ("exact_below" counts only under a reduced precision, which this function does not know: abi.hip, chain_key)
inline ChainOptions effective(ChainOptions o, bool guiding, int S, int start_t, bool w_zero) {
    if (o.draws <= 1) o.draw_G = 0;
    if (o.solver == 0) o.solver_noise = 0;
    if (o.win_O <= 0) o.win_blend = 0;
    o.guid = guiding ? dr::GuidanceInterval{o.guid.lo, o.guid.hi_eff(S)} : dr::GuidanceInterval{};
    const Stages s = stages_of(o, true, guiding && !w_zero);      // (no step of the chain reads the values of a stage none of them runs)
    if (!s.rescale) o.cfg_rescale = 0;
    if (!s.project) o.cfg_project = o.cfg_norm = 0;
    if (!s.momentum) o.cfg_momentum = 0;
    if (!s.stride) o.guid_stride = 0;
    o.start = start_t;
    return o;
}
// the samplers whose network output is the x0 prediction (DR_SAMPLER_* 0-5); the others predict epsilon
inline bool predicts_x0(int sampler) { return !(sampler >= DR_SAMPLER_DDPM_EPS && sampler <= DR_SAMPLER_DDIM2DDPM_EPS); }

// What a captured chain bakes in; the held chain is replayed while the key of the call equals the key it was captured
// under, and is stale - waited for, destroyed and captured again by dr_sample, nowhere else - once it does not.  By
// value: sampler, shape, the engine's work buffer and the injected-noise address (test mode).  Seed, batch offset and
// guidance weight live in the DynParams device block; the caller's roll buffer is copied into / out of the work buffer
// around the launch.
struct GraphKey {
    int sampler = -1, B = 0, T = 0;
    float* x = nullptr;
    const float* noise = nullptr;
    bool w_zero = false;        // guidance weight 0 captures a different (conditional-only) chain
    // ... and the effective options: the draw layout of the update's Philox keys, which steps run the unconditional
    // evaluation, how the prediction is integrated, clamped and thresholded, where the chain begins.  A chain captured
    // under another value is simply not replayed, and a façade that sets them around every call replays one graph.
    ChainOptions opt;
    // Everything else, by generation: the engine's own (dr_engine::baked, moved by stale()) and the process-wide one of
    // the tune.* knobs (kernels.h: tuning_epoch(), moved by any engine on any thread)
    unsigned baked = 0, tuning = 0;
    // A captured chain also bakes the clip count of the conditioner tensors (GemmArgs::c_n and the per-layer offsets
    // l * fe_B * 2 Cp T): dr_frontend calls stale() when fe_B changes, the key keeps that from being load-bearing.
    int fe_B = 0;
    const float* hist = nullptr;              // the history buffer of solver order 2 (null: order < 2; the parity is baked per node)
    const unsigned* thresh_work = nullptr;    // the work buffer the threshold launches point into - a buffer that grew since is another chain
    const unsigned* stats_work = nullptr;     // ... and the one the statistics launch of "cfg_rescale" or "cfg_project" / "cfg_norm" points into, likewise
    const float* momentum = nullptr;          // the state of "cfg_momentum" (null: off; "starts" is baked per node)
    const float* stride = nullptr;            // the state of "guidance_stride" (null: off; refresh / reuse is baked per node)
    bool operator==(const GraphKey& o) const {
        return sampler == o.sampler && B == o.B && T == o.T && x == o.x && noise == o.noise && w_zero == o.w_zero &&
               opt == o.opt && baked == o.baked && tuning == o.tuning && fe_B == o.fe_B && hist == o.hist &&
               thresh_work == o.thresh_work && stats_work == o.stats_work && momentum == o.momentum && stride == o.stride;
    }
};
using Chain = CapturedChain<GraphKey>;      // the captured reverse chain and its owner (captured_chain.h)

// The synchronisation words of the persistent kernels (stack_kernel, tail kernel) in one device allocation, plus the
// time-out flag in host-mapped memory: every later API call sees it without a synchronisation and fails loudly instead of
// returning rolls computed from a broken hand-off.
struct StackSync {
    // layout of `mem`, in words: [bar][tail bar][tail pair bar] 4 * STACK_GROUPS each, {arrivals, departures, generation, -}
    // per group (the first two zero between launches: re-armed in-kernel); [xid] 1024 (generation, XCC id) tags published
    // by the blocks of the last launch, one per block; [derr] 16, the time-out flag in device memory (what the kernels poll /
    // test at launch start); [ready] STACK_GROUPS, the tail kernel's per-window ready words (TailArgs::ready)
    static constexpr size_t G4 = (size_t)4 * STACK_GROUPS, XID = 3 * G4, DERR = XID + 1024, READY = DERR + 16,
                            WORDS = READY + STACK_GROUPS;
    struct HostFree { void operator()(volatile unsigned* p) const { (void)hipHostFree((void*)p); } };
    DevBuf<unsigned> mem;
    std::unique_ptr<volatile unsigned, HostFree> err_host;
    unsigned* err = nullptr;            // device address of *err_host
    unsigned* bar() const { return mem; }
    unsigned* tail_bar() const { return mem + G4; }
    unsigned* tail_pbar() const { return mem + 2 * G4; }
    unsigned* xid() const { return mem + XID; }
    unsigned* derr() const { return mem + DERR; }
    unsigned* ready() const { return mem + READY; }
    // every word to its between-launches value, both flags lowered (also after a barrier time-out, device idle)
    hipError_t clear() {
        hipError_t st = hipMemset(mem, 0, WORDS * sizeof(unsigned));
        if (st == hipSuccess) st = hipMemset(xid(), 0xFF, 1024 * sizeof(unsigned));      // no tag of a launch ever equals 0xFFFFFFFF
        if (st == hipSuccess) *err_host = 0;
        return st;
    }
    // (`mem` is left empty unless everything succeeded: the next commit tries again)
    hipError_t init() {
        void *hf = nullptr, *df = nullptr;
        hipError_t st = hipHostMalloc(&hf, 64, hipHostMallocMapped);
        if (st != hipSuccess) return st;
        err_host.reset((volatile unsigned*)hf);
        memset(hf, 0, 64);
        if ((st = hipHostGetDevicePointer(&df, hf, 0)) != hipSuccess) return st;
        err = (unsigned*)df;
        if ((st = mem.ensure(WORDS, false)) == hipSuccess && (st = clear()) != hipSuccess) mem.reset();
        return st;
    }
};

// dr_profile_*: the launches of the dominant kernel are bracketed by pairs of events, one pair per timed launch
struct EventPair {
    hipEvent_t first = nullptr, second = nullptr;
    EventPair() = default;
    ~EventPair() {
        if (first) (void)hipEventDestroy(first);
        if (second) (void)hipEventDestroy(second);
    }
    EventPair(EventPair&& o) noexcept : first(o.first), second(o.second) { o.first = o.second = nullptr; }      // (move-only)
    hipError_t create() {
        hipError_t st = hipEventCreate(&first);
        return st == hipSuccess ? hipEventCreate(&second) : st;
    }
};
struct Profile {
    bool on = false;
    std::vector<EventPair> events;      // created by the first dr_profile_enable: one pair per (step, layer)
    size_t used = 0;                    // pairs recorded since the last dr_profile_read
    int64_t launches = 0;
    double ms = 0.0;
    double flops = 0.0;                 // algorithmic FLOPs of the timed launches
    std::string name;
};

}  // namespace drh

struct dr_engine {
    dr_config cfg{};
    int C = 0, Cp = 0, L = 0, K = 0, S = 0, NM = 0;
    int max_dil = 1;                     // the largest dilation of the residual layers
    int n_bins = 0, bins_p = 0;          // n_fft/2+1 and its 64-multiple padding
    std::string err;
    std::map<std::string, std::vector<float>> params;
    std::vector<float> h_emb, h_coef;
    std::vector<float> h_win, h_fb;      // optional caller-built front-end tables (dr_set_frontend_tables)
    float h_win_norm = 0.f;
    bool committed = false;

    // device constants
    drh::DevBuf<float> d_coef;   // (DR_COEF_FAMILIES, S, 5)
    drh::DevBuf<float> d_dtab;   // (S, L, Cp)   hoisted diffusion_projection(diffusion_embedding(t))
    std::vector<drh::LayerW> layers;
    float *in_w = nullptr, *in_b = nullptr, *skip_w = nullptr, *skip_b = nullptr, *outp_w = nullptr, *outp_b = nullptr;
    float *dft_w = nullptr, *mel_w = nullptr;
    float *fft_win = nullptr, *fft_tw = nullptr;     // FFT front-end: window (n_fft), roots of unity (n_fft complex)
    float fft_norm = 1.f;                            // the spectrum is divided by it (normalized=True)
    bool use_fft = false;
    std::vector<drh::DevBuf<float>> consts;   // what layers, in_w, ... point into (replaced by the next commit)

    // activation workspace (sized for ws_NB samples x ws_T frames)
    int ws_NB = 0, ws_T = 0;
    // split-K workspace (partials) and ticket counters, see gemm_kernel (sizes SK_WS_FLOATS / SK_CNT_N: launch_plan.h)
    drh::DevBuf<float> sk_ws;
    drh::DevBuf<unsigned> sk_cnt;
    drh::DevBuf<float> h, hd, g, skip, tmp, x0buf;
    drh::DevBuf<float> xwork;              // the captured chain runs in place on this roll buffer (not the caller's)
    drh::DevBuf<float> hd3, g3;            // split-bf16 (S3) versions of hd and g: 1.5x the fp32 size; the one-plane 16-bit modes
                                           // (bf16, f16) use the first third - only one mode is active at a time
    int prec = 0;                          // 0: exact fp32 MFMA, 1: split-bf16 (bf16x3, 6 products), 2: one-pass bf16 (1 product), 4: one-pass f16 (1 product)
    bool s3_ready = false;                 // the split-bf16 packings exist (built on first use: ensure_s3)
    bool bf16_ready = false;               // the one-pass bf16 packings exist (built on first use: ensure_bf16)
    bool f16_ready = false;                // the one-pass f16 packings exist (built on first use: ensure_f16)
    double t_pack_s = 0.0, t_upload_s = 0.0, t_tables_s = 0.0;      // dr_cold_times (the capture's seconds: chain)
    int norm_framewise = 0;                // spectrogram normalisation: 0 imagewise, 1 framewise (norm_args[2])
    // conditioner tensors of the last dr_frontend: [L][fe_B][2Cp/4][fe_T][4]
    int fe_B = 0, fe_T = 0;
    drh::DevBuf<float> cond;
    drh::DevBuf<float> cond_dummy;  // one sample of readable memory for generation (no dr_frontend): never used
    // condition='trainable_spec': per-layer conditioner of the learned unconditional spectrogram, [L][2Cp/4][T][4]
    drh::DevBuf<float> cond_tr;
    int cond_tr_T = 0;
    // front-end workspace
    drh::DevBuf<float> wav_pad, power, logmel, specP4, mm;

    drh::DevBuf<long long> dbg_ticks;   // dr_bench_layer measurement hook
    drh::DevBuf<unsigned long long> d_counts;   // dr_frame_counts: result words, ticket, per-block partials (update.hip)
    size_t mm_scratch_off = 0;                // floats into `mm` where the multi-block min-max keeps its partials / tickets
    drh::DevBuf<dr::DynParams> d_dyn;   // per-call scalars of the captured chain (seed, batch offset, guidance weight)
    drh::DevBuf<int> d_tsel;            // per-sample steps of dr_forward_steps

    // fused residual stack (stack_kernel): one persistent launch for the residual layers when every block of the
    // launch is resident at once; fused.active() 0 = one launch per phase (options fused_stack / fused_rearm, yields,
    // time-outs and re-arms: fused_mode.h)
    drh::FusedMode fused;
    int opt_stack_xcd = 1;              // group-per-XCD block mapping (0: weight-panel-per-XCD)
    int opt_stack_fault = 0;            // test hook (option "stack_fault_test")
    int opt_stack_warm = 0;             // idle waves of the fused kernel warm the L2 for the next phase (measured: +-0)
    int opt_zero_taps = 1;              // lab option "zero_taps": fp32 128-frame conv blocks leave out their all-padding edge taps (GemmArgs::zero_taps)
    int n_cus = 0;
    drh::StackSync sync;                // group counters, XCC tags, time-out flags, window ready words
    int opt_tail = 1;                   // fused step: layer 0's shared conv inside the stack launch + the tail kernel
    int64_t tail_launches = 0;
    drh::ChainOptions opt;              // the value options of dr_set_option a chain is run under
    std::vector<int> win_marks;         // option "window_break", ascending: the windows that start a new recording (window 0 always does)
    // The per-window table behind UpdateArgs::win_tab (chain_tables.h: window_table).  A one-block kernel rewrites it on the
    // call's stream in front of every launch sequence / graph launch that reads it, as launch_set_dyn rewrites d_dyn; its
    // address is what a captured chain bakes in, so new marks at the same (sampler, B, T) replay the same graph.
    // Overwriting it is safe while an earlier chain is still running: that chain and the rewriting kernel are on the same
    // stream, so the rewrite starts only when every launch of the earlier chain has finished - and an engine is used
    // from one stream at a time (diffroll_amd.h), as d_dyn, xwork and the activation workspace already require.
    drh::DevBuf<unsigned> d_wintab;
    dr::ChainSteps steps;               // the visited steps S-1 = t_{n-1} > ... > t_0 = 0 in chain order (chain_tables.h); every step unless respaced
    drh::DevBuf<float> d_coef_rs;       // (DR_COEF_FAMILIES, S, 5): d_coef with the row of each visited t whose successor
                                        // is not t - 1 replaced by the respaced row (respaced_table); empty unless respaced
    std::vector<float> h_solver;        // option "solver_order", (2 S, 5): rows [0, S) of the chain's visited steps (solver_table; unvisited rows are
                                        // zero), rows [S, 2 S) the same rows with c = 0 - step t as the FIRST step of a chain
                                        // (option "start_step"); a table of their own, so no row a captured chain reads moves
    drh::DevBuf<float> d_solver;        // ... on the device
    // order 2: the previous step's prediction.  One buffer of two (B, T, 88) halves, allocated on first use and used
    // ping-pong (the tail kernel's row tiles recompute a quad in different blocks: the one that stores must not overwrite
    // what the others still read); hist_par = the half the next step reads.  A captured chain bakes the parity per node.
    drh::DevBuf<float> hist;
    int hist_par = 0;
    dr::HistoryKey hist_key;            // dr_step under order 2: what the history holds (chain_tables.h)
    drh::DevBuf<unsigned> thresh_work;  // option "x0_threshold": its work words and results (kernels.h: ThreshArgs), allocated zeroed on first use
    // options "cfg_rescale" and "cfg_project" / "cfg_norm" / "cfg_momentum": the one work buffer of their statistics launches (kernels.h:
    // GS_HEAD has the layout; a step runs one of them), gs_work_words(B, T, GS_SUMS_MAX) words whichever is set, allocated zeroed on first use
    drh::DevBuf<unsigned> stats_work;
    // option "cfg_momentum": the state m, one float per roll element (B x T x 88), updated in place by update_momentum_kernel.
    // mom_key: what it holds between dr_steps (chain_tables.h: momentum_step); mom_start: the verdict for the dr_step under
    // way - its guided step starts the state (run_step reads it where no chain says)
    drh::DevBuf<float> momentum;
    dr::MomentumKey mom_key;
    bool mom_start = true;
    // option "guidance_stride": the state d, one float per roll element (B x T x 88), written by a refresh step's update and
    // read by the reuse steps behind it.  stride_key: what it holds between dr_steps (chain_tables.h: stride_step);
    // stride_reuse: the verdict for the dr_step under way - its guided step reuses (run_step reads it where no chain says)
    drh::DevBuf<float> stride_d;
    dr::StrideKey stride_key;
    bool stride_reuse = false;
    int64_t inproj_launches = 0;        // standalone input-projection launches (dr_debug_launch_counts): steps no tail kernel primed
    int64_t conv0_launches = 0;         // ... and standalone shared first-layer conv launches in front of a fused stack
    unsigned win_epoch = 0;             // the last epoch handed to a tail launch (eager: one per launch; a chain graph: S per launch)
    drh::DevBuf<float> xalt;            // the tail kernel writes x_{t-1} here (it must not update x_t in place: other
                                        // blocks still read it); the chain ping-pongs between this and its roll buffer
    int last_mode = 0;                  // DR_MODE_* of the most recently planned evaluation (dr_launch_state)
    // The generation of everything a captured launch sequence bakes in that is neither an argument of the call nor a
    // ChainOptions value (both are GraphKey fields of their own): the launch mode (fused.active()), opt_tail, opt_blocked,
    // opt_stack_xcd, opt_stack_warm, opt_zero_taps, opt_stack_fault, stack_dbg_on and prec; the workspace and conditioner allocations and
    // fe_B / fe_T; the committed weights; the respaced coefficient table.  Whatever changes one of them calls stale().
    unsigned baked = 0;
    long kfd_gpu_id = -1;               // the driver's id of this GPU in /sys/class/kfd (tenants.h); -1: unknown, no scans
    double last_tenant_scan_s = -1.0;
    bool unverified = false;            // persistent launches have been issued since the last check of the time-out flag
    hipStream_t fused_stream = nullptr; // ... on this stream (the last one): what a check synchronises before it reads the flag
    int opt_blocked = 2;                // option "blocked_accumulation": 2 (default) = every fp32 flavour that has a blocked form, 1 = 128-frame blocks keep one chain per output (-0.5 % per chain, 2-3x the rounding error)
    drh::DevBuf<float> xsave;           // dr_sample_checked: copy of x_T, so that a timed-out chain can be re-run
    drh::DevBuf<long long> stack_dbg;   // phase tick marks of block 0 (dr_debug_stack_ticks)
    int stack_dbg_on = 0;
    int64_t stack_launches = 0;         // fused-kernel launches issued (captured launches count once, at capture)

    drh::Profile prof;                  // dr_profile_*: timing of the dominant kernel

    // The captured reverse chain of dr_sample (while it is being captured - chain.capturing() - run_step points the update
    // at d_dyn).  Declared after every DevBuf member: members are destroyed in reverse order, so the graph goes before the
    // buffers its nodes point into.
    drh::Chain chain;
};

namespace drh {

inline int fail(dr_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(e, expr)                                                                         \
    do {                                                                                        \
        hipError_t _st = (expr);                                                                \
        if (_st != hipSuccess)                                                                  \
            return drh::fail((e), DR_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_st),   \
                             __FILE__, __LINE__);                                               \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Every entry point runs on the engine's device and leaves the caller's current device as it found it (a process
// that drives several GPUs must not have its device switched by constructing or calling an engine).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// roctx ranges around the host-side phases (rocprofv3 --marker-trace shows them next to the kernel trace).  The
// marker library is looked up at run time: no link-time dependency, silent no-ops when it is absent.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* lib : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            void* h = dlopen(lib, RTLD_LAZY | RTLD_GLOBAL);
            if (!h) continue;
            push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
inline Roctx& roctx() { static Roctx r; return r; }
struct Range {
    explicit Range(const char* name) { if (roctx().push) roctx().push(name); }
    ~Range() { if (roctx().pop) roctx().pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

// The captured chain is stale and a dr_step history has ended.  Says so and nothing more: the chain stays held - it may
// still be running - until dr_sample replaces it (CapturedChain::capture waits for it first).
inline void stale(dr_engine* e) { e->baked += 1; e->hist_key.valid = false; e->mom_key.valid = false; e->stride_key.valid = false; }
// an option that shapes the prediction takes a new value: what dr_step left - the solver history, the momentum state, the
// stored guidance update - ends
inline void end_step_states(dr_engine* e) { e->hist_key.valid = false; e->mom_key.valid = false; e->stride_key.valid = false; }

// ---- abi.hip
int clear_stack_timeout(dr_engine* e);
int set_option(dr_engine* e, const char* name, int value, bool lab);      // lab: the names of dr_debug_set_option too
void set_kfd_root(const char* root);                                      // dr_debug_kfd_root
int build_respaced(dr_engine* e);       // option "sampling_steps": steps and d_coef_rs from opt.steps and h_coef
int build_solver(dr_engine* e);         // option "solver_order": h_solver / d_solver from the chain's steps and h_coef
int debug_threshold(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st);      // dr_debug_threshold
int debug_rescale(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st);        // dr_debug_rescale
int debug_project(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st);        // dr_debug_project
int debug_momentum(dr_engine* e, const float* d_x0c, const float* d_x0u, const float* d_m_prev, float* d_m_next, int B, int T, float w,
                   float* d_out, hipStream_t st);                                                                                    // dr_debug_momentum

// ---- pack.hip
const std::vector<float>* find_param(dr_engine* e, const std::string& name);
size_t expected_numel(const dr_engine* e, const std::string& name);
int ensure_s3(dr_engine* e);            // the split-bf16 packings, built on first use
int ensure_bf16(dr_engine* e);          // the one-pass bf16 packings, built on first use (independent of ensure_s3)
int ensure_f16(dr_engine* e);           // the one-pass f16 packings, built on first use (independent of the other two)
bool packings_ready(const dr_engine* e, int prec);      // the packings precision `prec` contracts exist
int ensure_packings(dr_engine* e, int prec);      // what precision `prec` needs beyond the fp32 packings (nothing for 0)
int commit(dr_engine* e, hipStream_t st);

// ---- plan.hip
hipError_t launch_tiled(const GemmArgs& a, int epi, Tile t, hipStream_t s, int prec);
void allow_splitk(const dr_engine* e, GemmArgs& a);
constexpr int MAX_DEVICES = 64;
extern const float* g_zero_vecs[MAX_DEVICES];
const float* zero_vec();
GemmArgs p4_gemm(const float* Wp, const float* bias, int MT, const float* X, int planes, int NB, int T);
void p4_out(GemmArgs& a, float* Y, int planes, int T, int rows);
int build_trainable_cond(dr_engine* e, int T);
int ensure_workspace(dr_engine* e, int NB, int T);
// What run_step offers run_network so that a whole reverse step becomes TWO launches (the residual stack incl. layer 0's
// shared contraction + the tail kernel: skip / output projection, update, next input projection) where the fused
// kernel applies; run_network reports back what it took.
struct TailPlan {
    UpdateArgs u{};            // this step's update (x = x_t, read only by the tail kernel)
    float* x_out = nullptr;    // where the tail kernel writes x_{t-1}
    int u_B = 0;               // rolls
    int next_t = -1;           // >= 0: the chain continues with step next_t (its input projection joins the tail)
    StepEval next{};           // ... whose evaluation has this shape (launch_plan.h: a guidance interval may begin or end here)
    int next_prec = 0;         // ... and this precision (option "exact_below": launch_plan.h, step_precision)
    bool skip_inproj = false;  // h / hd (and, guided, layer 0's g) were written by the previous step's tail ...
    StepEval primed{};         // ... for an evaluation of this shape: honoured only when it is THIS step's shape
    bool done = false;         // out: the tail kernel ran (update included, result in x_out)
    bool inproj_done = false;  // out: ... and it wrote the next step's h / hd (and layer 0's g for a guided pair)
};
// prec: the precision of this evaluation - the engine's mode (dr_forward), or the step's (run_step: option "exact_below")
int run_network(dr_engine* e, const float* xin, int bmod, int NB, int n_cond, int T, int t, int prec, float* x0_out,
                hipStream_t st, bool zero_spec = false, const int* tsel = nullptr, TailPlan* tail = nullptr);
int sampler_shape(int sampler, int B, int& NB, int& n_cond, int& family, bool& zero_spec);
int sampler_shape(int sampler, int B, int& NB, int& n_cond);
// the layout half of an update's arguments for B rolls of T frames: n, per_sample, dyn, win, draw_n / draw_G, win_tab
UpdateArgs update_base(const dr_engine* e, int B, int T);
// option "x0_threshold": the arguments of a step's threshold launches, from the update they precede
ThreshArgs thresh_args(const dr_engine* e, const UpdateArgs& u);
// option "cfg_rescale": the arguments of a step's statistics launch, likewise
RescaleArgs rescale_args(const dr_engine* e, const UpdateArgs& u);
// options "cfg_project" / "cfg_norm": likewise
ProjectArgs project_args(const dr_engine* e, const UpdateArgs& u);
// option "cfg_momentum": bf, the factor the kernels multiply m_prev by
inline float momentum_bf(const dr_engine* e) { return (float)((double)e->opt.cfg_momentum / 10000.0); }
// option "guidance_stride": the stride a step reads - n, or 0 for off (the values 0 and 1)
inline int guidance_stride(const dr_engine* e) { return e->opt.guid_stride > 1 ? e->opt.guid_stride : 0; }
struct ChainState {
    bool inproj_ready = false;
    StepEval ready{};          // the shape inproj_ready holds for (TailPlan::primed of the next step)
    int next_t = -1;
    float* x_out = nullptr;    // where a fused step writes x_{t-1} (null: e->xalt)
    bool guided = false;       // option "cfg_momentum": a guided step has run in this chain (the next one continues the state)
    int guided_k = 0;          // option "guidance_stride": the guided steps this chain has run - the ordinal of the next one
};
int run_step(dr_engine* e, int sampler, float* x, const float* noise, int B, int T, int t, float w, uint64_t seed,
             int first_sample, hipStream_t st, float** result = nullptr, ChainState* chain = nullptr);

}  // namespace drh
