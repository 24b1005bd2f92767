// Host side, part 3: the C-ABI of include/diffroll_amd.h (the boundary) - engine life cycle, front-end, forward / step / sample
// (the reverse chain as one hipGraph), time-out handling of the persistent kernels, the consumers of a finished roll, options.
#include "engine_state.h"
#include "tenants.h"

#include <algorithm>
#include <condition_variable>
#include <mutex>

namespace drh {

thread_local std::string g_create_error;
void release_stager(int dev);       // pack.hip
std::atomic<int> g_engines[MAX_DEVICES];      // live engines per device: the last one out releases the upload stager

// The persistent kernels assume that all their workgroups are resident at once - true while ONE engine computes on the
// device.  Engines of one process take turns on a per-device "fused slot".  An engine that wants to issue fused launches
// while another engine of the process is issuing its own (another host thread, inside an API call) waits for that call to
// return - microseconds to milliseconds of launch overhead, no GPU wait; if that engine's last fused work is still running
// on the device, the newcomer's stream is made to wait for it ON THE DEVICE (hipStreamWaitEvent on the event recorded
// behind that work): the two engines' persistent launches then never overlap, nobody synchronises the host and nobody gives
// up fusing.  (Until round 5 the newcomer yielded to per-phase launches for the rest of its life instead; its per-phase
// blocks cannot co-reside with a persistent launch that owns every CU's LDS either, so nothing was gained by not waiting.)
// (Other PROCESSES on the device are looked for in tenants.h; the ~1 s spin bound of the barriers stays as the backstop.)
struct FusedSlot {
    std::mutex mu;
    std::condition_variable cv;
    dr_engine* owner = nullptr;
    bool claimed = false;          // the owner is issuing launches right now (its event is not recorded yet)
    hipEvent_t done = nullptr;     // recorded behind the owner's last fused work
};
FusedSlot g_slots[MAX_DEVICES];

// true: the slot is ours (after `st` has been ordered behind the previous owner's fused work, if any is in flight)
bool claim_fused_slot(dr_engine* e, hipStream_t st) {
    FusedSlot& s = g_slots[e->cfg.device];
    std::unique_lock<std::mutex> lk(s.mu);
    s.cv.wait(lk, [&] { return !s.claimed || s.owner == e; });
    if (s.owner && s.owner != e && s.done && hipEventQuery(s.done) == hipErrorNotReady) {
        if (hipStreamWaitEvent(st, s.done, 0) != hipSuccess) return false;
    }
    s.owner = e;
    s.claimed = true;
    return true;
}
void release_fused_slot(dr_engine* e, hipStream_t st) {
    FusedSlot& s = g_slots[e->cfg.device];
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.owner != e) return;
        if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) s.done = nullptr;
        if (s.done) (void)hipEventRecord(s.done, st);
        s.claimed = false;
    }
    s.cv.notify_all();
}
void forget_fused_slot(dr_engine* e) {
    FusedSlot& s = g_slots[e->cfg.device];
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.owner == e) { s.owner = nullptr; s.claimed = false; }
    }
    s.cv.notify_all();
}
// "The captured chain is stale" has one spelling, stale(e) (engine_state.h): it moves the generation in the chain's key and
// destroys nothing.  Only dr_sample, about to capture the replacement, destroys a chain, and the owner waits for it first.
// Another process on this GPU (tenants.h)?  Asked at creation and in front of a chain, at most every 250 ms (a scan is
// ~0.1 ms of sysfs reads: 0.4 % of a single-clip chain if it ran every time; force: now - behind a graph capture).
// Returns 1 = yes, 0 = no, -1 = not looked (rate limit / no sysfs / undecided).  A first look that finds a second queue
// holder AND busy CUs may be seeing THIS process's own kernels - the engine's front-end, another stream of the caller, the
// previous sample's RCCL all-gather on the communicator's stream (a rank of a multi-GPU job never waits for that before it
// starts its next sample): only then - an exclusive GPU never pays for it - everything this process has in flight on
// the device is waited for (hipDeviceSynchronize: microseconds of front-end work in practice) and the look repeated, so
// that what is still busy afterwards is somebody else's.
std::mutex g_kfd_mu;
std::string g_kfd_root = "/sys/class/kfd/kfd";
std::string kfd_root() { std::lock_guard<std::mutex> lk(g_kfd_mu); return g_kfd_root; }
void set_kfd_root(const char* root) { std::lock_guard<std::mutex> lk(g_kfd_mu); g_kfd_root = root ? root : "/sys/class/kfd/kfd"; }
int shared_with_another_process(dr_engine* e, bool force = false, bool may_sync = true) {
    if (e->kfd_gpu_id < 0) return -1;
    const double now = now_s();
    if (!force && now - e->last_tenant_scan_s < 0.250) return -1;
    e->last_tenant_scan_s = now;
    const std::string root = kfd_root();
    TenantScan t = scan_tenants(root, e->kfd_gpu_id);
    if (!t.readable) return -1;
    if (!(t.holders >= 2 && t.busy_cus > 0)) return 0;
    if (!may_sync) {                    // (undecided: what is busy may be this process's own other engines)
        e->last_tenant_scan_s = 0;      // the look in front of the engine's first chain decides, whatever the rate limit says
        return -1;
    }
    (void)hipDeviceSynchronize();
    t = scan_tenants(root, e->kfd_gpu_id);
    return (t.holders >= 2 && t.busy_cus > 0) ? 1 : 0;
}
// What a look found goes into the engine's FusedMode: another process computing yields (per-phase launches from the next
// launch on); while yielded, two looks in a row that find the GPU exclusive again switch the fused launches back on.
void fused_look(dr_engine* e, int shared) {
    const bool yielded = e->fused.state == FusedMode::YIELDED;
    if (!e->fused.look(shared)) return;
    stale(e);
    if (!yielded && e->fused.yields <= 3)       // per engine (a measurement reads the counter: dr_launch_state); not a log flood
        fprintf(stderr, "[diffroll_amd] engine %p: another process is computing on device %d - one launch per phase from now on (same "
                        "results, no co-residency assumption; yield #%lld of this engine; fused launches come back after two clean looks)\n",
                (void*)e, e->cfg.device, (long long)e->fused.yields);
    if (yielded && e->fused.rearms <= 3)
        fprintf(stderr, "[diffroll_amd] engine %p: device %d is this process's own again - fused launches back on\n", (void*)e, e->cfg.device);
}

// the engine's turn on the slot for the duration of one API call that may issue fused launches
struct FusedTurn {
    dr_engine* e;
    hipStream_t st;
    bool held = false;
    int rc = DR_OK;
    FusedTurn(dr_engine* e_, hipStream_t st_) : e(e_), st(st_) {
        if (!e->fused.active()) return;
        if (claim_fused_slot(e, st)) held = true;
        else rc = fail(e, DR_EHIP, "hipStreamWaitEvent behind another engine's fused work failed");
    }
    ~FusedTurn() { if (held) release_fused_slot(e, st); }
    FusedTurn(const FusedTurn&) = delete;
    FusedTurn& operator=(const FusedTurn&) = delete;
};

// After a barrier time-out (device idle): re-arm the group counters, forget the published XCC tags, lower both flags.
int clear_stack_timeout(dr_engine* e) {
    HIPCHK(e, e->sync.clear());
    e->win_epoch = 0;
    return DR_OK;
}

int check_ready(dr_engine* e, int sampler, int B, int T) {
    if (!e->committed) return fail(e, DR_ESTATE, "dr_commit has not been called");
    if (e->sync.err_host && *e->sync.err_host)
        return fail(e, DR_ETIMEOUT, "a group barrier of an earlier fused residual-stack launch timed out (the results since the "
                                    "last dr_finish are invalid): is another stream / engine computing on this device at the "
                                    "same time? call dr_finish (or dr_stack_status) to clear the condition and recompute - "
                                    "dr_finish also switches this engine to per-phase launches; dr_sample_checked does all of that");
    if (B <= 0 || T <= 0) return fail(e, DR_EINVAL, "bad shape B=%d T=%d", B, T);
    if (!packings_ready(e, e->prec)) {       // (a commit after dr_set_precision, or a packing build that failed: never launch without them)
        int rc = ensure_packings(e, e->prec);
        if (rc) return rc;
    }
    // option "draws": the B rolls are D draws of B / D clips, and the front-end ran on the clips
    const int D = e->opt.draws;
    if (B % D) return fail(e, DR_EINVAL, "B=%d rolls are not a whole number of draws (option draws = %d)", B, D);
    if (sampler != DR_SAMPLER_GENERATION_DDPM_X0 && (e->fe_B != B / D || e->fe_T != T)) {
        if (D > 1)
            return fail(e, DR_ESTATE, "dr_frontend(B=%d,T=%d) must precede a conditional evaluation of %d draws of B/draws=%d clips (B=%d,T=%d)",
                        e->fe_B, e->fe_T, D, B / D, B, T);
        return fail(e, DR_ESTATE, "dr_frontend(B=%d,T=%d) must precede a conditional evaluation with B=%d,T=%d",
                    e->fe_B, e->fe_T, B, T);
    }
    return DR_OK;
}

// The options, against what only a call knows - sampler, batch and frames; NB (out) is the sampler's evaluation batch.
// option "window_overlap": at most two windows share a frame (O <= T / 2)
// option "window_break": every mark names a window of this batch (marks are ignored while "window_overlap" is 0)
// options "solver_order", "x0_clip" and "x0_threshold" act on an x0 prediction (DR_SAMPLER_* 0-5): the epsilon samplers
// refuse them; "x0_threshold" refines "x0_clip", which names the range, and is refused without it
// options "guidance_t_min" / "guidance_t_max": the samplers that guide need lo <= hi (the others ignore both)
// options "cfg_project" / "cfg_norm": refused beside "x0_threshold" (whose selection would have to rank the projected
// prediction) and beside "cfg_rescale" (an alternative; a combined form would need the spread of the projected prediction)
// option "cfg_momentum": refused while "cfg_project" and "cfg_norm" are both 0 (beside either, the two refusals above cover it)
// option "guidance_stride": refused beside "x0_threshold", "cfg_rescale", "cfg_project", "cfg_norm" and "cfg_momentum" (a step
// that reuses has no unconditional prediction for their statistics) and by a sampler that does not guide
int check_options(dr_engine* e, int sampler, int B, int& NB, int T) {
    const ChainOptions& o = e->opt;
    if (2 * o.win_O > T)
        return fail(e, DR_EINVAL, "window_overlap %d exceeds half the window (T = %d frames)", o.win_O, T);
    if (o.win_O > 0 && T >= (1 << WIN_BLEND_SHIFT))
        return fail(e, DR_EINVAL, "window_overlap: windows hold fewer than %d frames, got T = %d", 1 << WIN_BLEND_SHIFT, T);
    const int D = o.draws, n = B / D;      // (option "draws": the marks are those of one draw and repeat per draw)
    if (o.win_O > 0 && !e->win_marks.empty()) {
        if (e->win_marks.back() >= n) {
            if (D > 1)
                return fail(e, DR_EINVAL, "window_break %d is not a window of one draw (B = %d windows in %d draws of %d)", e->win_marks.back(), B, D, n);
            return fail(e, DR_EINVAL, "window_break %d is not a window of this batch (B = %d windows)", e->win_marks.back(), B);
        }
        if (B > STACK_GROUPS)
            return fail(e, DR_EINVAL, "window_break: a batch with recording boundaries holds at most %d windows, got B = %d", STACK_GROUPS, B);
    }
    if (o.win_O > 0 && D > 1) {
        if (B > STACK_GROUPS)
            return fail(e, DR_EINVAL, "draws: a window batch of several draws holds at most %d windows, got B = %d", STACK_GROUPS, B);
        const long R = (long)e->win_marks.size() + 1, G = o.draw_G > 0 ? o.draw_G : R;
        if ((D - 1) * G + R > 65536)
            return fail(e, DR_EINVAL, "draws: %d draws at key stride %ld do not fit the window table (sample key offsets < 65536)", D, G);
    }
    int n_cond;
    if (sampler_shape(sampler, B, NB, n_cond)) return fail(e, DR_EINVAL, "unknown sampler %d", sampler);
    const bool eps = !predicts_x0(sampler);
    if (o.solver != 0 && eps)
        return fail(e, DR_EINVAL, "sampler %d predicts epsilon: solver_order = %d integrates an x0 prediction (samplers 0-5); set "
                                  "solver_order 0 for the sampler's own update", sampler, o.solver);
    if (o.x0_thresh != 0 && o.x0_clamp == 0)
        return fail(e, DR_EINVAL, "x0_threshold = %d needs x0_clip: the range the rolls were normalised to (x0_clip 1 = [0, 1], 2 = "
                                  "[-1, 1]) is what the threshold is compared with, and x0_clip is 0", o.x0_thresh);
    if (o.x0_thresh != 0 && eps)
        return fail(e, DR_EINVAL, "sampler %d predicts epsilon: x0_clip = %d and x0_threshold = %d act on an x0 prediction (samplers "
                                  "0-5); set both 0 for this sampler", sampler, o.x0_clamp, o.x0_thresh);
    if (o.x0_clamp != 0 && eps)
        return fail(e, DR_EINVAL, "sampler %d predicts epsilon: x0_clip = %d clamps an x0 prediction (samplers 0-5); set "
                                  "x0_clip 0 for this sampler", sampler, o.x0_clamp);
    if ((o.cfg_project != 0 || o.cfg_norm != 0) && o.x0_thresh != 0)
        return fail(e, DR_EINVAL, "cfg_project = %d / cfg_norm = %d do not combine with x0_threshold = %d: the selection would have "
                                  "to rank the projected prediction; set x0_threshold 0 (x0_clip alone combines)", o.cfg_project, o.cfg_norm, o.x0_thresh);
    if ((o.cfg_project != 0 || o.cfg_norm != 0) && o.cfg_rescale != 0)
        return fail(e, DR_EINVAL, "cfg_project = %d / cfg_norm = %d do not combine with cfg_rescale = %d: the two are alternatives; "
                                  "set one of them 0", o.cfg_project, o.cfg_norm, o.cfg_rescale);
    if (o.cfg_momentum != 0 && o.cfg_project == 0 && o.cfg_norm == 0)
        return fail(e, DR_EINVAL, "cfg_momentum = %d acts on the update that cfg_project / cfg_norm shape, and cfg_project = %d and "
                                  "cfg_norm = %d are both off; set one of them, or cfg_momentum 0", o.cfg_momentum, o.cfg_project, o.cfg_norm);
    if (o.guid_stride > 1) {
        // (the statistics of each of them need the unconditional prediction, which a step that reuses does not have)
        const struct { const char* name; int value; } partners[] = {{"x0_threshold", o.x0_thresh}, {"cfg_rescale", o.cfg_rescale},
            {"cfg_project", o.cfg_project}, {"cfg_norm", o.cfg_norm}, {"cfg_momentum", o.cfg_momentum}};
        for (const auto& p : partners)
            if (p.value != 0)
                return fail(e, DR_EINVAL, "guidance_stride = %d does not combine with %s = %d: its statistics need the unconditional "
                                          "prediction, which a step that reuses the guidance update does not evaluate; set one of "
                                          "them 0", o.guid_stride, p.name, p.value);
        if (NB != 2 * B)
            return fail(e, DR_EINVAL, "sampler %d does not guide: guidance_stride = %d reuses the guidance update of a sampler that "
                                      "guides (samplers 1, 3, 5); set guidance_stride 0 for this sampler", sampler, o.guid_stride);
    }
    if (NB == 2 * B && o.guid.empty(e->S))
        return fail(e, DR_EINVAL, "guidance interval is empty: guidance_t_min = %d exceeds guidance_t_max = %d", o.guid.lo,
                    o.guid.hi_eff(e->S));
    return DR_OK;
}

// The per-window table of this batch (engine_state.h: d_wintab) from the marks, written on `st` in front of the launches
// that read it: an eager sequence with marks, and every launch of a captured chain (force: its graph holds the table's
// address whether or not marks were set when it was captured).  Without marks: window b of recording 0.
int write_windows(dr_engine* e, int B, bool force, hipStream_t st) {
    if (e->opt.win_O <= 0 || B > STACK_GROUPS || (!force && e->win_marks.empty() && e->opt.draws <= 1)) return DR_OK;
    HIPCHK(e, launch_set_windows(e->d_wintab, window_table(e->win_marks, B, e->opt.draws, e->opt.draw_G), B, st));
    return DR_OK;
}

// option "sampling_steps": the chain's steps and, for a respaced chain, its coefficient table on the device (chain_tables.h:
// ChainSteps, respaced_table).  Rebuilt by dr_commit and by the option.
int build_respaced(dr_engine* e) {
    e->steps = ChainSteps(e->S, 0);
    e->d_coef_rs.reset();
    const ChainSteps steps(e->S, e->opt.steps);
    if (!steps.respaced()) return DR_OK;      // the full chain: committed rows
    const std::vector<float> tab = respaced_table(e->h_coef, steps);
    HIPCHK(e, e->d_coef_rs.ensure(tab.size(), false));
    HIPCHK(e, hipMemcpy(e->d_coef_rs, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    e->steps = steps;
    return DR_OK;
}

// option "solver_order": the solver's rows for the steps the chain visits (chain_tables.h: solver_table), on the host and -
// while an order is set - on the device.  Rebuilt by dr_commit and whenever "sampling_steps", "solver_order" or
// "solver_noise" changes; the caller has made sure no chain is reading it.
int build_solver(dr_engine* e) {
    e->h_solver = solver_table(e->h_coef, e->steps, e->opt.solver, e->opt.solver_noise);
    if (e->opt.solver == 0) return DR_OK;
    HIPCHK(e, e->d_solver.ensure(e->h_solver.size(), false));
    HIPCHK(e, hipMemcpy(e->d_solver, e->h_solver.data(), e->h_solver.size() * sizeof(float), hipMemcpyHostToDevice));
    return DR_OK;
}

// option "start_step": the chain position of the step a chain begins at (chain_tables.h: start_position); a step the chain
// does not visit is refused, naming the visited steps on either side of it
int start_position(dr_engine* e, int& i0) {
    const StartPosition p = dr::start_position(e->steps, e->opt.start);
    i0 = std::max(p.pos, 0);
    if (p.pos >= 0) return DR_OK;
    return fail(e, DR_EINVAL, "start_step %d is not a step this chain visits (option sampling_steps = %d): the visited steps "
                              "on either side of it are %d and %d", e->opt.start, e->opt.steps, p.above, p.below);
}
// option "start_noise": the chain's first node - the clean roll in x becomes x at step ts (update.hip: diffuse_kernel).
// z is row 0 of the injected noise (no reverse step reads it: step 0 draws none), else Philox with counter word S + ts,
// keyed as run_step keys the updates of this chain (plan.hip).
int run_diffuse(dr_engine* e, float* x, const float* d_noise, int B, int T, int ts, uint64_t seed, int first_sample, hipStream_t st) {
    UpdateArgs u = update_base(e, B, T);
    u.x = x; u.noise = d_noise;
    u.coef = e->d_coef + (size_t)ts * 5;      // family 0: [.., .., sqrt_acp[ts], sqrt_1m_acp[ts], ..], the committed row
    u.t = e->S + ts;
    u.seed = seed; u.first_sample = first_sample;
    HIPCHK(e, launch_diffuse(u, st));
    return DR_OK;
}

// A buffer the chain's launches point into (the history of solver order 2, the threshold launches' work words) grows to n
// zeroed elements before anything is launched or captured: what may still read the old one is waited for
template <class V>
int grow_chain_buffer(dr_engine* e, DevBuf<V>& buf, size_t n, hipStream_t st) {
    if (buf.fits(n)) return DR_OK;
    HIPCHK(e, hipStreamSynchronize(st));
    HIPCHK(e, e->chain.wait());
    HIPCHK(e, buf.ensure(n, true));
    return DR_OK;
}

// The engine's one work buffer of the statistics launches ("cfg_rescale", "cfg_project" / "cfg_norm" / "cfg_momentum"): sized for the
// widest of them whichever is set, so a switch between the options at one shape neither grows it nor costs a captured chain its key
int grow_stats_work(dr_engine* e, int B, int T, hipStream_t st) {
    return grow_chain_buffer(e, e->stats_work, gs_work_words(B, T, GS_SUMS_MAX), st);
}

// The opening the four dr_debug_* probes of the stages share: the engine is committed, the probed option - a or b - is on (else
// refused with `off`), the options are ones a step of B rolls of T frames can run under, the window table is written, and the
// update a step would hand its stage stands on the caller's tensors (clamp: with the range "x0_clip" names).  Then `body`, the
// probe's own buffer growth, launch and gather, on the engine's device.
struct ProbeOf { int ChainOptions::*a, ChainOptions::*b; const char* off; bool clamp; };
template <class Body>
int probe(dr_engine* e, const ProbeOf& of, const float* d_x0c, const float* d_x0u, int B, int T, float w, const float* d_out,
          hipStream_t st, Body&& body) {
    if (!e || !d_x0c || !d_out) return fail(e, DR_EINVAL, "null argument");
    if (B <= 0 || T <= 0) return fail(e, DR_EINVAL, "bad shape B=%d T=%d", B, T);
    if (!e->committed) return fail(e, DR_ESTATE, "dr_commit has not been called");
    DeviceGuard guard(e->cfg.device);
    if (e->opt.*of.a == 0 && e->opt.*of.b == 0) return fail(e, DR_EINVAL, "%s", of.off);
    if (B % e->opt.draws) return fail(e, DR_EINVAL, "draws = %d does not divide B = %d", e->opt.draws, B);
    int rc, NB;
    if ((rc = check_options(e, DR_SAMPLER_DDPM_X0, B, NB, T))) return rc;
    if ((rc = write_windows(e, B, false, st))) return rc;
    UpdateArgs u = update_base(e, B, T);      // (never captured: no d_dyn, the table only where marks or draws need it)
    u.x0c = d_x0c; u.x0u = d_x0u;
    u.w = w; u.onepw = (float)(1.0 + (double)w);
    if (of.clamp) { u.clamp_lo = e->opt.x0_clamp == 2 ? -1.f : 0.f; u.clamp_hi = 1.f; }
    return body(u);
}

// dr_debug_threshold: the threshold launches of a step on the caller's tensors, then the groups' {q, s} gathered into d_out
int debug_threshold(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st) {
    const ProbeOf of{&ChainOptions::x0_thresh, &ChainOptions::x0_thresh, "dr_debug_threshold: x0_threshold is 0 (off)", true};
    return probe(e, of, d_x0c, d_x0u, B, T, w, d_out, st, [&](const UpdateArgs& u) -> int {
        if (int rc = grow_chain_buffer(e, e->thresh_work, thresh_work_words(B), st)) return rc;
        const ThreshArgs ta = thresh_args(e, u);
        HIPCHK(e, launch_threshold(ta, B, st));
        HIPCHK(e, launch_thresh_gather(ta, B, d_out, st));
        return DR_OK;
    });
}

// dr_debug_rescale: the statistics launch of a step on the caller's tensors, then the groups' g gathered into d_out
int debug_rescale(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st) {
    const ProbeOf of{&ChainOptions::cfg_rescale, &ChainOptions::cfg_rescale, "dr_debug_rescale: cfg_rescale is 0 (off)", false};
    return probe(e, of, d_x0c, d_x0u, B, T, w, d_out, st, [&](const UpdateArgs& u) -> int {
        if (int rc = grow_stats_work(e, B, T, st)) return rc;
        const RescaleArgs ra = rescale_args(e, u);
        HIPCHK(e, launch_rescale(ra, B, st));
        HIPCHK(e, launch_group_gather(ra.u, ra.work, 1, B, d_out, st));
        return DR_OK;
    });
}

// dr_debug_project: the statistics launch of a step on the caller's tensors, then the groups' (a, b) gathered into d_out
int debug_project(dr_engine* e, const float* d_x0c, const float* d_x0u, int B, int T, float w, float* d_out, hipStream_t st) {
    const ProbeOf of{&ChainOptions::cfg_project, &ChainOptions::cfg_norm, "dr_debug_project: cfg_project and cfg_norm are both 0 (off)", false};
    return probe(e, of, d_x0c, d_x0u, B, T, w, d_out, st, [&](const UpdateArgs& u) -> int {
        if (int rc = grow_stats_work(e, B, T, st)) return rc;
        const ProjectArgs pa = project_args(e, u);
        HIPCHK(e, launch_project(pa, B, st));
        HIPCHK(e, launch_group_gather(pa.u, pa.work, 2, B, d_out, st));
        return DR_OK;
    });
}

// dr_debug_momentum: the statistics launch of a step under "cfg_momentum" on the caller's tensors and state, the groups' (a, b)
// gathered into d_out, and - where wanted - the state the step would leave
int debug_momentum(dr_engine* e, const float* d_x0c, const float* d_x0u, const float* d_m_prev, float* d_m_next, int B, int T, float w,
                   float* d_out, hipStream_t st) {
    const ProbeOf of{&ChainOptions::cfg_momentum, &ChainOptions::cfg_momentum, "dr_debug_momentum: cfg_momentum is 0 (off)", false};
    return probe(e, of, d_x0c, d_x0u, B, T, w, d_out, st, [&](const UpdateArgs& u) -> int {
        if (int rc = grow_stats_work(e, B, T, st)) return rc;
        const MomentumArgs ma{project_args(e, u), d_m_prev, momentum_bf(e)};
        HIPCHK(e, launch_momentum(ma, B, st));
        HIPCHK(e, launch_group_gather(ma.p.u, ma.p.work, 2, B, d_out, st));
        if (d_m_next) HIPCHK(e, launch_momentum_state(u, d_m_prev, ma.bf, d_m_next, st));
        return DR_OK;
    });
}

// A setting that captured launches bake in (engine_state.h: dr_engine::baked) takes a new value: a change makes the chain stale
template <class Field>
bool put(dr_engine* e, Field& field, int value) {
    if (field == value) return false;
    field = value;
    stale(e);
    return true;
}

// The options that are a value of ChainOptions and nothing else: refused outside [lo, hi] (or_zero: 0 is accepted beside it)
// with the option's own text, which takes the value; stored.  None drops a captured chain - each is part of the chain's key
// (GraphKey), so a chain captured under another value is simply not replayed and one captured under this value still is.
// ends_step_states: the option shapes the prediction - under "solver_order" 2 the history holds the prediction as the previous
// step blended / clamped / thresholded / rescaled / projected it, and the momentum state holds sums under the previous value - so
// a dr_step sequence does not continue across a change: the next step that is not a chain's first is refused, as for "solver_noise".
// What a value needs of a call - "draws" B % D and the front-end's batch, "x0_threshold" its "x0_clip", ... - check_options asks.
struct ValueOption {
    const char* name;
    int ChainOptions::*field;
    int lo, hi;
    bool or_zero, ends_step_states;
    const char* refusal;
};
constexpr int NO_BOUND = 0x7fffffff;
const ValueOption VALUE_OPTIONS[] = {
    {"window_blend", &ChainOptions::win_blend, 0, 2, false, true,
     "window_blend is 0 (the mean of the two windows' predictions), 1 (linear cross-fade) or 2 (hand-over at the middle of the overlap), got %d"},
    {"draws", &ChainOptions::draws, 1, NO_BOUND, false, true, "draws is >= 1 (1 = every roll its own clip), got %d"},
    {"draw_stride", &ChainOptions::draw_G, 0, NO_BOUND, false, false, "draw_stride is >= 0 (0 = the clips of the batch), got %d"},
    {"start_noise", &ChainOptions::start_noise, 0, 1, false, false,
     "start_noise is 0 (x on entry is x at the start step) or 1 (a clean roll, diffused to it), got %d"},
    {"x0_clip", &ChainOptions::x0_clamp, 0, 2, false, true, "x0_clip is 0 (off), 1 (clamp the x0 prediction to [0, 1]) or 2 (to [-1, 1]), got %d"},
    {"x0_threshold", &ChainOptions::x0_thresh, 5000, 10000, true, true,
     "x0_threshold is 0 (off) or the percentile in units of 1 / 10000, 5000 .. 10000 (9950 = 99.5 %%), got %d"},
    {"cfg_rescale", &ChainOptions::cfg_rescale, 0, 10000, false, true,
     "cfg_rescale is 0 (off) or phi in units of 1 / 10000, 1 .. 10000 (7000 = 0.7), got %d"},
    {"cfg_project", &ChainOptions::cfg_project, 0, 10000, false, true,
     "cfg_project is 0 (off) or rho in units of 1 / 10000, 1 .. 10000 (10000 = the whole parallel component), got %d"},
    {"cfg_norm", &ChainOptions::cfg_norm, 0, 100000, false, true,
     "cfg_norm is 0 (off) or the rms bound r in units of 1 / 10000, 1 .. 100000 (500 = 0.05), got %d"},
    {"cfg_momentum", &ChainOptions::cfg_momentum, -9999, 9999, false, true,
     "cfg_momentum is 0 (off) or beta in units of 1 / 10000, -9999 .. 9999 (-5000 = -0.5), got %d"},
    {"guidance_stride", &ChainOptions::guid_stride, 0, 64, false, true,
     "guidance_stride is 0 or 1 (off) or the stride n, 2 .. 64 (2 = every second guided step runs both evaluations), got %d"},
};

// dr_set_option (lab = false: the product's options) / dr_debug_set_option (lab = true: the A/B and test knobs too)
int set_option(dr_engine* e, const char* name, int value, bool lab) {
    if (!e || !name) return fail(e, DR_EINVAL, "null argument");
    const std::string n = name;
    DeviceGuard guard(e->cfg.device);
    if (n == "fused_stack") { if (e->fused.set_option(value)) stale(e); return DR_OK; }      // (forgets a pending yield or heal)
    if (n == "fused_rearm") { e->fused.rearm_after = value; return DR_OK; }
    if (n == "blocked_accumulation") {
        if (value != 1 && value != 2) return fail(e, DR_EINVAL, "blocked_accumulation is 1 or 2");
        put(e, e->opt_blocked, value);
        return DR_OK;
    }
    if (n == "fused_tail") { put(e, e->opt_tail, value); return DR_OK; }
    if (n == "window_overlap") {      // (O <= T / 2 is checked by dr_step / dr_sample, which know T)
        if (value < 0) return fail(e, DR_EINVAL, "window_overlap is >= 0 (0 = off)");
        put(e, e->opt.win_O, value);
        return DR_OK;
    }
    for (const ValueOption& o : VALUE_OPTIONS) {
        if (n != o.name) continue;
        if ((value < o.lo || value > o.hi) && !(o.or_zero && value == 0)) return fail(e, DR_EINVAL, o.refusal, value);
        if (o.ends_step_states && e->opt.*o.field != value) end_step_states(e);
        e->opt.*o.field = value;
        return DR_OK;
    }
    // (a mark >= B is refused by dr_step / dr_sample, which know B; no captured chain is dropped: the table is data)
    if (n == "window_break") {
        if (value < 0) return fail(e, DR_EINVAL, "window_break is >= 0 (0 = clear all marks), got %d", value);
        if (value == 0) { e->win_marks.clear(); return DR_OK; }
        auto at = std::lower_bound(e->win_marks.begin(), e->win_marks.end(), value);
        if (at == e->win_marks.end() || *at != value) e->win_marks.insert(at, value);
        return DR_OK;
    }
    if (n == "sampling_steps") {
        if (value != 0 && (value < 2 || value > e->S))
            return fail(e, DR_EINVAL, "sampling_steps is 0 (off) or in [2, timesteps = %d], got %d", e->S, value);
        if (!put(e, e->opt.steps, value)) return DR_OK;
        (void)hipDeviceSynchronize();         // a chain of the previous value may still be reading the two tables rebuilt below
        if (!e->committed) return DR_OK;      // (dr_commit builds it)
        if (int rc = build_respaced(e)) { e->opt.steps = 0; return rc; }
        return build_solver(e);               // (its rows belong to the steps this chain visits)
    }
    if (n == "solver_order") {
        // (no captured chain is dropped: the value is part of the chain's key - GraphKey - as "draws" is.  A chain captured
        // under this value reads the table at replay, and the table is this value's whenever that chain is replayed.)
        if (value < 0 || value > 2)
            return fail(e, DR_EINVAL, "solver_order is 0 (the sampler's own update), 1 or 2 (DPM-Solver++ 2M), got %d", value);
        if (e->opt.solver == value) return DR_OK;
        (void)hipDeviceSynchronize();         // a chain of the previous order may still be reading the table
        e->opt.solver = value;
        end_step_states(e);
        if (!e->committed) return DR_OK;      // (dr_commit builds it)
        return build_solver(e);
    }
    if (n == "solver_noise") {
        // (as "solver_order": part of the chain's key, nothing is dropped; the table is rebuilt while an order is set - a
        // chain captured under the other value is not replayed until the value, and with it the table, is back)
        if (value != 0 && value != 1)
            return fail(e, DR_EINVAL, "solver_noise is 0 (the deterministic solver) or 1 (its stochastic form, SDE-DPM-Solver++), got %d", value);
        if (e->opt.solver_noise == value) return DR_OK;
        if (e->opt.solver != 0) (void)hipDeviceSynchronize();      // a chain of the previous value may still be reading the table
        e->opt.solver_noise = value;
        end_step_states(e);
        if (!e->committed || e->opt.solver == 0) return DR_OK;      // (dr_commit / "solver_order" builds it)
        return build_solver(e);
    }
    if (n == "start_step") {
        // (no captured chain is dropped: the effective start is part of the chain's key - GraphKey - as "draws" is; whether
        // the chain visits the step is checked by dr_sample, which knows the chain)
        if (value < -1 || value >= e->S)
            return fail(e, DR_EINVAL, "start_step is -1 (the chain's first step) or in [0, timesteps = %d), got %d", e->S, value);
        e->opt.start = value;
        return DR_OK;
    }
    if (n == "guidance_t_min" || n == "guidance_t_max") {
        // (no captured chain is dropped: the effective pair is part of the chain's key - GraphKey - as "draws" is; lo > hi is
        // refused by dr_step / dr_sample, once both values are in)
        const bool is_max = n == "guidance_t_max";
        if (!guidance_value_ok(is_max, value, e->S))
            return fail(e, DR_EINVAL, is_max ? "guidance_t_max is -1 (= timesteps - 1) or in [0, timesteps = %d), got %d"
                                             : "guidance_t_min is in [0, timesteps = %d), got %d", e->S, value);
        (is_max ? e->opt.guid.hi : e->opt.guid.lo) = value;
        return DR_OK;
    }
    if (n == "exact_below") {
        // (no captured chain is dropped by the set itself: the value is part of the chain's key - GraphKey - as "draws" is, so
        // a chain captured under another value is not replayed and one captured under this value still is.  No state of a
        // dr_step sequence depends on the mode: the roll, the history, the momentum and stride states are fp32)
        if (!exact_below_ok(value, e->S))
            return fail(e, DR_EINVAL, "exact_below is 0 (off) or v in [1, timesteps = %d]: the steps t < v run in exact fp32, got %d", e->S, value);
        e->opt.exact_below = value;
        return DR_OK;
    }
    if (!lab) return fail(e, DR_ENAME, "unknown option '%s'", name);
    if (n == "fused_stack_xcd") { put(e, e->opt_stack_xcd, value); return DR_OK; }
    if (n == "fused_stack_warm") { put(e, e->opt_stack_warm, value); return DR_OK; }
    if (n == "zero_taps") { put(e, e->opt_zero_taps, value != 0); return DR_OK; }
#ifdef DR_FAULT_HOOK
    if (n == "stack_fault_test") { put(e, e->opt_stack_fault, value); return DR_OK; }
#endif
    if (n == "stack_ticks") { put(e, e->stack_dbg_on, value); return DR_OK; }
    if (n.compare(0, 5, "tune.") == 0) {      // A/B knobs of planners and launchers: PROCESS-wide (kernels.h: Tuning)
        Tuning& t = tuning();
        const std::string f = n.substr(5);
        if (f == "ksplit_blocks") {
            if (put(e, t.ksplit_blocks, value)) tuning_epoch().fetch_add(1);
            return DR_OK;
        }
        std::atomic<int>* field = f == "pack_threads" ? &t.pack_threads : f == "tile" ? &t.tile : f == "pw" ? &t.pw : f == "pw_nw" ? &t.pw_nw
                   : f == "pwk" ? &t.pwk : f == "ksplit_max" ? &t.ksplit_max : f == "one_ks" ? &t.one_ks : f == "stack3" ? &t.stack3
                   : f == "stack_fl" ? &t.stack_fl : f == "tail_t4" ? &t.tail_t4 : f == "xcd_n" ? &t.xcd_n : f == "xcd_model" ? &t.xcd_model
                   : f == "s3_eager" ? &t.s3_eager : f == "debug_chunks" ? &t.debug_chunks : nullptr;
        if (!field) return fail(e, DR_ENAME, "unknown option '%s'", name);
        if (put(e, *field, value)) tuning_epoch().fetch_add(1);      // (part of every engine's chain key: each captures again at its next dr_sample)
        return DR_OK;
    }
    return fail(e, DR_ENAME, "unknown option '%s'", name);
}

// The opening dr_step and dr_sample share: the engine is ready for (sampler, B, T), the options are ones this call can run
// under, and the buffers its launches point into exist before anything is launched or captured.  step: dr_step's t, checked
// in its place; null for dr_sample, whose i0 is then the chain position option "start_step" names.  NB: the sampler's batch.
int open_chain_call(dr_engine* e, int sampler, int B, int T, const int* step, int& NB, int& i0, hipStream_t st) {
    int rc = check_ready(e, sampler, B, T);
    if (rc) return rc;
    if (step) {
        const int t = *step;
        if (t < 0 || t >= e->S) return fail(e, DR_EINVAL, "step %d out of range", t);
        if (e->steps.position(t) < 0)
            return fail(e, DR_EINVAL, "step %d is not visited by the respaced chain (option sampling_steps = %d)", t, e->opt.steps);
    }
    if ((rc = check_options(e, sampler, B, NB, T))) return rc;
    i0 = 0;
    if (!step && (rc = start_position(e, i0))) return rc;
    if ((rc = ensure_workspace(e, NB, T))) return rc;
    if (e->opt.solver == 2) {      // order 2: the history buffer (two halves)
        const size_t need = 2 * (size_t)B * T * 88;
        if (!e->hist.fits(need)) e->hist_key.valid = false;
        if ((rc = grow_chain_buffer(e, e->hist, need, st))) return rc;
    }
    const Stages stage = stages_of(e->opt, predicts_x0(sampler), NB == 2 * B);      // (what a step of this sampler can run, at some w)
    // option "x0_threshold": the work buffer of the threshold launches (tickets and counts start at zero: armed)
    if (stage.thresh && (rc = grow_chain_buffer(e, e->thresh_work, thresh_work_words(B), st))) return rc;
    // options "cfg_rescale" and "cfg_project" / "cfg_norm": the work buffer of the statistics launch (the ticket starts at zero: armed)
    if ((stage.rescale || stage.project) && (rc = grow_stats_work(e, B, T, st))) return rc;
    // option "cfg_momentum": the state, one float per roll element (a buffer that grew holds nothing)
    if (stage.momentum) {
        const size_t need = (size_t)B * T * 88;
        if (!e->momentum.fits(need)) e->mom_key.valid = false;
        if ((rc = grow_chain_buffer(e, e->momentum, need, st))) return rc;
    }
    // option "guidance_stride": the state, one float per roll element (a buffer that grew holds nothing)
    if (stage.stride) {
        const size_t need = (size_t)B * T * 88;
        if (!e->stride_d.fits(need)) e->stride_key.valid = false;
        if ((rc = grow_chain_buffer(e, e->stride_d, need, st))) return rc;
    }
    return DR_OK;
}

// What dr_sample was asked for; i0: the chain position of the first step it runs (option "start_step")
struct ChainCall { int sampler; const float* noise; int B, T; float w; uint64_t seed; int first_sample; int i0; };

// The reverse chain of one call, in place on xbuf, as launches on st - the caller's stream (eager) or the stream of a capture
int run_chain(dr_engine* e, const ChainCall& c, float* xbuf, hipStream_t st) {
    const size_t per = (size_t)c.B * c.T * 88;
    // the roll ping-pongs between xbuf and e->xalt while the fused step runs (its tail kernel cannot update in
    // place), and each tail also computes the next step's input projection
    ChainState cs;
    float* cur = xbuf;
    e->hist_par = 0;      // (option "solver_order": the first step reads no history - its row has c = 0)
    // option "start_noise": xbuf holds a clean roll - diffuse it to the first step, in place, in front of everything
    if (e->opt.start_noise)
        if (int r = run_diffuse(e, xbuf, c.noise, c.B, c.T, e->steps.at(c.i0), c.seed, c.first_sample, st)) return r;
    // every step t = S-1 .. 0, or the visited steps of option "sampling_steps" (run_step reads their rows) - from
    // position i0 on (option "start_step"; 0: the whole chain)
    for (int i = c.i0, n = e->steps.count(); i < n; ++i) {
        const int t = e->steps.at(i);
        // row t of the injected noise is the z of step t; t == 0 draws none (task/diffusion.py:957-960)
        const float* z = c.noise ? c.noise + (size_t)t * per : nullptr;
        cs.next_t = e->steps.at(i + 1);
        cs.x_out = cur == e->xalt ? xbuf : e->xalt;      // (the previous step left the roll in the engine's buffer: back into xbuf)
        float* res = nullptr;
        if (int r = run_step(e, c.sampler, cur, z, c.B, c.T, t, c.w, c.seed, c.first_sample, st, &res, &cs)) return r;
        cur = res;
    }
    if (cur != xbuf) HIPCHK(e, hipMemcpyAsync(xbuf, cur, per * sizeof(float), hipMemcpyDeviceToDevice, st));
    return DR_OK;
}

// What the capture of this call's chain bakes in (engine_state.h: GraphKey); NB: the sampler's evaluation batch
GraphKey chain_key(const dr_engine* e, const ChainCall& c, int NB) {
    GraphKey key;
    key.sampler = c.sampler; key.B = c.B; key.T = c.T; key.x = e->xwork; key.noise = c.noise; key.w_zero = (c.w == 0.f);
    key.opt = effective(e->opt, NB == 2 * c.B, e->S, e->steps.at(c.i0), key.w_zero);
    // option "exact_below": each node bakes its step's precision.  Under DR_PRECISION_F32 no step reads the value
    if (e->prec == DR_PRECISION_F32) key.opt.exact_below = 0;
    key.baked = e->baked; key.tuning = tuning_epoch().load();
    key.fe_B = e->fe_B;
    key.hist = e->opt.solver == 2 ? (const float*)e->hist : nullptr;
    // the buffers of the stages a step of this chain can run (the same question effective() asked for key.opt)
    const Stages stage = stages_of(e->opt, predicts_x0(c.sampler), NB == 2 * c.B && !key.w_zero);
    key.thresh_work = stage.thresh ? (const unsigned*)e->thresh_work : nullptr;
    key.stats_work = (stage.rescale || stage.project) ? (const unsigned*)e->stats_work : nullptr;
    key.momentum = stage.momentum ? (const float*)e->momentum : nullptr;
    key.stride = stage.stride ? (const float*)e->stride_d : nullptr;
    return key;
}

}  // namespace drh
using namespace drh;

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int dr_abi_version(void) { return DR_ABI_VERSION; }

const char* dr_last_error(const dr_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int dr_create(dr_engine** out, const dr_config* cfg) {
    if (!out || !cfg) return fail(nullptr, DR_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->abi_version != DR_ABI_VERSION)
        return fail(nullptr, DR_EINVAL, "ABI version mismatch: header %d, library %d", cfg->abi_version, DR_ABI_VERSION);
    if (cfg->residual_channels <= 0 || cfg->residual_channels % 4 || cfg->residual_layers <= 0 ||
        cfg->kernel_size <= 0 || cfg->kernel_size % 2 == 0 || cfg->n_mels <= 0 || cfg->timesteps <= 0 ||
        cfg->n_fft <= 0 || cfg->n_fft % 32 || cfg->hop_length <= 0 || cfg->hop_length % 4 ||
        cfg->dilation_base <= 0 || cfg->dilation_bound <= 0)
        return fail(nullptr, DR_EINVAL, "unsupported configuration");
    if (cfg->n_fft > (1 << 16) || cfg->residual_channels > (1 << 15))
        return fail(nullptr, DR_EINVAL, "configuration too large");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, DR_EHIP, "no HIP device available: the engine has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, DR_EINVAL, "device %d out of range", cfg->device);
    DeviceGuard guard(cfg->device);
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) return fail(nullptr, DR_EHIP, "hipSetDevice failed");
    }
    {
        hipError_t ie = init_kernels();
        if (ie != hipSuccess) return fail(nullptr, DR_EHIP, "kernel init failed: %s", hipGetErrorString(ie));
    }
    if (cfg->device >= MAX_DEVICES) return fail(nullptr, DR_EINVAL, "device %d out of range", cfg->device);
    if (!g_zero_vecs[cfg->device]) {
        void* z = nullptr;
        const size_t zn = 1 << 16;   // floats; covers every Cin on the path (n_fft, bins, channels)
        if (hipMalloc(&z, zn * sizeof(float)) != hipSuccess || hipMemset(z, 0, zn * sizeof(float)) != hipSuccess)
            return fail(nullptr, DR_EHIP, "allocating the zero vector failed");
        g_zero_vecs[cfg->device] = (const float*)z;
    }
    dr_engine* e = new dr_engine();
    e->cfg = *cfg;
    e->C = cfg->residual_channels;
    e->Cp = round_up(e->C, 64);
    e->L = cfg->residual_layers;
    e->K = cfg->kernel_size;
    e->S = cfg->timesteps;
    e->steps = ChainSteps(e->S, 0);
    e->NM = cfg->n_mels;
    e->n_bins = cfg->n_fft / 2 + 1;
    e->bins_p = round_up(e->n_bins, 64);
    for (int i = 0; i < e->L; ++i) {
        int d = 1;
        for (int q = 0; q < i % cfg->dilation_bound; ++q) d *= cfg->dilation_base;
        e->max_dil = std::max(e->max_dil, d);
    }
    if (gemm_lds_bytes(1, 1, e->K, e->max_dil, 1, EPI_GATE) > 160 * 1024) {
        const int rf = (e->K - 1) * e->max_dil;
        delete e;
        return fail(nullptr, DR_EINVAL, "receptive halo (k-1)*dil = %d does not fit the 160 KiB LDS tile", rf);
    }
    g_engines[cfg->device].fetch_add(1);
    {   // whose GPU is it?
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess)
            e->kfd_gpu_id = kfd_gpu_id(kfd_root(), prop.pciDomainID, prop.pciBusID, prop.pciDeviceID);
        // (only the FIRST engine of the process on this device may wait for the device in a doubtful look: later ones would
        // wait for their siblings' chains - and if those are what is busy, the fused slot already handles it)
        (void)fused_look(e, shared_with_another_process(e, false, g_engines[cfg->device].load() == 1));
    }
    *out = e;
    return DR_OK;
}

void dr_destroy(dr_engine* e) {
    if (!e) return;
    const int dev = e->cfg.device;
    DeviceGuard guard(dev);
    (void)hipDeviceSynchronize();
    forget_fused_slot(e);
    delete e;       // (the members' destructors release everything it holds, the captured chain first)
    if (g_engines[dev].fetch_sub(1) == 1) release_stager(dev);
}

int dr_set_param(dr_engine* e, const char* name, const float* host_data, size_t numel) {
    if (!e || !name || !host_data) return fail(e, DR_EINVAL, "null argument");
    const size_t want = expected_numel(e, name);
    if (want == 0) return fail(e, DR_ENAME, "unknown parameter '%s'", name);
    if (want != numel) return fail(e, DR_ENAME, "parameter '%s': expected %zu elements, got %zu", name, want, numel);
    e->params[name].assign(host_data, host_data + numel);
    e->committed = false;
    return DR_OK;
}

int dr_set_tables(dr_engine* e, const float* host_embedding, const float* host_coef) {
    if (!e || !host_embedding || !host_coef) return fail(e, DR_EINVAL, "null argument");
    e->h_emb.assign(host_embedding, host_embedding + (size_t)e->S * 128);
    e->h_coef.assign(host_coef, host_coef + (size_t)DR_COEF_FAMILIES * e->S * 5);
    e->committed = false;
    return DR_OK;
}

int dr_set_frontend_tables(dr_engine* e, const float* host_window, float window_norm, const float* host_fb) {
    if (!e) return DR_EINVAL;
    e->h_win.clear(); e->h_fb.clear(); e->h_win_norm = 0.f;
    if (host_window) {
        if (!(window_norm > 0.f)) return fail(e, DR_EINVAL, "window_norm must be positive");
        e->h_win.assign(host_window, host_window + e->cfg.n_fft);
        e->h_win_norm = window_norm;
    }
    if (host_fb) e->h_fb.assign(host_fb, host_fb + (size_t)e->n_bins * e->NM);
    e->committed = false;
    return DR_OK;
}

int dr_commit(dr_engine* e, void* stream) {
    if (!e) return DR_EINVAL;
    return commit(e, (hipStream_t)stream);
}

int dr_frontend(dr_engine* e, const float* d_wav, int B, int L, int T_roll, int mask_t0, int mask_t1, int mask_f0,
                int mask_f1, float* d_spec_out, void* stream) {
    if (!e || !d_wav) return fail(e, DR_EINVAL, "null argument");
    if (!e->committed) return fail(e, DR_ESTATE, "dr_commit has not been called");
    Range range("dr_frontend: mel + conditioner projections");
    DeviceGuard guard(e->cfg.device);
    hipStream_t st = (hipStream_t)stream;
    const int N = e->cfg.n_fft, hop = e->cfg.hop_length, pad = N / 2;
    if (B <= 0 || L <= pad || T_roll <= 0) return fail(e, DR_EINVAL, "bad front-end shape B=%d L=%d T=%d", B, L, T_roll);
    const int TF = L / hop + 1;
    const int T = std::min(T_roll, TF);
    const int Lp = (L + 2 * pad + 3) & ~3;
    const int Cp = e->Cp, NM = e->NM, bp = e->bins_p;
    const int mel_planes = (NM + 3) / 4;
    // (min, max) per clip / per frame, followed by the per-clip partials + ticket words of the multi-block min-max
    const size_t mm_vals = e->norm_framewise ? (size_t)B * TF * 2 : (size_t)B * 2;
    const size_t mm_need = mm_vals + minmax_scratch_floats(B), cond_need = (size_t)e->L * B * 2 * Cp * T;
    struct { DevBuf<float>& b; size_t n; } fe[] = {{e->wav_pad, (size_t)B * Lp}, {e->power, (size_t)B * bp * TF},
        {e->logmel, (size_t)B * mel_planes * 4 * TF}, {e->specP4, (size_t)B * mel_planes * 4 * T}, {e->mm, mm_need}, {e->cond, cond_need}};
    // the buffers grow (new zeroed blocks) only when a shape does: synchronise just then (a previous call may still be
    // reading them), not on every call
    bool fits = true;
    for (auto& f : fe) fits = fits && f.b.fits(f.n);
    if (!fits) HIPCHK(e, hipDeviceSynchronize());
    const bool mm_moved = !e->mm.fits(mm_need), cond_moved = !e->cond.fits(cond_need);
    for (auto& f : fe) HIPCHK(e, f.b.ensure(f.n, true));
    if (!mm_moved && e->mm_scratch_off != mm_vals)      // same buffer, other split: the ticket words must be zero where they now lie
        HIPCHK(e, hipMemsetAsync(e->mm, 0, e->mm.size() * sizeof(float), st));
    e->mm_scratch_off = mm_vals;
    if (cond_moved || B != e->fe_B || T != e->fe_T) {
        // a captured chain bakes the conditioner pointers / strides: stale when they change
        stale(e);
    }

    // 1. center / reflect padding
    HIPCHK(e, launch_reflect_pad(d_wav, e->wav_pad, B, L, pad, st));
    // 2. STFT power spectrum: frames are read straight out of the padded waveform (frame stride hop) - no framed
    //    copy.  FFT per frame (n_fft a power of two), else the windowed DFT as a GEMM.
    if (e->use_fft) {
        HIPCHK(e, launch_stft_power(e->wav_pad, e->fft_win, e->fft_tw, e->power, B, Lp, TF, N, hop, bp, e->fft_norm, st));
    } else {
        GemmArgs a{};
        a.Wp = e->dft_w; a.MT = bp / 64; a.bias = zero_vec();
        a.X = e->wav_pad; a.x_bs = Lp; a.x_ps = 4; a.x_fs = hop; a.x_planes = N / 4; a.kchunks = N / 32;
        a.NB = B; a.T = TF; a.taps = 1; a.dil = 1; a.alpha = 1.f;
        a.d2 = zero_vec();
        p4_out(a, e->power, bp / 4, TF, bp);
        HIPCHK(e, launch_gemm(a, EPI_POWER, 2, st));
    }
    // 3. mel filterbank + log(. + 1e-6)   (model/diffwave.py:644)
    {
        GemmArgs a = p4_gemm(e->mel_w, nullptr, (NM + 127) / 128, e->power, bp / 4, B, TF);
        if (e->use_fft) {     // power is (B, TF, bins) row-major: 4 bins per plane at stride 4, frames at stride bins
            a.x_bs = (long)TF * bp; a.x_ps = 4; a.x_fs = bp;
        }
        p4_out(a, e->logmel, mel_planes, TF, mel_planes * 4);
        HIPCHK(e, launch_gemm(a, EPI_LOG, 2, st));
    }
    // 4. imagewise min-max over the untrimmed TF frames, mask, trim
    if (e->norm_framewise) HIPCHK(e, launch_minmax_frame(e->logmel, e->mm, B, mel_planes, TF, NM, st));
    else HIPCHK(e, launch_minmax(e->logmel, e->mm, e->mm + e->mm_scratch_off, B, mel_planes, TF, NM, st));
    HIPCHK(e, launch_normalize(e->logmel, e->mm, e->specP4, d_spec_out, B, mel_planes, mel_planes, TF, T, NM,
                               mask_t0, mask_t1, mask_f0, mask_f1, st, e->norm_framewise));
    // 5. hoisted conditioner projections, one (B, 2C, T) tensor per layer (model/diffwave.py:143)
    for (int l = 0; l < e->L; ++l) {
        const LayerW& w = e->layers[l];
        GemmArgs a = p4_gemm(w.cond_w, w.cond_b, Cp / 64, e->specP4, mel_planes, B, T);
        p4_out(a, e->cond + (size_t)l * B * 2 * Cp * T, 2 * Cp / 4, T, 2 * Cp);
        HIPCHK(e, launch_gemm(a, EPI_PLAIN, 2, st));
    }
    e->fe_B = B;
    e->fe_T = T;
    return DR_OK;
}

int dr_forward(dr_engine* e, const float* d_x, int B, int T, int t, int cond, float* d_x0_out, void* stream) {
    if (!e || !d_x || !d_x0_out) return fail(e, DR_EINVAL, "null argument");
    DeviceGuard guard(e->cfg.device);
    const int sampler = cond == DR_COND_UNCOND ? DR_SAMPLER_GENERATION_DDPM_X0 : DR_SAMPLER_DDPM_X0;
    int rc = check_ready(e, sampler, B, T);
    if (rc) return rc;
    if (t < 0 || t >= e->S) return fail(e, DR_EINVAL, "step %d out of range", t);
    if ((rc = ensure_workspace(e, B, T))) return rc;
    FusedTurn turn(e, (hipStream_t)stream);
    if (turn.rc) return turn.rc;
    return run_network(e, d_x, 0, B, cond == DR_COND_UNCOND ? 0 : B, T, t, e->prec, d_x0_out, (hipStream_t)stream);
}

int dr_forward_steps(dr_engine* e, const float* d_x, int B, int T, const int32_t* host_t, int cond, float* d_x0_out,
                     void* stream) {
    if (!e || !d_x || !d_x0_out || !host_t) return fail(e, DR_EINVAL, "null argument");
    DeviceGuard guard(e->cfg.device);
    const int sampler = cond == DR_COND_UNCOND ? DR_SAMPLER_GENERATION_DDPM_X0 : DR_SAMPLER_DDPM_X0;
    int rc = check_ready(e, sampler, B, T);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
        if (host_t[b] < 0 || host_t[b] >= e->S) return fail(e, DR_EINVAL, "step %d of sample %d out of range", host_t[b], b);
    if ((rc = ensure_workspace(e, B, T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(e, hipStreamSynchronize(st));       // the previous call may still be reading the step buffer
    HIPCHK(e, e->d_tsel.ensure(B, false));
    HIPCHK(e, hipMemcpy(e->d_tsel, host_t, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    FusedTurn turn(e, st);
    if (turn.rc) return turn.rc;
    return run_network(e, d_x, 0, B, cond == DR_COND_UNCOND ? 0 : B, T, 0, e->prec, d_x0_out, st, false, e->d_tsel);
}

int dr_step(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T, int t, float w, uint64_t seed,
            int first_sample, void* stream) {
    if (!e || !d_x) return fail(e, DR_EINVAL, "null argument");
    DeviceGuard guard(e->cfg.device);
    int NB, i0;
    int rc = open_chain_call(e, sampler, B, T, &t, NB, i0, (hipStream_t)stream);
    if (rc) return rc;
    // Both pieces of engine state a step can continue are asked about before either is touched: a refusal changes nothing.
    // option "cfg_momentum": the state, over the steps that guide (chain_tables.h: momentum_step)
    const bool momentum = stages_of(e->opt, predicts_x0(sampler), NB == 2 * B && step_guided(e->opt.guid, e->S, w == 0.f, t)).momentum;
    MomentumVerdict mv{MomentumStep::STARTS, t};
    if (momentum) {
        mv = momentum_step(e->mom_key, sampler, B, T, t, e->steps, e->opt.start, e->opt.guid, e->S, w == 0.f);
        if (mv.what == MomentumStep::REFUSED)
            return fail(e, DR_ESTATE, "cfg_momentum = %d: dr_step at step %d continues no momentum state - the step expected next is %d "
                                      "(the chain's first guided step starts a new state; every other guided step follows the guided "
                                      "step before it)", e->opt.cfg_momentum, t, mv.expect);
    }
    // option "guidance_stride": the stored guidance update, over the steps that guide (chain_tables.h: stride_step)
    const bool strided = stages_of(e->opt, predicts_x0(sampler), NB == 2 * B && step_guided(e->opt.guid, e->S, w == 0.f, t)).stride;
    StrideVerdict sv{StrideStep::REFRESHES, t, 0};
    if (strided) {
        sv = stride_step(e->stride_key, sampler, B, T, t, e->steps, e->opt.start, e->opt.guid, e->S, w == 0.f, e->opt.guid_stride);
        if (sv.what == StrideStep::REFUSED)
            return fail(e, DR_ESTATE, "guidance_stride = %d: dr_step at step %d reuses no stored guidance update - the step expected next "
                                      "is %d (a step that refreshes - the chain's first guided step, every %d-th one behind it, step 0 - "
                                      "needs nothing; every other guided step follows the guided step before it)", e->opt.guid_stride, t,
                        sv.expect, e->opt.guid_stride);
    }
    if (e->opt.solver == 2) {
        // the history is engine state: t starts one or continues the one the previous dr_step left (chain_tables.h: history_step)
        const HistoryVerdict v = history_step(e->hist_key, sampler, B, T, t, e->steps, e->opt.start);
        if (v.what == HistoryStep::REFUSED)
            return fail(e, DR_ESTATE, "solver_order = 2: dr_step at step %d continues no history - the step expected next is %d "
                                      "(the chain's first step starts a new history; every other step follows its predecessor)", t, v.expect);
        if (v.what == HistoryStep::STARTS) e->hist_par = 0;
        e->hist_key.valid = false;      // (until the step has been issued)
    }
    if (momentum) {
        e->mom_start = mv.what == MomentumStep::STARTS;
        e->mom_key.valid = false;       // (until the step has been issued)
    }
    e->stride_reuse = strided && sv.what == StrideStep::REUSES;
    if (strided) e->stride_key.valid = false;      // (until the step has been issued)
    FusedTurn turn(e, (hipStream_t)stream);
    if (turn.rc) return turn.rc;
    if ((rc = write_windows(e, B, false, (hipStream_t)stream))) return rc;
    float* res = nullptr;
    if ((rc = run_step(e, sampler, d_x, d_noise, B, T, t, w, seed, first_sample, (hipStream_t)stream, &res))) return rc;
    if (res != d_x)      // the fused step wrote x_{t-1} into the engine's buffer: hand it back in place
        HIPCHK(e, hipMemcpyAsync(d_x, res, (size_t)B * T * 88 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (e->opt.solver == 2 && t > 0) { auto& k = e->hist_key; k.valid = true; k.sampler = sampler; k.B = B; k.T = T; k.t = t; }
    if (momentum) { auto& k = e->mom_key; k.valid = true; k.sampler = sampler; k.B = B; k.T = T; k.t = t; }
    if (strided) { auto& k = e->stride_key; k.valid = true; k.sampler = sampler; k.B = B; k.T = T; k.t = t; }
    return DR_OK;
}

int dr_sample(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T, float w, uint64_t seed,
              int first_sample, int use_graph, void* stream) {
    if (!e || !d_x) return fail(e, DR_EINVAL, "null argument");
    DeviceGuard guard(e->cfg.device);
    hipStream_t st = (hipStream_t)stream;
    int NB, i0;      // i0: the chain position of the first step this call runs (option "start_step")
    int rc = open_chain_call(e, sampler, B, T, nullptr, NB, i0, st);
    if (rc) return rc;
    e->hist_key.valid = false;      // (a whole chain uses the history buffers: a dr_step sequence does not continue across it)
    e->mom_key.valid = false;       // (... and the momentum state)
    e->stride_key.valid = false;    // (... and the stored guidance update)
    // (a yield is a precaution, not a verdict: the looks in front of later chains, >= 250 ms apart, may re-arm)
    if (e->fused.may_fuse()) fused_look(e, shared_with_another_process(e));
    FusedTurn turn(e, st);      // (released - event recorded on `st` - when this call returns, behind the chain's launches)
    if (turn.rc) return turn.rc;
    const ChainCall call{sampler, d_noise, B, T, w, seed, first_sample, i0};
    if (!use_graph || e->prof.on) {
        Range range("dr_sample: eager chain");
        if ((rc = write_windows(e, B, false, st))) return rc;
        return run_chain(e, call, d_x, st);
    }

    // (a held chain of another key is stale: the owner waits for its last launch and destroys it, then captures)
    GraphKey key;
    for (int attempt = 0; attempt < 2 && !e->chain.holds(key = chain_key(e, call, NB)); ++attempt) {
        Range range("dr_sample: capture + instantiate the chain graph");
        const auto cap = e->chain.capture(key, [&](hipStream_t cs) { return run_chain(e, call, e->xwork, cs); });
        if (cap.failed == Chain::Step::RECORD) return cap.rc;      // (the error text is the failing launch's own)
        if (cap.failed == Chain::Step::END) return fail(e, DR_EHIP, "%s failed: %s", cap.call, hipGetErrorString(cap.hip));
        if (!cap) return fail(e, DR_EHIP, "%s failed: %s (%s:%d)", cap.call, hipGetErrorString(cap.hip), __FILE__, __LINE__);
        // capture + instantiation took tens of milliseconds: look again before a chain of persistent launches goes out
        // (a yield makes the chain stale: the key moves, and the second attempt captures per phase)
        if (attempt == 0 && e->fused.active() && turn.held) fused_look(e, shared_with_another_process(e, true));
    }
    Range range("dr_sample: launch the chain graph");
    const size_t bytes = (size_t)B * T * 88 * sizeof(float);
    // the graph owns no caller address: x_T is copied in, the finished roll copied out (0.7 MB each way)
    HIPCHK(e, hipMemcpyAsync(e->xwork, d_x, bytes, hipMemcpyDeviceToDevice, st));
    // (the chain's tail launches publish epochs in win_epoch + 1 .. win_epoch + S, one per step: TailArgs::ready)
    HIPCHK(e, launch_set_dyn(e->d_dyn, seed, first_sample, w, (float)(1.0 + (double)w), e->win_epoch, st));
    if ((rc = write_windows(e, B, true, st))) return rc;      // (the captured chain reads the table of THIS call's marks)
    e->win_epoch += (unsigned)e->S;
    HIPCHK(e, e->chain.launch(st));
    if (e->stack_launches || e->tail_launches) { e->unverified = true; e->fused_stream = st; }      // (the captured chain may hold persistent launches)
    HIPCHK(e, hipMemcpyAsync(d_x, e->xwork, bytes, hipMemcpyDeviceToDevice, st));
    return DR_OK;
}

int dr_finish(dr_engine* e, void* stream) {
    if (!e) return DR_EINVAL;
    DeviceGuard guard(e->cfg.device);
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    if (e->unverified && e->fused_stream != (hipStream_t)stream) HIPCHK(e, hipStreamSynchronize(e->fused_stream));
    if (!e->sync.err_host || !*e->sync.err_host) {
        e->unverified = false;
        return DR_OK;
    }
    // A group barrier of the fused kernel gave up: something else held CUs while it ran (another engine / stream /
    // process on this device).  Everything computed since the last dr_finish is invalid.  Heal: wait for the
    // device, re-arm, and run this engine on the per-phase kernels from now on (bit-identical results, no
    // co-residency assumption) - the caller recomputes.
    HIPCHK(e, hipDeviceSynchronize());
    int rc = clear_stack_timeout(e);
    if (rc) return rc;
    stale(e);
    e->unverified = false;
    e->fused.timeout();         // (option "fused_rearm" may fuse again after clean chains; looks no longer do)
    static std::atomic<bool> warned{false};           // (engines of several host threads may get here together)
    if (!warned.exchange(true)) {
        fprintf(stderr, "[diffroll_amd] a group barrier of the fused residual-stack kernel timed out (another stream, engine or "
                        "process is computing on device %d): this engine now uses one launch per phase (option fused_stack = 0); "
                        "results since the last check are recomputed\n", e->cfg.device);
    }
    return fail(e, DR_ETIMEOUT, "a fused residual-stack launch timed out: results since the last dr_finish are invalid and must be "
                                "recomputed; the engine has been switched to per-phase launches (fused_stack = 0)");
}

int dr_sample_checked(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T, float w, uint64_t seed,
                      int first_sample, int use_graph, int32_t* recovered, void* stream) {
    if (recovered) *recovered = 0;
    if (!e || !d_x) return fail(e, DR_EINVAL, "null argument");
    if (B <= 0 || T <= 0) return fail(e, DR_EINVAL, "bad shape B=%d T=%d", B, T);
    DeviceGuard guard(e->cfg.device);
    hipStream_t st = (hipStream_t)stream;
    const size_t per = (size_t)B * T * 88;
    // only a fused launch can time out: keep x_T so that the chain can be re-run (a yielded engine may re-arm in dr_sample)
    const bool may_fuse = e->fused.may_fuse();
    if (may_fuse) {
        if (!e->xsave.fits(per)) {
            HIPCHK(e, hipStreamSynchronize(st));
            HIPCHK(e, e->xsave.ensure(per, false));
        }
        HIPCHK(e, hipMemcpyAsync(e->xsave, d_x, per * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    int rc = dr_sample(e, sampler, d_x, d_noise, B, T, w, seed, first_sample, use_graph, st);
    if (rc == DR_ETIMEOUT) {          // a flag left by unchecked earlier calls: clear it and carry on (nothing of THIS call ran)
        (void)dr_finish(e, st);
        rc = dr_sample(e, sampler, d_x, d_noise, B, T, w, seed, first_sample, use_graph, st);
    }
    if (rc) return rc;
    rc = dr_finish(e, st);
    // option "fused_rearm": the tenant that caused a time-out has had that many chains to leave - fuse again
    if (rc == DR_OK && e->fused.clean_chain()) stale(e);
    if (rc != DR_ETIMEOUT) return rc;
    if (!may_fuse) return rc;         // (guard: fusing was not possible on entry, so no fused launch was issued)
    HIPCHK(e, hipMemcpyAsync(d_x, e->xsave, per * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc = dr_sample(e, sampler, d_x, d_noise, B, T, w, seed, first_sample, use_graph, st);     // per-phase kernels now
    if (rc) return rc;
    rc = dr_finish(e, st);
    if (rc == DR_OK && recovered) *recovered = 1;
    if (rc == DR_OK) e->err.clear();
    return rc;
}

int dr_pending_timeout(dr_engine* e, void* stream) {
    if (!e || !e->sync.err_host) return DR_OK;
    if (e->unverified) {
        // the flag is final once the stream the fused launches ran on has drained - which need not be the stream the
        // consumer passes (a roll sampled on one stream, scored on another)
        DeviceGuard guard(e->cfg.device);
        HIPCHK(e, hipStreamSynchronize(e->fused_stream));
        if ((hipStream_t)stream != e->fused_stream) HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    }
    if (*e->sync.err_host)
        return fail(e, DR_ETIMEOUT, "a fused residual-stack launch issued on this engine timed out and has not been checked: the roll is "
                                    "invalid - call dr_finish (clears the condition, switches to per-phase launches) and recompute, or "
                                    "use dr_sample_checked");
    e->unverified = false;
    return DR_OK;
}

int dr_launch_state(dr_engine* e, dr_launch_info* out) {
    if (!e || !out) return DR_EINVAL;
    out->mode = e->last_mode;
    out->fused_enabled = e->fused.active();
    out->fallbacks = e->fused.fallbacks;
    out->yields = e->fused.yields;
    out->rearms = e->fused.rearms;
    out->stack_launches = e->stack_launches;
    out->tail_launches = e->tail_launches;
    return DR_OK;
}

int dr_note_runs(dr_engine* e, const float* d_roll, int B, int T, float threshold, int32_t* d_note_end, void* stream) {
    if (!e || !d_roll || !d_note_end) return fail(e, DR_EINVAL, "null argument");
    if (B <= 0 || T <= 0) return fail(e, DR_EINVAL, "bad shape B=%d T=%d", B, T);
    DeviceGuard guard(e->cfg.device);
    if (int rc = dr_pending_timeout(e, stream)) return rc;
    HIPCHK(e, launch_note_runs(d_roll, d_note_end, B, T, threshold, (hipStream_t)stream));
    return DR_OK;
}

int dr_frame_counts(dr_engine* e, const float* d_pred, const float* d_label, size_t n, float threshold,
                    int64_t* host_counts, void* stream) {
    if (!e || !d_pred || !d_label || !host_counts) return fail(e, DR_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(e->cfg.device);
    if (int rc = dr_pending_timeout(e, stream)) return rc;
    HIPCHK(e, e->d_counts.ensure(frame_counts_work_words(), true));      // (the ticket word starts at zero)
    HIPCHK(e, launch_frame_counts(d_pred, d_label, threshold, (long)n, e->d_counts, st));
    unsigned long long h[3];
    HIPCHK(e, hipMemcpyAsync(h, e->d_counts, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) host_counts[i] = (int64_t)h[i];
    return DR_OK;
}

static int noise_mix(dr_engine* e, int mode, const float* a, const float* b, const int64_t* d_t, const float* d_sac,
                     const float* d_s1m, int n_steps, int B, size_t per_sample, float* d_out, void* stream) {
    // e may be NULL (free functions of the reference: no engine state is involved; current device; the error text
    // is then read with dr_last_error(NULL))
    if (!a || !b || !d_t || !d_sac || !d_s1m || !d_out) return fail(e, DR_EINVAL, "null argument");
    if (B <= 0 || n_steps <= 0 || per_sample == 0) return fail(e, DR_EINVAL, "bad shape B=%d n_steps=%d", B, n_steps);
    if (int rc = dr_pending_timeout(e, stream)) return rc;
    HIPCHK(e, launch_noise_mix(mode, a, b, d_t, d_sac, d_s1m, n_steps, B, (long)per_sample, d_out, (hipStream_t)stream));
    return DR_OK;
}
int dr_q_sample(dr_engine* e, const float* d_x_start, const float* d_noise, const int64_t* d_t, const float* d_sac,
                const float* d_s1m, int n_steps, int B, size_t per_sample, float* d_out, void* stream) {
    return noise_mix(e, 0, d_x_start, d_noise, d_t, d_sac, d_s1m, n_steps, B, per_sample, d_out, stream);
}
int dr_extract_x0(dr_engine* e, const float* d_x_t, const float* d_epsilon, const int64_t* d_t, const float* d_sac,
                  const float* d_s1m, int n_steps, int B, size_t per_sample, float* d_out, void* stream) {
    return noise_mix(e, 1, d_x_t, d_epsilon, d_t, d_sac, d_s1m, n_steps, B, per_sample, d_out, stream);
}

int dr_set_option(dr_engine* e, const char* name, int value) { return drh::set_option(e, name, value, false); }

int dr_set_spec_norm(dr_engine* e, int mode) {
    if (!e) return DR_EINVAL;
    if (mode != DR_NORM_IMAGEWISE && mode != DR_NORM_FRAMEWISE) return fail(e, DR_EINVAL, "unknown normalisation mode %d", mode);
    e->norm_framewise = mode == DR_NORM_FRAMEWISE;
    return DR_OK;
}

int dr_set_precision(dr_engine* e, int mode) {
    if (!e) return DR_EINVAL;
    // (3 is reserved: refused like every other unknown value, the engine stays where it was)
    if (mode != DR_PRECISION_F32 && mode != DR_PRECISION_BF16X3 && mode != DR_PRECISION_BF16 && mode != DR_PRECISION_F16)
        return fail(e, DR_EINVAL, "unknown precision mode %d", mode);
    if (mode != e->prec) {
        DeviceGuard guard(e->cfg.device);
        stale(e);
        if (mode) {           // the mode changes only once its own packings exist (bf16x3: 520 MB of uploads, bf16 and f16: a third each - the build can fail)
            int rc = ensure_packings(e, mode);      // (adds buffers, frees and rewrites none: nothing to wait for)
            if (rc) return rc;
        }
        e->prec = mode;
    }
    return DR_OK;
}

}  // extern "C"
