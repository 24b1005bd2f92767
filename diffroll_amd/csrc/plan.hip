// Host side, part 2: the launch sequences of one network evaluation (run_network) and one reverse step (run_step).  What
// they launch - tile flavours, split-K factors, the fused-stack shape - is decided in launch_plan.h.
#include "engine_state.h"
#include "stride_quad.h"      // StrideUpd

namespace drh {

hipError_t launch_tiled(const GemmArgs& a, int epi, Tile t, hipStream_t s, int prec) {
    if (t.flavor == 3) return launch_pointwise_ksplit(a, t.n, s);
    if (t.flavor == 2) return launch_pointwise(a, t.n, s);
    return t.flavor == 1 ? launch_gemm16(a, epi, t.n, s) : launch_gemm(a, epi, t.n, s, prec);
}
// let the launcher split K when the launch under-fills the chip (single clips, narrow projections)
void allow_splitk(const dr_engine* e, GemmArgs& a) {
    a.ws = e->sk_ws; a.ws_cnt = e->sk_cnt;
    a.ws_floats = SK_WS_FLOATS; a.ws_cnt_n = SK_CNT_N;
}

// common GemmArgs for a P4 activation input [NB][planes][T][4]
// Device zero vector (a never-null bias / d2 operand: epilogue loads are unconditional), one per device, shared by
// the engines of the process on that device and never freed.
const float* g_zero_vecs[MAX_DEVICES] = {};
const float* zero_vec() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return (dev >= 0 && dev < MAX_DEVICES) ? g_zero_vecs[dev] : nullptr;
}

GemmArgs p4_gemm(const float* Wp, const float* bias, int MT, const float* X, int planes, int NB, int T) {
    GemmArgs a{};
    a.d2 = zero_vec();
    a.Wp = Wp; a.bias = bias ? bias : zero_vec(); a.MT = MT;
    a.X = X; a.x_bs = (long)planes * T * 4; a.x_ps = (long)T * 4; a.x_fs = 4; a.x_planes = planes;
    a.kchunks = (planes + 7) / 8;
    a.NB = NB; a.T = T; a.taps = 1; a.dil = 1; a.alpha = 1.f;
    return a;
}
void p4_out(GemmArgs& a, float* Y, int planes, int T, int rows) {
    a.Y = Y; a.y_bs = (long)planes * T * 4; a.y_ps = (long)T * 4; a.y_fs = 4; a.y_rows = rows;
}

// condition='trainable_spec' (model/diffwave.py:600-606, :656-658): the unconditional branch feeds the learned
// (n_mels, 641) spectrogram, trimmed to the roll length, through every layer's conditioner projection.  Like the
// conditional tensors it is hoisted: [L][2Cp/4][T][4], rebuilt when T changes (one-time, null stream).
int build_trainable_cond(dr_engine* e, int T) {
    const std::vector<float>* P = find_param(e, "trainable_parameters");
    if (!P) return DR_OK;
    if (e->cond_tr && e->cond_tr_T == T) return DR_OK;
    if (T > 641) return fail(e, DR_EINVAL, "condition='trainable_spec' holds 641 frames, roll has %d", T);
    const int NM = e->NM, Cp = e->Cp, mel_planes = (NM + 3) / 4;
    std::vector<float> sp((size_t)mel_planes * T * 4, 0.f);      // P4 image of P[:, :T]
    for (int m = 0; m < NM; ++m)
        for (int t = 0; t < T; ++t) sp[((size_t)(m >> 2) * T + t) * 4 + (m & 3)] = (*P)[(size_t)m * 641 + t];
    DevBuf<float> d_sp;         // (released after the device synchronisation below)
    HIPCHK(e, d_sp.ensure(sp.size(), false));
    HIPCHK(e, hipMemcpy(d_sp, sp.data(), sp.size() * sizeof(float), hipMemcpyHostToDevice));
    e->cond_tr.reset();
    HIPCHK(e, e->cond_tr.ensure((size_t)e->L * 2 * Cp * T, true));
    for (int l = 0; l < e->L; ++l) {
        const LayerW& w = e->layers[l];
        GemmArgs a = p4_gemm(w.cond_w, w.cond_b, Cp / 64, d_sp, mel_planes, 1, T);
        p4_out(a, e->cond_tr + (size_t)l * 2 * Cp * T, 2 * Cp / 4, T, 2 * Cp);
        HIPCHK(e, launch_gemm(a, EPI_PLAIN, 2, nullptr));
    }
    HIPCHK(e, hipDeviceSynchronize());
    e->cond_tr_T = T;
    return DR_OK;
}

int ensure_workspace(dr_engine* e, int NB, int T) {
    if (NB <= e->ws_NB && T == e->ws_T) return DR_OK;
    stale(e);       // a captured chain holds the addresses of the buffers that are about to be replaced
    const int nb = std::max(NB, e->ws_T == T ? e->ws_NB : 0);
    const size_t act = (size_t)nb * e->Cp * T, s3 = act + act / 2, roll = (size_t)nb * T * 88;
    struct { DevBuf<float>& b; size_t n; } ws[] = {{e->h, act}, {e->hd, act}, {e->hd3, s3}, {e->g3, s3}, {e->g, act},
        {e->skip, act}, {e->tmp, act}, {e->x0buf, roll}, {e->xwork, roll}, {e->xalt, roll}, {e->cond_dummy, (size_t)2 * e->Cp * T}};
    for (auto& w : ws) {        // new zeroed blocks of exactly this size (a smaller T shrinks them)
        w.b.reset();
        HIPCHK(e, w.b.ensure(w.n, true));
    }
    e->ws_NB = nb;
    e->ws_T = T;
    return build_trainable_cond(e, T);
}

// One network evaluation's arguments, as run_network received them.
struct Eval {
    dr_engine* e;
    const float* xin;              // (B,T,88) rows used modulo bmod
    int bmod, NB, n_cond, T, t;
    int prec;                      // the evaluation's precision (DR_PRECISION_*): the engine's mode, or the step's under "exact_below"
    float* x0_out;
    hipStream_t st;
    bool zero_spec;
    const int* tsel;               // (device, NB ints): per-sample diffusion steps; null: step t for all
};

// per-sample size (4-byte units) of the reduced-precision form of an activation tensor with Cp channels: the three bf16
// pieces of S3 (prec = 1) or the one 16-bit plane set (prec = 2 / 4: one_plane16)
static long lowp_bs(int prec, int Cp, int T) {
    const long act_bs = (long)Cp * T;
    return one_plane16(prec) ? act_bs / 2 : act_bs + act_bs / 2;
}
// S3 / one-plane 16-bit input description of an activation tensor with Cp channels
static void s3_in(GemmArgs& a, const float* X, int Cp, int T, int prec) {
    a.X = X; a.x_bs = lowp_bs(prec, Cp, T); a.x_piece = (long)(Cp / 8) * T * 4; a.x_ps = (long)T * 4; a.x_fs = 4;
    a.x_planes = Cp / 8; a.kchunks = Cp / 32;
}

// The profiling pass (dr_profile_*): the launch of the dominant kernel is bracketed by the next unused pair of events
// (none left, or not eligible: it runs untimed), then `account` adds its FLOPs and names it.
template <class Launch, class Account>
static int profiled(dr_engine* e, hipStream_t st, bool eligible, Launch&& launch, Account&& account) {
    const bool timed = e->prof.on && eligible && e->prof.used < e->prof.events.size();
    if (timed) HIPCHK(e, hipEventRecord(e->prof.events[e->prof.used].first, st));
    if (int rc = launch()) return rc;
    if (timed) {
        HIPCHK(e, hipEventRecord(e->prof.events[e->prof.used++].second, st));
        account();
    }
    return DR_OK;
}

// input projection + relu (model/diffwave.py:667-668)
static int launch_inproj(const Eval& v, const PlanKnobs& k) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, T = v.T;
    const long act_bs = (long)Cp * T;
    GemmArgs a{};
    a.Wp = e->in_w; a.bias = e->in_b; a.MT = (Cp + 127) / 128;
    a.X = v.xin; a.x_bs = (long)T * 88; a.x_ps = 4; a.x_fs = 88; a.x_planes = 22; a.x_bmod = v.bmod;
    a.kchunks = 3; a.NB = v.NB; a.T = T; a.taps = 1; a.dil = 1; a.alpha = 1.f;
    p4_out(a, e->h, Cp / 4, T, Cp);
    // hd = h + d_0 (model/diffwave.py:138-139), fp32 P4 or split-bf16 for the first dilated conv
    a.d2 = e->d_dtab + (v.tsel ? 0 : (size_t)v.t * e->L * Cp);
    a.tsel = v.tsel; a.d2_ts = (long)e->L * Cp;
    if (v.prec == 1) { a.Y2 = e->hd3; a.y2_bs = act_bs + act_bs / 2; a.out_s3 = 2; }
    else { a.Y2 = e->hd; a.y2_bs = act_bs; }
    allow_splitk(e, a);
    HIPCHK(e, launch_gemm(a, EPI_RELU, pick_ni(k, a.MT, v.NB, T, 1, 1), v.st));
    // (one-pass bf16 / f16: this fp32 kernel leaves hd in P4; the first conv's operand is its rounding)
    if (v.prec == DR_PRECISION_BF16) HIPCHK(e, launch_round_bf16(e->hd, e->hd3, v.NB, Cp, T, v.st));
    if (v.prec == DR_PRECISION_F16) HIPCHK(e, launch_round_f16(e->hd, e->hd3, v.NB, Cp, T, v.st));
    e->inproj_launches += 1;
    return DR_OK;
}

// phases [p0, p1) of the residual layers as fused launches (stack_kernel), one per sample chunk
static int launch_stack_range(const Eval& v, const NetPlan& p, int p0, int p1) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, L = e->L, T = v.T, prec = v.prec;
    const long act_n = (long)Cp * T, c_bs = (long)2 * Cp * T;
    int b0 = 0;
    for (int ck = 0; ck < p.stack_chunks; ++ck) {
        const int nb = v.NB / p.stack_chunks + (ck < v.NB % p.stack_chunks ? 1 : 0);      // balanced chunk sizes
        StackArgs sa{};
        sa.h = e->h + b0 * act_n; sa.hd = e->hd + b0 * act_n; sa.g = e->g + b0 * act_n; sa.skip = e->skip + b0 * act_n;
        if (prec) { sa.hd = e->hd3 + b0 * lowp_bs(prec, Cp, T); sa.g = e->g3 + b0 * lowp_bs(prec, Cp, T); }      // the S3 / one-plane tensors
        sa.d2 = e->d_dtab + (v.tsel ? 0 : (size_t)v.t * L * Cp);
        sa.tsel = v.tsel ? v.tsel + b0 : nullptr; sa.d2_ts = (long)L * Cp;
        sa.zero = zero_vec();
        sa.NB = nb; sa.T = T; sa.Cp = Cp; sa.taps = e->K; sa.L = L;
        sa.n_cond = std::max(0, std::min(nb, v.n_cond - b0));
        sa.c_bs = c_bs;
        // conditional sample b of this chunk is row b0 + b of the roll batch and reads clip (b0 + b) % fe_B (option "draws":
        // a chunk may start inside a draw and wrap); the layers' pointers below are the tensors' un-offset bases
        sa.c_b0 = b0 < v.n_cond ? b0 : 0; sa.c_n = e->fe_B;
        sa.p0 = p0; sa.p1 = p1;
        sa.xcd_n = e->opt_stack_xcd;
        sa.warm = e->opt_stack_warm;
        sa.zero_taps = e->opt_zero_taps;
        sa.fault = e->opt_stack_fault;
        sa.fold128 = e->opt_blocked >= 2;
        sa.bar = e->sync.bar(); sa.err = e->sync.err; sa.derr = e->sync.derr(); sa.xid = e->sync.xid();
        sa.dbg = e->stack_dbg_on ? e->stack_dbg : nullptr;
        for (int l = 0; l < L; ++l) {
            const LayerW& w = e->layers[l];
            StackLayer& y = sa.layer[l];
            y.conv_w = w.conv_w_of(prec); y.conv_b = w.conv_b;
            y.conv_b2 = v.zero_spec ? w.conv_b_z : w.conv_b_u;
            y.cond2 = nullptr;
            if (e->cond_tr && !v.zero_spec) { y.cond2 = e->cond_tr + (size_t)l * 2 * Cp * T; y.conv_b2 = w.conv_b; }
            // (a chunk without conditional samples keeps a readable pointer: the kernel prefetches, then ignores it)
            y.cond = e->cond ? e->cond + (size_t)l * e->fe_B * 2 * Cp * T : e->cond_dummy;
            y.out_w = w.out_w_of(prec); y.out_b = w.out_b; y.dil = w.dil;
        }
        int rc = profiled(e, v.st, true, [&]() -> int {
            HIPCHK(e, launch_stack(sa, p.stack_fl, e->max_dil, v.st, prec));
            e->stack_launches += 1;
            e->unverified = true; e->fused_stream = v.st;
            return DR_OK;
        }, [&] {
            const double C = e->C, fr = (double)nb * T;
            // executed work only: the last layer's 1x1 computes its skip half alone (the residual half is never read)
            for (int q = p0; q < p1; ++q)
                e->prof.flops += fr * 2.0 * C * 2.0 * C * ((q & 1) ? (q == 2 * L - 1 ? 0.5 : 1.0) : (double)e->K);
            e->prof.name = "stack_kernel<" + std::to_string(p.stack_fl) + "> (fused residual stack: dilated conv k=" +
                           std::to_string(e->K) + " + conditioner + gate and 1x1 + residual/skip, phases " +
                           std::to_string(p0) + ".." + std::to_string(p1 - 1) + " of " + std::to_string(2 * L) +
                           (p.stack_chunks > 1 ? ", " + std::to_string(p.stack_chunks) + " sample chunks" : "") +
                           (prec == DR_PRECISION_F16 ? (p.fold ? ", f16, blocked accumulation" : ", f16, one chain per output")
                            : prec == DR_PRECISION_BF16 ? (p.fold ? ", bf16, blocked accumulation" : ", bf16, one chain per output")
                            : prec ? (p.fold ? ", split-bf16, blocked accumulation" : ", split-bf16, one chain per output")
                                 : (p.fold ? ", blocked accumulation" : ", one fp32 chain per output")) + ")";
        });
        if (rc) return rc;
        b0 += nb;
    }
    return DR_OK;
}

// layer l's dilated conv of (h + d_l) + conditioner, gate (model/diffwave.py:138-147)
static int launch_conv(const Eval& v, const NetPlan& p, const PlanKnobs& k, int l) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, L = e->L, T = v.T, NB = v.NB, bmod = v.bmod, prec = v.prec;
    const LayerW& w = e->layers[l];
    GemmArgs a = p4_gemm(w.conv_w_of(prec), w.conv_b, Cp / 64, e->hd, Cp / 4, NB, T);
    if (prec) s3_in(a, e->hd3, Cp, T, prec);
    a.bias2 = v.zero_spec ? w.conv_b_z : w.conv_b_u;     // samples >= n_cond: spec == 0 or spec == -1
    if (e->cond_tr && !v.zero_spec) {                    // ... or the learned unconditional spectrogram
        a.cond2 = e->cond_tr + (size_t)l * 2 * Cp * T;
        a.bias2 = w.conv_b;
    }
    a.taps = e->K; a.dil = w.dil;
    a.fold128 = e->opt_blocked >= 2;
    a.zero_taps = e->opt_zero_taps;
    a.cond = e->cond ? e->cond + (size_t)l * e->fe_B * 2 * Cp * T : e->cond_dummy;
    a.c_bs = (long)2 * Cp * T;
    a.c_n = e->fe_B;        // (option "draws": conditional row b reads clip b % fe_B)
    a.n_cond = v.n_cond;
    p4_out(a, e->g, Cp / 4, T, Cp);
    if (prec) { a.Y = e->g3; a.y_bs = lowp_bs(prec, Cp, T); a.out_s3 = 1; }
    allow_splitk(e, a);
    // Classifier-free guidance evaluates the same x_t twice (samples b and b + bmod): in the first layer
    // both halves convolve the same h + d_0, so the contraction is done once per pair and the epilogue
    // writes both gated outputs (conditioner of b / constant unconditional bias).  Bit-identical.
    const bool dual = l == 0 && p.dual0;
    if (dual) {
        a.NB = bmod; a.dual = bmod; a.nofold64 = !p.fold;
        // (the single-chain 64-frame instance exists unsplit only, and it must be THE instance that runs - the tail
        // kernel's copy of this conv is what it has to agree with bit for bit: no split-K for this launch)
        if (a.nofold64) { a.ws = nullptr; a.ws_cnt = nullptr; }
    }
    const Tile tile = dual ? pick_tile(k, Cp / 64, bmod, T, e->K, w.dil, prec, EPI_GATE, false, e->opt_blocked >= 2)
                           : pick_tile(k, Cp / 64, NB, T, e->K, w.dil, prec, EPI_GATE, true, e->opt_blocked >= 2);
    if (e->stack_dbg_on && l + 1 == L) a.dbg = e->stack_dbg + 64;
    return profiled(e, v.st, !dual && p.stack_from < 0, [&]() -> int {
        HIPCHK(e, launch_tiled(a, EPI_GATE, tile, v.st, prec));
        return DR_OK;
    }, [&] {
        e->prof.flops += (double)NB * T * 2.0 * e->C * 2.0 * e->C * e->K;
        e->prof.name = "gemm_kernel<EPI_GATE> (dilated conv k=" + std::to_string(e->K) + " + conditioner + gate)";
    });
}

// layer l's 1x1 output projection, residual and skip (model/diffwave.py:149-151, :680)
static int launch_res_skip(const Eval& v, const PlanKnobs& k, int l) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, L = e->L, T = v.T, NB = v.NB, prec = v.prec;
    const long act_bs = (long)Cp * T;
    const LayerW& w = e->layers[l];
    GemmArgs a = p4_gemm(w.out_w_of(prec), w.out_b, Cp / 64, e->g, Cp / 4, NB, T);
    if (prec) s3_in(a, e->g3, Cp, T, prec);
    p4_out(a, e->h, Cp / 4, T, Cp);
    if (l + 1 < L) {
        a.d2 = e->d_dtab + ((v.tsel ? 0 : (size_t)v.t * L) + l + 1) * Cp;
        a.tsel = v.tsel; a.d2_ts = (long)L * Cp;
        if (prec) { a.Y2 = e->hd3; a.y2_bs = lowp_bs(prec, Cp, T); a.out_s3 = 2; }
        else { a.Y2 = e->hd; a.y2_bs = act_bs; }
    }
    a.skip = e->skip; a.s_bs = (long)Cp * T; a.skip_init = (l == 0);
    allow_splitk(e, a);
    if (e->stack_dbg_on && l + 2 == L) a.dbg = e->stack_dbg + 96;     // same tick marks as the fused kernel's
    Tile tile = pick_pointwise_tile(k, Cp / 64, NB, T, prec);
    // the last layer's residual output is never read (model/diffwave.py:678-682 only uses the skip sum
    // after the loop): launch the skip half of the M tiles only
    if (l + 1 == L && tile.flavor >= 2) {
        // packed rows [0, Cp) are the residual half: the first 128-row tile holding a skip row is Cp / 128
        // (when Cp is not a multiple of 128 that tile also recomputes a few residual rows: harmless)
        const int first = Cp / 128, count = Cp / 64 - first;
        const Tile half = pick_pointwise_tile(k, count, NB, T, prec, Cp / 32);
        if (half.flavor == tile.flavor) { tile = half; a.MT = count; a.mt0 = first; }
    }
    HIPCHK(e, launch_tiled(a, EPI_RES_SKIP, tile, v.st, prec));
    return DR_OK;
}

// the rest of the step in one launch (tail kernel): skip projection, output projection, combine + update, next input projection
static int launch_tail_step(const Eval& v, const NetPlan& p, const PlanKnobs& k, TailPlan* tail) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, L = e->L, T = v.T;
    // The successor's own plan decides what this tail leaves behind for it.  Under a guidance interval its shape may differ
    // from this step's (2B evaluations -> B or back): h / hd go to the rows it will read, and the shared first-layer conv
    // runs iff it is guided.  A successor that does not take the fused step (B evaluations may leave too much of the chip
    // idle for the fused stack: plan_network) is not primed at all - it starts with launch_inproj like a chain's first step.
    NetPlan np{};
    bool prime = false;
    if (tail->next_t >= 0) {
        np = plan_network(NetShape{tail->next.NB, tail->next.n_cond, v.bmod, T, Cp, L, e->K, e->max_dil, tail->next_prec, e->n_cus,
                                   e->fused.active(), e->opt_blocked, e->opt_tail, false, true}, k);
        prime = np.use_tail;
    }
    TailArgs ta{};
    ta.NB = v.NB; ta.T = T; ta.Cp = Cp; ta.BN = stack_tile_frames(p.stack_fl);
    ta.dual = (v.bmod > 0 && v.NB == 2 * v.bmod) ? v.bmod : 0;
    ta.u_B = tail->u_B;
    ta.xcd_n = e->opt_stack_xcd; ta.fault = e->opt_stack_fault;
    ta.alpha = (float)(1.0 / std::sqrt((double)L));
    ta.skip = e->skip; ta.tmp = e->tmp; ta.x0 = v.x0_out;
    ta.skip_w = e->skip_w; ta.skip_b = e->skip_b; ta.outp_w = e->outp_w; ta.outp_b = e->outp_b; ta.zero = zero_vec();
    ta.u = tail->u; ta.x_out = tail->x_out;
    if (prime) {
        ta.dual_next = np.dual0 ? v.bmod : 0;
        ta.in_w = e->in_w; ta.in_b = e->in_b; ta.d2_next = e->d_dtab + (size_t)tail->next_t * L * Cp;
        ta.h = e->h; ta.hd = e->hd;
        if (np.dual0) {       // the next step's shared first-layer conv (as the dual launch of launch_conv)
            const LayerW& w0 = e->layers[0];
            ta.conv_w = w0.conv_w; ta.conv_b = w0.conv_b;
            ta.conv_b2 = v.zero_spec ? w0.conv_b_z : w0.conv_b_u;
            if (e->cond_tr && !v.zero_spec) { ta.cond2 = e->cond_tr; ta.conv_b2 = w0.conv_b; }
            ta.cond = e->cond ? e->cond : e->cond_dummy;
            ta.c_bs = (long)2 * Cp * T; ta.c_n = e->fe_B;
            ta.taps = e->K; ta.dil = w0.dil;
            ta.fold = np.fold;
            ta.t4_ni = k.tail_t4;
            ta.g = e->g;
        }
    }
    ta.bar = e->sync.tail_bar(); ta.pbar = e->sync.tail_pbar(); ta.err = e->sync.err; ta.derr = e->sync.derr();
    // long-form windows: every window of the chain is in this one resident launch (the plan only takes the tail when
    // stack_chunks == 1), so the neighbour wait of T3 always has its neighbours running.  Epoch: position in the chain
    // for a captured one (added to DynParams::epoch at run time), else the next value of the engine's count.
    ta.ready = e->sync.ready();
    // S - t grows strictly along any chain, a respaced one (option "sampling_steps") included - its visited t decrease
    // strictly - and stays in [1, S], so the words keep growing across chains (dr_sample moves the base on by S per chain).
    ta.epoch = e->chain.capturing() ? (unsigned)(e->S - v.t) : ++e->win_epoch;
    // ticks 112..119 of dr_stack_status: the last tail launch of a chain that has a next step (all its parts run)
    ta.dbg = (e->stack_dbg_on && prime) ? e->stack_dbg + 112 : nullptr;
    HIPCHK(e, launch_tail(ta, v.st));
    e->tail_launches += 1;
    e->unverified = true; e->fused_stream = v.st;
    tail->done = true;
    tail->inproj_done = prime;
    return DR_OK;
}

// skip and output projections (model/diffwave.py:682-686)
static int launch_head(const Eval& v) {
    dr_engine* e = v.e;
    const int Cp = e->Cp, P = Cp / 4, T = v.T, NB = v.NB;
    {   // skip / sqrt(L) -> skip_projection -> relu (model/diffwave.py:682-684)
        GemmArgs a = p4_gemm(e->skip_w, e->skip_b, (Cp + 127) / 128, e->skip, P, NB, T);
        a.alpha = (float)(1.0 / std::sqrt((double)e->L));
        p4_out(a, e->tmp, P, T, Cp);
        allow_splitk(e, a);
        HIPCHK(e, launch_gemm(a, EPI_RELU, 1, v.st));   // M = C only: 64-frame tiles to fill more CUs
    }
    {   // output projection, written straight into the (B,T,88) roll layout (:685-686)
        GemmArgs a = p4_gemm(e->outp_w, e->outp_b, 1, e->tmp, P, NB, T);
        a.Y = v.x0_out; a.y_bs = (long)T * 88; a.y_ps = 4; a.y_fs = 88; a.y_rows = 88;
        allow_splitk(e, a);
        HIPCHK(e, launch_gemm(a, EPI_PLAIN, 1, v.st));  // M = 88 (one row tile): 64-frame tiles
    }
    return DR_OK;
}

// One network evaluation for NB samples (first n_cond conditional) at step t.
//   xin (B,T,88) rows are used modulo bmod (classifier-free batching: 2B evaluations of B inputs).
// It carries out the plan of launch_plan.h: the layers one launch per phase, or fused launches (stack_kernel) - and, when
// run_step offered the fused step and the plan takes it, the tail kernel instead of the head projections and the update.
int run_network(dr_engine* e, const float* xin, int bmod, int NB, int n_cond, int T, int t, int prec, float* x0_out,
                hipStream_t st, bool zero_spec, const int* tsel, TailPlan* tail) {
    // tsel (device, NB ints): per-sample diffusion steps (forward() with a (B,) step tensor); else step t for all
    const Eval v{e, xin, bmod, NB, n_cond, T, t, prec, x0_out, st, zero_spec, tsel};
    const PlanKnobs k = plan_knobs();
    const NetPlan p = plan_network(NetShape{NB, n_cond, bmod, T, e->Cp, e->L, e->K, e->max_dil, prec, e->n_cus, e->fused.active(),
                                            e->opt_blocked, e->opt_tail, tsel != nullptr, tail != nullptr}, k);
    e->last_mode = p.mode;      // dr_launch_state
    // h / hd of this step (and, guided, layer 0's g) were already written by the previous step's tail kernel - for an
    // evaluation of exactly this shape (the rows written and whether layer 0's g exists depend on it)
    const bool primed = p.use_tail && tail->skip_inproj && tail->primed.NB == NB && tail->primed.n_cond == n_cond &&
                        tail->primed.dual == p.dual0;
    int rc;
    if (!primed && (rc = launch_inproj(v, k))) return rc;
    if (p.stack_from >= 0) {
        // (a guided pair's first conv is a launch of its own; everything from its 1x1 on is one launch)
        if (p.stack_from == 1 && !primed) {
            if ((rc = launch_conv(v, p, k, 0))) return rc;
            e->conv0_launches += 1;
        }
        if ((rc = launch_stack_range(v, p, p.stack_from, 2 * e->L))) return rc;
    } else {
        for (int l = 0; l < e->L; ++l)
            if ((rc = launch_conv(v, p, k, l)) || (rc = launch_res_skip(v, k, l))) return rc;
    }
    return p.use_tail ? launch_tail_step(v, p, k, tail) : launch_head(v);
}

int sampler_shape(int sampler, int B, int& NB, int& n_cond, int& family, bool& zero_spec) {
    zero_spec = false;
    switch (sampler) {
        case DR_SAMPLER_DDPM_X0: NB = B; n_cond = B; family = DR_COEF_DDPM_X0; return DR_OK;
        case DR_SAMPLER_CFDG_DDPM_X0:
        case DR_SAMPLER_INPAINTING_DDPM_X0: NB = 2 * B; n_cond = B; family = DR_COEF_DDPM_X0; return DR_OK;
        case DR_SAMPLER_GENERATION_DDPM_X0: NB = B; n_cond = 0; family = DR_COEF_DDPM_X0; return DR_OK;
        case DR_SAMPLER_DDIM_X0: NB = B; n_cond = B; family = DR_COEF_DDIM_X0; return DR_OK;
        case DR_SAMPLER_CFDG_DDIM_X0: NB = 2 * B; n_cond = B; family = DR_COEF_DDIM_X0; zero_spec = true; return DR_OK;
        case DR_SAMPLER_DDPM_EPS: NB = B; n_cond = B; family = DR_COEF_DDPM_EPS; return DR_OK;
        case DR_SAMPLER_DDIM_EPS: NB = B; n_cond = B; family = DR_COEF_DDIM_EPS; return DR_OK;
        case DR_SAMPLER_DDIM2DDPM_EPS: NB = B; n_cond = B; family = DR_COEF_DDIM2DDPM_EPS; return DR_OK;
    }
    return DR_EINVAL;
}
int sampler_shape(int sampler, int B, int& NB, int& n_cond) {
    int fam; bool z;
    return sampler_shape(sampler, B, NB, n_cond, fam, z);
}

UpdateArgs update_base(const dr_engine* e, int B, int T) {
    UpdateArgs u{};
    u.n = (long)B * T * 88; u.per_sample = (long)T * 88;
    u.dyn = e->chain.capturing() ? e->d_dyn : nullptr;
    // (option "window_blend" rides in the word's spare bits - kernels.h: win_H / win_blend; check_options keeps T below them)
    u.win = e->opt.win_O > 0 ? (T - e->opt.win_O) | (e->opt.win_blend << WIN_BLEND_SHIFT) : 0;
    // option "draws": the rows' Philox keys (update_quad.h); windows carry theirs in the table (chain_tables.h: window_table)
    if (e->opt.draws > 1) { u.draw_n = B / e->opt.draws; u.draw_G = e->opt.draw_G > 0 ? e->opt.draw_G : u.draw_n; }
    // recording boundaries (option "window_break"): the engine's table - always in a captured chain, so that new marks
    // replay the same graph; without marks an eager chain keeps the one-recording definition (null)
    // (the table has STACK_GROUPS words: a larger batch is one recording - check_options refuses marks there)
    u.win_tab = (u.win > 0 && B <= STACK_GROUPS && (e->chain.capturing() || !e->win_marks.empty() || e->opt.draws > 1)) ? (const unsigned*)e->d_wintab : nullptr;
    return u;
}

// One reverse step.  The result is written in place on x - or, when the fused step ran (tail kernel), into e->xalt (or
// chain->x_out): *result tells which; chain (optional) carries "h / hd of this step are already there" from step to step.
int run_step(dr_engine* e, int sampler, float* x, const float* noise, int B, int T, int t, float w, uint64_t seed,
             int first_sample, hipStream_t st, float** result, ChainState* chain) {
    int NB, n_cond, family;
    bool zero_spec;
    if (sampler_shape(sampler, B, NB, n_cond, family, zero_spec)) return fail(e, DR_EINVAL, "unknown sampler %d", sampler);
    // Guidance weight 0: x0 = (1 + 0) c - 0 u = c (task/diffusion.py:953) - the unconditional evaluation is
    // multiplied by zero, so it is not run (half the work; the w = 0 points of the paper's guidance sweeps).  A step
    // outside the guidance interval (options "guidance_t_min" / "guidance_t_max") is that step, whatever the caller's w;
    // w == 0 is the empty interval (launch_plan.h: plan_step).
    const bool guiding = NB == 2 * B;
    // option "guidance_stride": a step that guides refreshes or reuses by its ordinal among the guided steps of the chain -
    // counted along the chain, or dr_step's verdict; a captured chain bakes it into the node.  A reuse step is the
    // conditional evaluation alone, and so is planned as a step outside the interval is (launch_plan.h: plan_step)
    const int stride = guiding ? guidance_stride(e) : 0;
    const bool strided = stride > 1 && step_guided(e->opt.guid, e->S, w == 0.f, t);
    bool reuse = false, reuse_next = false;
    if (strided) {
        reuse = chain ? !stride_refreshes(stride, chain->guided_k, t) : e->stride_reuse;
        if (chain) chain->guided_k += 1;
    }
    if (stride > 1 && chain && chain->next_t >= 0 && step_guided(e->opt.guid, e->S, w == 0.f, chain->next_t))
        reuse_next = !stride_refreshes(stride, chain->guided_k, chain->next_t);
    const StepShapes shapes = plan_step(NB, n_cond, B, e->opt.guid, e->S, w == 0.f, t, chain ? chain->next_t : -1, reuse, reuse_next);
    NB = shapes.now.NB; n_cond = shapes.now.n_cond;
    if (guiding && !shapes.now.dual) w = 0.f;
    UpdateArgs u = update_base(e, B, T);
    u.x = x; u.x0c = e->x0buf; u.x0u = (NB == 2 * B) ? e->x0buf + (size_t)B * T * 88 : nullptr;
    // row t of the family's table: the committed one, or under option "sampling_steps" the row for t's successor in the
    // respaced chain (chain_tables.h: respaced_table; unvisited rows are never read)
    const float* coef = e->steps.respaced() ? e->d_coef_rs : e->d_coef;
    u.noise = noise; u.coef = coef + ((size_t)family * e->S + t) * 5; u.t = t; u.mode = family;
    u.w = w; u.onepw = (float)(1.0 + (double)w);
    u.seed = seed; u.first_sample = first_sample;
    // option "solver_order" (the callers have refused the epsilon samplers): the solver's own row and update.  Noise and
    // seed are read only where the row's c4 is not 0 (option "solver_noise": the z of the DDPM updates at this step).  Order
    // 2 reads the previous step's prediction where the row says so and leaves this step's for the next (the two halves of
    // the history buffer, ping-pong); order 1 neither reads nor stores.
    if (e->opt.solver != 0 && predicts_x0(sampler)) {
        const bool hist = e->opt.solver == 2;
        // (option "start_step": the step it names is a chain's first - the copy of its row with c = 0, chain_tables.h: solver_table)
        u.coef = e->d_solver + ((size_t)(t == e->opt.start ? e->S : 0) + t) * 5; u.mode = 5;
        u.hist = hist ? (float*)e->hist : nullptr; u.hist_par = hist ? e->hist_par : 0;
        if (hist) e->hist_par ^= 1;
    }
    // option "x0_clip" (the callers have refused the epsilon samplers): the update clamps the prediction it consumes
    if (e->opt.x0_clamp != 0 && predicts_x0(sampler)) { u.clamp_lo = e->opt.x0_clamp == 2 ? -1.f : 0.f; u.clamp_hi = 1.f; }
    float* const xalt = chain && chain->x_out ? chain->x_out : e->xalt;
    TailPlan plan;
    plan.u = u; plan.x_out = xalt; plan.u_B = B;
    plan.next_t = chain ? chain->next_t : -1;
    plan.next = shapes.next;
    // option "exact_below": the precision is a property of the step.  The visited t decrease, so every exact step lies behind
    // every reduced one: a reduced step takes no tail kernel and primes nothing, the first exact step computes its own input
    // layer, and the tail kernel of an exact step primes an exact successor (launch_plan.h: step_precision)
    const int prec = step_precision(e->prec, e->opt.exact_below, t);
    plan.next_prec = plan.next_t >= 0 ? step_precision(e->prec, e->opt.exact_below, plan.next_t) : prec;
    plan.skip_inproj = chain && chain->inproj_ready;
    if (chain) plan.primed = chain->ready;
    // (x and the tail kernel's output buffer must differ: a caller that hands us xalt itself gets the unfused tail)
    // option "x0_threshold": the selection sits between the network and the update, so the step offers no tail plan - the
    // evaluation keeps its fused stack launch, the head projections write e->x0buf, the rest are ordinary launches
    // option "cfg_rescale": likewise at a step that guides - the statistics sit between the network and everything that reads
    // the prediction; a step that runs no unconditional evaluation does not read the option and keeps its tail kernel
    // options "cfg_project" / "cfg_norm": likewise (check_options has refused them beside "x0_threshold" and "cfg_rescale")
    // option "guidance_stride": likewise at a step that guides, a refresh or a reuse - the stride form of the update stands
    // behind the head projections (check_options has refused the options above beside it)
    const Stages stage = stages_of(e->opt, predicts_x0(sampler), u.x0u != nullptr || strided);
    TailPlan* offer = (result && x != xalt && !stage.thresh && !stage.rescale && !stage.project && !stage.stride) ? &plan : nullptr;
    if (chain) chain->inproj_ready = false;
    int rc = run_network(e, x, B, NB, n_cond, T, t, prec, e->x0buf, st, zero_spec, nullptr, offer);
    if (rc) return rc;
    if (offer && plan.done) {
        *result = xalt;
        if (chain) { chain->inproj_ready = plan.inproj_done; chain->ready = plan.next; }
        return DR_OK;
    }
    if (result) *result = x;
    if (stage.stride) {       // update that stores d = y - c, or consumes c + d
        HIPCHK(e, launch_update_stride(u, StrideUpd{e->stride_d, reuse ? 1 : 0}, st));
        return DR_OK;
    }
    if (stage.project) {      // statistics, update on (a c) + (b y)
        const ProjectArgs pa = project_args(e, u);
        if (stage.momentum) {
            // option "cfg_momentum": the same two launches in their momentum form, over the engine's state.  Whether this
            // step starts the state is a fact of the chain - its first guided step - or dr_step's verdict; a captured chain
            // bakes it into the node
            const bool start = chain ? !chain->guided : e->mom_start;
            if (chain) chain->guided = true;
            float* const m = e->momentum;
            HIPCHK(e, launch_momentum(MomentumArgs{pa, start ? nullptr : m, momentum_bf(e)}, B, st));
            HIPCHK(e, launch_update_momentum(u, MomentumUpd{gs_records(pa.work), m, momentum_bf(e), start ? 1 : 0}, st));
            return DR_OK;
        }
        HIPCHK(e, launch_project(pa, B, st));
        HIPCHK(e, launch_update_project(u, ProjectUpd{gs_records(pa.work)}, st));
        return DR_OK;
    }
    if (stage.rescale) {      // statistics, [threshold launches ranking |g y - m|], update on g y
        const RescaleArgs ra = rescale_args(e, u);
        RescaleUpd rs{gs_records(ra.work), ThreshUpd{nullptr, 0.f, 0.f}};
        HIPCHK(e, launch_rescale(ra, B, st));
        if (stage.thresh) {
            const ThreshArgs ta = thresh_args(e, u);
            HIPCHK(e, launch_threshold_rescaled(ta, rs.g, B, st));
            rs.th = ThreshUpd{reinterpret_cast<const float*>(ta.work + THRESH_HEAD + THRESH_QS), ta.m, ta.r};
        }
        HIPCHK(e, launch_update_rescale(u, rs, st));
        return DR_OK;
    }
    if (stage.thresh) {
        const ThreshArgs ta = thresh_args(e, u);
        HIPCHK(e, launch_threshold(ta, B, st));
        HIPCHK(e, launch_update_thresh(u, ThreshUpd{reinterpret_cast<const float*>(ta.work + THRESH_HEAD + THRESH_QS), ta.m, ta.r}, st));
        return DR_OK;
    }
    HIPCHK(e, launch_update(u, st));
    return DR_OK;
}

ThreshArgs thresh_args(const dr_engine* e, const UpdateArgs& u) {
    ThreshArgs a{};
    a.u = u;
    // m = (lo + hi) / 2, r = (hi - lo) / 2 of the range "x0_clip" names: [0, 1] or [-1, 1], both exact
    a.m = 0.5f * (u.clamp_lo + u.clamp_hi); a.r = 0.5f * (u.clamp_hi - u.clamp_lo);
    a.v = e->opt.x0_thresh;
    a.work = e->thresh_work;
    return a;
}

RescaleArgs rescale_args(const dr_engine* e, const UpdateArgs& u) {
    RescaleArgs a{};
    a.u = u;
    a.phi = e->opt.cfg_rescale;
    a.work = e->stats_work;
    return a;
}

ProjectArgs project_args(const dr_engine* e, const UpdateArgs& u) {
    ProjectArgs a{};
    a.u = u;
    a.rho = e->opt.cfg_project;
    a.norm = e->opt.cfg_norm;
    a.work = e->stats_work;
    return a;
}

}  // namespace drh
