// Philox4x32-10 + Box-Muller, the posterior update and the multistep solver update of one roll quad: shared by
// update_kernel (update.hip) and part T3 of the tail kernel (tail.hip) - identical arithmetic.
#pragma once
#include "device_common.h"

namespace dr {

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller: z ~ N(0,1), keyed by (seed, global sample, step, element/4) so the
// noise of a sample does not depend on how the batch is sharded over GPUs.
// ---------------------------------------------------------------------------------------------
DR_DEVINL void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                             uint32_t (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

DR_DEVINL void box_muller(uint32_t u0, uint32_t u1, float& z0, float& z1) {
    const float a = ((float)(u0 >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
    const float bb = (float)(u1 >> 8) * (1.0f / 16777216.0f);           // [0, 1)
    const float rad = sqrtf(-2.0f * logf(a));
    float sn, cs;
    sincosf(6.283185307179586f * bb, &sn, &cs);
    z0 = rad * cs;
    z1 = rad * sn;
}

// THE NOISE-KEY RULE, stated once: which Philox (sample key sk, quad q) belongs to a float4 of the roll batch.  Used by
// update_quad (the z of a reverse step, counter word 2 = t) and by diffuse_kernel (update.hip: the z of option
// "start_noise", counter word 2 = timesteps + the start step).
//   a window (win_H(a) > 0) is window idx of recording rec of the batch - the table's word (options "window_break" /
//   "draws": the draw is part of rec), else window smp of recording 0 - and is keyed by its recording and the element on
//   that recording's canvas: two windows draw the same z on the frames they share;
//   a clip is keyed by its row, or under option "draws" (a.draw_n > 0) as draw smp / n of clip smp % n.
// (update_quad reads the table's word itself, inside its test for neighbouring windows: calling window_place there costs
// the tail kernel one more scalar parked in a VGPR lane - profiles/start_kernel_resources.txt - so only the two key
// functions are shared code; the word's meaning is window_rec / window_idx of kernels.h in both.)
DR_DEVINL void window_place(const UpdateArgs& a, const long smp, long& rec, long& idx) {
    rec = 0; idx = smp;
    if (a.win_tab) {
        const unsigned me = a.win_tab[smp];
        rec = window_rec(me); idx = window_idx(me);
    }
}
// within: the quad's first element inside its window
DR_DEVINL void window_key(const UpdateArgs& a, const long rec, const long idx, const long within, const int first_sample,
                          long& q, long& sk) {
    sk = first_sample + rec;
    q = (idx * win_H(a) * 88 + within) >> 2;
}
DR_DEVINL void clip_key(const UpdateArgs& a, const long i4, const int first_sample, long& q, long& sk) {
    const long e0 = i4 * 4;
    const long smp = e0 / a.per_sample;
    q = (e0 - smp * a.per_sample) >> 2;
    // (option "draws": draw smp / n of clip smp % n)
    sk = a.draw_n > 0 ? first_sample + smp % a.draw_n + (smp / a.draw_n) * a.draw_G : first_sample + smp;
}

// The guided prediction of one float4 (index i4) of the roll: (1 + w) x0c - w x0u, or x0c alone (task/diffusion.py:953).
DR_DEVINL void guided_quad(const UpdateArgs& a, const long i4, const float gw, const float g1pw, float (&y)[4]) {
#pragma clang fp contract(off)
    const float4 xc = reinterpret_cast<const float4*>(a.x0c)[i4];
    y[0] = xc.x; y[1] = xc.y; y[2] = xc.z; y[3] = xc.w;
    if (a.x0u) {
        const float4 xu = reinterpret_cast<const float4*>(a.x0u)[i4];
        const float u[4] = {xu.x, xu.y, xu.z, xu.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = g1pw * y[e] - gw * u[e];
    }
}

// Classifier-free combine + x0-prediction posterior update of ONE float4 (4 consecutive elements, index i4) of the
// roll.  Same operation order as task/diffusion.py:953 and :957-967; contraction off so that no FMA is formed where
// the reference rounds twice.  Shared by update_kernel and the tail kernel (identical arithmetic).
// Long-form windows (win_H(a) > 0, UpdateArgs): on a frame shared with a neighbouring window of the same recording the prediction is the mean
// 0.5f * (y_lower + y_upper) of both windows' guided predictions - the same bits in both (the operands are the same
// two values, added in the same order) - or what option "window_blend" makes of the two (blend_quad below) - and the noise
// is keyed by the canvas element.
// mode 5 (option "solver_order", x0-prediction samplers): the exponential integrator in lambda = log(sqrt_acp / sqrt_1m_acp)
// of Lu et al. 2022 (DPM-Solver++), row [sqrt_1m_acp' / sqrt_1m_acp, -sqrt_acp' expm1(-h), sqrt_acp, c, 0] (chain_tables.h:
// solver_table).  y is the guided prediction after the shared-frame mean, p the y of the previous step (hist_prev(a)):
//   d = c != 0 ? y + c (y - p) : y      (2M; c = h / (2 h_prev), 0 = first order: p is not loaded)
//   o = c0 x + c1 d;   t == 0: o = y / c2, the x0 samplers' own last step
// One fp32 rounding per operation, no noise (deterministic).  The caller stores y to hist_next(a) for the next step
// (update_quad hands it out): in the tail kernel several blocks recompute a quad and one of them stores.
// Option "solver_noise" (SDE-DPM-Solver++, same paper): the row is [(sqrt_1m_acp' / sqrt_1m_acp) exp(-h), -sqrt_acp'
// expm1(-2h), sqrt_acp, c, sqrt_1m_acp' sqrt(-expm1(-2h))] and o = (c0 x + c1 d) + c4 z at t > 0, z the step's noise_quad -
// the z update_quad's DDPM modes draw at that step.  The deterministic rows have c4 = 0 exactly and take the expression
// without the last term: the option at 0 changes no bit.
DR_DEVINL float4 solver_quad(const UpdateArgs& a, const long i4, const float (&y)[4], const float (&x)[4], const bool noisy,
                             const float (&z)[4]) {
#pragma clang fp contract(off)
    const float c0 = a.coef[0], c1 = a.coef[1], c2 = a.coef[2], c = a.coef[3];
    float o[4];
    if (a.t == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = y[e] / c2;
        return make_float4(o[0], o[1], o[2], o[3]);
    }
    float d[4] = {y[0], y[1], y[2], y[3]};
    if (c != 0.f) {
        const float4 pv = reinterpret_cast<const float4*>(hist_prev(a))[i4];
        const float p[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = y[e] + c * (y[e] - p[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c0 * x[e] + c1 * d[e];
    if (noisy) {
        const float c4 = a.coef[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] + c4 * z[e];
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// The z of one float4 at step a.t: the quad of the injected noise, or Philox by the noise-key rule above (key_smp >= 0: the
// window key update_quad has worked out; else the clip's).  Shared by every update that draws noise - the DDPM modes and
// mode 5 under option "solver_noise".
DR_DEVINL void noise_quad(const UpdateArgs& a, const long i4, const long key_smp, const long key_q, const int first_sample,
                          const uint64_t seed, float (&z)[4]) {
    if (a.noise) {
        const float4 zv = reinterpret_cast<const float4*>(a.noise)[i4];
        z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else {
        long within, sk;
        if (key_smp >= 0) { within = key_q; sk = key_smp; }
        else clip_key(a, i4, first_sample, within, sk);
        uint32_t rnd[4];
        philox4x32_10((uint32_t)within, (uint32_t)(within >> 32), (uint32_t)a.t,
                      (uint32_t)sk, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
        box_muller(rnd[0], rnd[1], z[0], z[1]);
        box_muller(rnd[2], rnd[3], z[2], z[3]);
    }
}

// Option "x0_clip" (a.clamp_lo < a.clamp_hi: [0, 1] or [-1, 1]; else off): the static clamp of the prediction the update
// consumes ("clip_denoised" of the DDPM code bases, the static thresholding DPM-Solver++ was published with).
// Compare-and-select, not fminf(fmaxf()): both comparisons are false for a NaN, which stays a NaN as under torch.clamp.
// Everything behind it reads the clamped value: both terms of modes 0 / 1, y / c2 of the last step (the final roll lies in
// [lo / c2, hi / c2]), mode 5's d = y + c (y - p) and its history p (d itself is not clamped), an unguided step's c alone;
// two windows clamp the same mean.
DR_DEVINL void clamp_quad(const float lo, const float hi, float (&y)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = y[e] < lo ? lo : (y[e] > hi ? hi : y[e]);
}

// The update's plain form: the clamp where UpdateArgs names one.  What stands in this place in the other forms is the
// overload of form_quad on the form's second kernel argument - ThreshUpd (threshold_quad.h), RescaleUpd (rescale_quad.h),
// ProjectUpd (project_quad.h), MomentumUpd (momentum_quad.h) - which the units that instantiate a form include behind this header.
struct PlainUpd {};
DR_DEVINL void form_quad(const UpdateArgs& a, const PlainUpd&, const long, float (&y)[4]) {
    if (a.clamp_lo < a.clamp_hi) clamp_quad(a.clamp_lo, a.clamp_hi, y);
}

// Option "window_blend" (win_blend() of UpdateArgs::win): what a frame shared by windows b and b + 1 takes of the two guided predictions
// lo (window b's, its frame H + j) and up (window b + 1's, its frame j), j = 0 .. O - 1 the position within the overlap:
//   0  the mean 0.5f * (lo + up)
//   1  the linear cross-fade lo + wu * (up - lo), wu = (float)(j + 1) / (float)(O + 1): subtraction, product and sum each
//      rounded once (contraction off), the IEEE division; lo == up gives that value exactly
//   2  the hand-over: lo for j < (O + 1) / 2, else up - a select; the lower window takes the odd frame
// Both windows call it with the lower window's value first: the frames they share stay bit-identical.  y may be lo or up
// (element e is read before it is written).  Shared by update_quad and pred_quad (threshold_quad.h).
DR_DEVINL void blend_quad(const int mode, const int j, const int O, const float (&lo)[4], const float (&up)[4], float (&y)[4]) {
#pragma clang fp contract(off)
    if (mode == 1) {
        const float wu = (float)(j + 1) / (float)(O + 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = lo[e] + wu * (up[e] - lo[e]);
    } else if (mode == 2) {
        const bool lower = j < (O + 1) / 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = lower ? lo[e] : up[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = 0.5f * (lo[e] + up[e]);
    }
}

// pred (optional): receives the prediction the update consumed - guided, after the shared-frame mean and the clamp of
// option "x0_clip" (mode 5's history).  form: what the step does between the shared-frame blend and the update - form_quad
// of its type; the tail kernel instantiates the plain form, the text it always had.
template <class Form = PlainUpd>
DR_DEVINL float4 update_quad(const UpdateArgs& a, const long i4, float4* pred = nullptr, const Form& form = Form{}) {
#pragma clang fp contract(off)
    float x0[4];
    // per-call scalars: by value (eager launches) or from the device block (captured chain)
    const float gw = a.dyn ? a.dyn->w : a.w, g1pw = a.dyn ? a.dyn->onepw : a.onepw;
    const uint64_t seed = a.dyn ? a.dyn->seed : a.seed;
    const int first_sample = a.dyn ? a.dyn->first_sample : a.first_sample;
    guided_quad(a, i4, gw, g1pw, x0);
    long key_smp = -1, key_q = 0;             // Philox sample / quad key of a window (win_H > 0): canvas coordinates
    if (win_H(a) > 0) {
        const long e0 = i4 * 4;
        const long smp = e0 / a.per_sample;
        const long within = e0 - smp * a.per_sample;
        const int f = (int)(within / 88);
        const long o4 = a.per_sample / 4 - (long)win_H(a) * 22;      // O frames x 22 quads: window b's frame f <-> b + 1's f - H
        long p4 = -1;
        bool upper = false;                                        // the partner is the upper window (b + 1)
        // which neighbours exist, and this window's place on its canvas: one recording (rec 0, window smp of it), or the
        // table's word (option "window_break": b + 1 shares frames with b unless it is the first window of a recording)
        bool has_up = (smp + 1) * a.per_sample < a.n, has_lo = smp > 0;
        long rec = 0, idx = smp;
        if (a.win_tab) {
            const unsigned me = a.win_tab[smp];
            rec = window_rec(me); idx = window_idx(me);
            has_lo = idx > 0;
            has_up = has_up && window_idx(a.win_tab[smp + 1]) > 0;
        }
        if (f >= win_H(a) && has_up) { p4 = i4 + o4; upper = true; }
        else if (f < (int)(o4 / 22) && has_lo) p4 = i4 - o4;
        if (p4 >= 0) {
            float yp[4];
            guided_quad(a, p4, gw, g1pw, yp);
            // (the lower window's value first in both windows: the same operands in the same order, the same bits)
            if (upper) blend_quad(win_blend(a), f - win_H(a), (int)(o4 / 22), x0, yp, x0);
            else blend_quad(win_blend(a), f, (int)(o4 / 22), yp, x0, x0);
        }
        window_key(a, rec, idx, within, first_sample, key_q, key_smp);
    }
    form_quad(a, form, i4, x0);
    if (pred) *pred = make_float4(x0[0], x0[1], x0[2], x0[3]);
    const float c0 = a.coef[0], c1 = a.coef[1], c2 = a.coef[2], c3 = a.coef[3], c4 = a.coef[4];
    float o[4];
    // which updates draw noise at t > 0: x0 DDPM (0), eps ddpm (2), eps ddim2ddpm (4) - and the solver (5) where its row
    // has c4 != 0 (option "solver_noise": a stochastic row has c4 > 0 at every t > 0 - chain_tables.h: solver_table)
    const bool noisy = (a.mode == 0 || a.mode == 2 || a.mode == 4 || (a.mode == 5 && c4 != 0.f)) && a.t > 0;
    float x[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.t > 0 || a.mode >= 2) {
        const float4 xv = reinterpret_cast<const float4*>(a.x)[i4];
        x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
    }
    if (noisy) noise_quad(a, i4, key_smp, key_q, first_sample, seed, z);
    if (a.mode == 5) return solver_quad(a, i4, x0, x, noisy, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float y = x0[e];   // network output: x0 prediction (modes 0/1) or epsilon (modes 2-4)
        if (a.mode <= 1) {
            // ddpm_x0 family :957-967 / ddim_x0 family :864-873 (c4 = sigma = 0, the 0*z term is dropped)
            if (a.t == 0) o[e] = y / c2;
            else {
                const float t1 = c0 * y;
                const float t2 = (c1 * (x[e] - c2 * y)) / c3;
                o[e] = (a.mode == 0) ? (t1 + t2) + c4 * z[e] : (t1 + t2);
            }
        } else if (a.mode == 2) {
            // ddpm :820-829: sqrt_recip_alphas_t * (x - betas_t * eps / sqrt_1m_acp_t) [+ sqrt(post_var_t) * z]
            const float m = c0 * (x[e] - (c1 * y) / c2);
            o[e] = (a.t == 0) ? m : m + c3 * z[e];
        } else {
            // ddim :885-890 / ddim2ddpm :902-909
            const float xe = (x[e] - c3 * y) / c2;
            if (a.t == 0) o[e] = xe;
            else if (a.mode == 3) o[e] = c0 * xe + c1 * y;
            else o[e] = (c0 * xe + c1 * y) + c4 * z[e];
        }
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace dr
