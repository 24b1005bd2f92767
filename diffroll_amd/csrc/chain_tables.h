// The tables of a reverse chain: the steps it visits (option "sampling_steps"), the coefficient rows derived for them
// (respaced rows; options "solver_order" / "solver_noise"), the position option "start_step" names, the rule by which a
// dr_step continues the history of solver order 2 or the state of option "cfg_momentum" or "guidance_stride", and the per-window words of options "window_break" / "draws".  Every
// one is a pure function of host values; abi.hip uploads what they return and words the refusals.  Host code; plain C++
// (tests/test_chain_tables_cpu.py compiles it without HIP).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <functional>
#include <vector>

#include "../../include/diffroll_amd.h"      // DR_COEF_FAMILIES
#include "launch_plan.h"                     // STACK_GROUPS

namespace dr {

// The steps a chain of n network evaluations over S diffusion steps visits, in chain order (position 0 = the first step,
// S - 1): t_i = round-half-up(i (S - 1) / (n - 1)), i = n-1 .. 0, in integer arithmetic - strictly decreasing to 0.
// n == 0 or n == S: every step, stored empty.
class ChainSteps {
    int S_ = 0;
    std::vector<int> v_;
public:
    ChainSteps() = default;
    ChainSteps(int S, int n) : S_(S) {
        if (n == 0 || n == S) return;
        v_.resize(n);
        for (int i = n - 1; i >= 0; --i) v_[n - 1 - i] = (int)((2LL * i * (S - 1) + (n - 1)) / (2LL * (n - 1)));
    }
    int S() const { return S_; }
    bool respaced() const { return !v_.empty(); }
    int count() const { return v_.empty() ? S_ : (int)v_.size(); }
    // position -> step; -1 past either end
    int at(int i) const {
        if (i < 0 || i >= count()) return -1;
        return v_.empty() ? S_ - 1 - i : v_[i];
    }
    // step -> position; -1: not visited
    int position(int t) const {
        if (t < 0 || t >= S_) return -1;
        if (v_.empty()) return S_ - 1 - t;
        const auto it = std::lower_bound(v_.begin(), v_.end(), t, std::greater<int>());
        return it != v_.end() && *it == t ? (int)(it - v_.begin()) : -1;
    }
    // the step visited after t; -1: t is the last one (0) or not visited
    int successor(int t) const {
        const int i = position(t);
        return i < 0 ? -1 : at(i + 1);
    }
};

// option "sampling_steps" (include/diffroll_amd.h): the (DR_COEF_FAMILIES, S, 5) table a respaced chain reads.  A visited t
// whose successor t' is t - 1 (or t == 0) keeps the committed row, and so does every unvisited step (never read); every
// other one gets a row derived in double precision from the committed fp32 sqrt_acp / sqrt_1m_acp of t and t' (family 0,
// columns 2 and 3) and rounded to fp32 once, in the column order update_quad.h reads.
inline std::vector<float> respaced_table(const std::vector<float>& h_coef, const ChainSteps& steps) {
    const int S = steps.S(), n = steps.count();
    std::vector<float> tab(h_coef);
    const float* h = h_coef.data();           // family 0 row t: [.., .., sqrt_acp[t], sqrt_1m_acp[t], ..]
    for (int i = 0; i + 1 < n; ++i) {
        const int t = steps.at(i), tp = steps.at(i + 1);
        if (tp == t - 1) continue;
        const double A = h[(size_t)t * 5 + 2], Sm = h[(size_t)t * 5 + 3], Ap = h[(size_t)tp * 5 + 2], Smp = h[(size_t)tp * 5 + 3];
        const double r2 = (A / Ap) * (A / Ap);                       // alpha of the stride: acp[t] / acp[t']
        const double sigma = (Smp / Sm) * std::sqrt(1.0 - r2);
        const double dir = std::sqrt(std::max(0.0, 1.0 - Ap * Ap - sigma * sigma));   // (>= 0 exactly; clamps rounding)
        const double beta = 1.0 - r2;
        const double rows[DR_COEF_FAMILIES][5] = {
            {Ap, dir, A, Sm, sigma},                                  // ddpm_x0 family
            {Ap, std::sqrt(1.0 - Ap * Ap), A, Sm, 0.0},               // ddim_x0 family
            {Ap / A, beta, Sm, std::sqrt(beta * Smp * Smp / (Sm * Sm)), 0.0},   // ddpm (epsilon)
            {Ap, Smp, A, Sm, 0.0},                                    // ddim (epsilon)
            {Ap, dir, A, Sm, sigma}};                                 // ddim2ddpm (epsilon)
        for (int f = 0; f < DR_COEF_FAMILIES; ++f)
            for (int c = 0; c < 5; ++c) tab[((size_t)f * S + t) * 5 + c] = (float)rows[f][c];
    }
    return tab;
}

// option "solver_order" (include/diffroll_amd.h): the (2 S, 5) rows solver_quad reads (update_quad.h), for the steps the chain
// visits; unvisited rows are zero, and so is the whole table for order 0.  With lambda_t = log(sqrt_acp[t] / sqrt_1m_acp[t]),
// t' the successor of t and t'' its predecessor in the chain, h = lambda_t' - lambda_t and h_prev = lambda_t - lambda_t'':
//   t > 0:  [sqrt_1m_acp[t'] / sqrt_1m_acp[t], -sqrt_acp[t'] expm1(-h), sqrt_acp[t], c, 0]
//           c = h / (2 h_prev) for order 2 when t is not the chain's first step and t' != 0, else 0: the step into 0 is
//           first order (lambda jumps between steps 1 and 0 of the linear schedule; extrapolating across it hurts short chains)
//   t == 0: [0, 0, sqrt_acp[0], 0, 0]
// option "solver_noise" (the stochastic form, SDE-DPM-Solver++), same c:
//   t > 0:  [(sqrt_1m_acp[t'] / sqrt_1m_acp[t]) exp(-h), -sqrt_acp[t'] expm1(-2h), sqrt_acp[t], c, sqrt_1m_acp[t'] sqrt(-expm1(-2h))]
// With sqrt_acp^2 + sqrt_1m_acp^2 = 1 column 4 is the sigma of the derived DR_COEF_DDPM_X0 row of respaced_table and column
// 0 its sqrt(1 - acp' - sigma^2) / sqrt_1m_acp: first order is the ddpm_x0 update by another arithmetic route.
// Derived in double from the committed fp32 scalars (family 0, columns 2 and 3), rounded to fp32 once.
// Rows [S, 2 S) repeat rows [0, S) with c = 0: step t as a chain's FIRST step (option "start_step": a started chain has no
// previous prediction).  run_step picks row S + t for the step the option names - no row is rewritten when the option
// changes, so a chain captured under another start reads at replay what it read when it was captured.
inline std::vector<float> solver_table(const std::vector<float>& h_coef, const ChainSteps& steps, int order, int noise) {
    const int S = steps.S(), n = steps.count();
    std::vector<float> tab((size_t)2 * S * 5, 0.f);
    if (order == 0) return tab;
    const float* h = h_coef.data();
    auto lambda = [&](int t) { return std::log((double)h[(size_t)t * 5 + 2] / (double)h[(size_t)t * 5 + 3]); };
    for (int i = 0; i < n; ++i) {
        const int t = steps.at(i);
        float* row = tab.data() + (size_t)t * 5;
        row[2] = h[(size_t)t * 5 + 2];
        if (t == 0) continue;
        const int tp = steps.at(i + 1);
        const double Sm = h[(size_t)t * 5 + 3], Ap = h[(size_t)tp * 5 + 2], Smp = h[(size_t)tp * 5 + 3];
        const double hh = lambda(tp) - lambda(t);
        if (noise) {
            const double g = -std::expm1(-2.0 * hh);      // 1 - exp(-2h) > 0: lambda increases along the chain
            row[0] = (float)((Smp / Sm) * std::exp(-hh));
            row[1] = (float)(Ap * g);
            row[4] = (float)(Smp * std::sqrt(g));
        } else {
            row[0] = (float)(Smp / Sm);
            row[1] = (float)(-Ap * std::expm1(-hh));
        }
        if (order == 2 && i > 0 && tp != 0) row[3] = (float)(hh / (2.0 * (lambda(t) - lambda(steps.at(i - 1)))));
    }
    for (int t = 0; t < S; ++t) {
        const float* row = tab.data() + (size_t)t * 5;
        float* first = tab.data() + ((size_t)S + t) * 5;
        std::copy(row, row + 5, first);
        first[3] = 0.f;
    }
    return tab;
}

// option "start_step": the chain position of the step a chain begins at - 0 when the option is off (-1).  pos < 0: the chain
// does not visit the step; `above` > start_step > `below` are the visited steps on either side of it (the steps decrease
// strictly and end at 0, so below exists for every start_step >= 0, and above for every one below S)
struct StartPosition { int pos, above, below; };
inline StartPosition start_position(const ChainSteps& steps, int start_step) {
    if (start_step < 0) return {0, -1, -1};
    const int pos = steps.position(start_step);
    if (pos >= 0) return {pos, -1, -1};
    int i = 0;
    while (steps.at(i) > start_step) ++i;
    return {-1, steps.at(i - 1), steps.at(i)};
}

// dr_step under solver order 2: what the engine's history holds - the prediction of step t of a (sampler, B, T) chain
struct HistoryKey { bool valid = false; int sampler = -1, B = 0, T = 0, t = -1; };
// The history is engine state: the chain's first step starts one, and so does the step option "start_step" names (its row
// has c = 0); every other step continues the one the previous dr_step left - it must be the successor of that step, in a
// chain of the same (sampler, B, T) - or is refused, with the step expected next (the chain's first where nothing continues)
enum class HistoryStep { STARTS, CONTINUES, REFUSED };
struct HistoryVerdict { HistoryStep what; int expect; };
inline HistoryVerdict history_step(const HistoryKey& k, int sampler, int B, int T, int t, const ChainSteps& steps, int start_step) {
    const int first = steps.at(0);
    if (t == first || t == start_step) return {HistoryStep::STARTS, t};
    const bool same = k.valid && k.sampler == sampler && k.B == B && k.T == T;
    const int next = same ? steps.successor(k.t) : -1;
    const int expect = next >= 0 ? next : first;
    return {same && expect == t ? HistoryStep::CONTINUES : HistoryStep::REFUSED, expect};
}

// dr_step under option "cfg_momentum": what the engine's momentum state holds - m of the guided step t of a (sampler, B, T) chain
struct MomentumKey { bool valid = false; int sampler = -1, B = 0, T = 0, t = -1; };
// The first step at or below `from` (from < 0: from the chain's first step) that the chain visits and that guides; -1: none.
// Guiding is launch_plan.h's step_guided: w != 0, inside the guidance interval (the caller has a sampler that guides).
inline int guided_from(const ChainSteps& steps, int from, const GuidanceInterval& g, int S, bool w_zero) {
    for (int i = 0, n = steps.count(); i < n; ++i) {
        const int t = steps.at(i);
        if ((from < 0 || t <= from) && step_guided(g, S, w_zero, t)) return t;
    }
    return -1;
}
// The state is engine state with the history's discipline, over the steps that guide alone (a step that does not guide
// neither reads nor writes it, and is never asked about here): the first guided step of a chain from its start position
// (option "start_step") starts it; every other guided step continues the one the previous guided dr_step left - it must be
// the guided visited step behind that one, in a chain of the same (sampler, B, T) - or is refused, with the step expected
// next (the first guided step where nothing continues).
enum class MomentumStep { STARTS, CONTINUES, REFUSED };
struct MomentumVerdict { MomentumStep what; int expect; };
inline MomentumVerdict momentum_step(const MomentumKey& k, int sampler, int B, int T, int t, const ChainSteps& steps, int start_step,
                                     const GuidanceInterval& g, int S, bool w_zero) {
    const int first = guided_from(steps, start_step, g, S, w_zero);
    if (t == first) return {MomentumStep::STARTS, t};
    const bool same = k.valid && k.sampler == sampler && k.B == B && k.T == T;
    const int next = same && k.t > 0 ? guided_from(steps, k.t - 1, g, S, w_zero) : -1;
    const int expect = next >= 0 ? next : first;
    return {same && expect == t ? MomentumStep::CONTINUES : MomentumStep::REFUSED, expect};
}

// dr_step under option "guidance_stride": what the engine's stride state holds - d of the last refresh, as the guided step t
// of a (sampler, B, T) chain left it (t: the last guided step run, a refresh or a reuse)
struct StrideKey { bool valid = false; int sampler = -1, B = 0, T = 0, t = -1; };
// The ordinal k of step t among the steps at or below `from` (from < 0: from the chain's first step) that the chain visits
// and that guide, in chain order - guided_from's counting; -1: t is not one of them.
inline int guided_ordinal(const ChainSteps& steps, int from, const GuidanceInterval& g, int S, bool w_zero, int t) {
    for (int i = 0, k = 0, n = steps.count(); i < n; ++i) {
        const int v = steps.at(i);
        if ((from >= 0 && v > from) || !step_guided(g, S, w_zero, v)) continue;
        if (v == t) return k;
        ++k;
    }
    return -1;
}
// The state has the discipline of the momentum's, over the steps that guide alone: a step that refreshes (launch_plan.h:
// stride_refreshes of its ordinal - the chain's first guided step, every n-th one behind it, step 0) needs nothing and
// overwrites the state; a step that reuses must be the guided visited step behind the guided step the previous guided
// dr_step ran, in a chain of the same (sampler, B, T) - or is refused, with the step expected next (the first guided step
// where nothing continues, and for a step that is no guided step of this chain).  k: the step's ordinal.
enum class StrideStep { REFRESHES, REUSES, REFUSED };
struct StrideVerdict { StrideStep what; int expect; int k; };
inline StrideVerdict stride_step(const StrideKey& key, int sampler, int B, int T, int t, const ChainSteps& steps, int start_step,
                                 const GuidanceInterval& g, int S, bool w_zero, int n) {
    const int first = guided_from(steps, start_step, g, S, w_zero);
    const int k = guided_ordinal(steps, start_step, g, S, w_zero, t);
    if (k < 0) return {StrideStep::REFUSED, first, k};
    if (stride_refreshes(n, k, t)) return {StrideStep::REFRESHES, t, k};
    const bool same = key.valid && key.sampler == sampler && key.B == B && key.T == T;
    const int next = same && key.t > 0 ? guided_from(steps, key.t - 1, g, S, w_zero) : -1;
    const int expect = next >= 0 ? next : first;
    return {same && expect == t ? StrideStep::REUSES : StrideStep::REFUSED, expect, k};
}

// one word per window: Philox key offset of its recording (the ordinal in the batch; + draw x stride under option "draws":
// < 65536) and index within the recording (< STACK_GROUPS)
constexpr unsigned window_entry(unsigned rec, unsigned idx) { return (rec << 16) | idx; }
constexpr int window_rec(unsigned w) { return (int)(w >> 16); }
constexpr int window_idx(unsigned w) { return (int)(w & 0xFFFFu); }
// The table travels to the device BY VALUE in the kernel arguments of a one-block launch (2 KiB: no host buffer has to
// outlive the call), stream-ordered like launch_set_dyn.
struct WindowTable { unsigned w[STACK_GROUPS]; };
// The table of a batch of B <= STACK_GROUPS windows: `draws` draws of B / draws windows each, `marks` (ascending) the windows
// of one draw that start a new recording - window 0 always does, and every draw starts new recordings.  Draw d of recording r
// is keyed first_sample + r + d * stride: draw_stride, or 0 = the recordings of one draw.  Without marks: window b of
// recording 0.
inline WindowTable window_table(const std::vector<int>& marks, int B, int draws, int draw_stride) {
    WindowTable tab{};
    const int n = B / draws;
    const size_t stride = draw_stride > 0 ? (size_t)draw_stride : marks.size() + 1;
    size_t m = 0;
    for (int b = 0, first = 0; b < B && b < STACK_GROUPS; ++b) {
        const int j = b % n;
        if (j == 0) { m = 0; first = b; }
        if (m < marks.size() && marks[m] == j) { ++m; first = b; }
        tab.w[b] = window_entry((unsigned)((size_t)(b / n) * stride + m), (unsigned)(b - first));
    }
    return tab;
}

}  // namespace dr
