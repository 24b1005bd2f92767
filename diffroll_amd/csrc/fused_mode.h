// Whether an engine's residual layers run as persistent launches (stack_kernel, tail_kernel) or one launch per phase: the
// caller's option "fused_stack" and what has happened to it since.  Four events move it -
//   set_option   the caller sets "fused_stack": its word replaces any pending yield or heal
//   look         abi.hip asks tenants.h whether another PROCESS is computing on the device (1 yes, 0 no, -1 not looked):
//                a yes yields (per-phase launches, no co-residency assumption); two noes in a row re-arm
//   timeout      dr_finish found a group barrier that gave up: per-phase launches until option "fused_rearm" clean
//                checked chains (0: never) - a time-out outranks a pending yield, looks no longer re-arm
//   clean_chain  dr_sample_checked finished a chain without a time-out
// Every transition returns whether active() changed: the caller then marks its captured chain, which bakes the launch
// mode, stale.  Host code; plain C++ (tests/test_fused_mode_cpu.py compiles it without HIP).
#pragma once
#include <cstdint>

namespace drh {

struct FusedMode {
    int option = 1;                // the caller's "fused_stack": 0 one launch per phase, 1 fused where the planner likes it, 2 fused regardless
    int rearm_after = 0;           // the caller's "fused_rearm"
    enum State { ON, YIELDED, TIMED_OUT } state = ON;
    int clean = 0;                 // YIELDED: looks in a row that found the GPU exclusive; TIMED_OUT: clean checked chains since
    int64_t yields = 0;            // times fusing was given up because another process was computing (no time-out)
    int64_t fallbacks = 0;         // time-outs dr_finish detected
    int64_t rearms = 0;            // times fused launches were switched back on (after a yield or a time-out)

    // what every launch decision reads
    int active() const { return state == ON ? option : 0; }
    // this call may issue fused launches (a yielded engine may re-arm inside dr_sample): looks are taken, x_T is kept
    bool may_fuse() const { return option != 0 && state != TIMED_OUT; }

    bool set_option(int v) {
        const int was = active();
        option = v;
        to(ON);
        return was != v;
    }
    bool yield() {
        if (!active()) return false;
        to(YIELDED);
        yields += 1;
        return true;
    }
    bool look(int shared) {
        if (state == ON) return shared == 1 && yield();
        if (state != YIELDED || shared < 0) return false;
        if (shared == 1) { clean = 0; return false; }
        if (++clean < 2) return false;
        return rearm();
    }
    bool timeout() {
        const int was = active();
        fallbacks += 1;
        if (option) to(TIMED_OUT);
        return was != 0;
    }
    bool clean_chain() {
        if (state != TIMED_OUT || rearm_after <= 0 || ++clean < rearm_after) return false;
        return rearm();
    }

private:
    void to(State s) { state = s; clean = 0; }
    bool rearm() {
        to(ON);
        rearms += 1;
        return true;
    }
};

}  // namespace drh
