"""csrc/fused_mode.h without a GPU: the launch-mode state machine of an engine (option fused_stack, yields after a look
at the device, time-outs found by dr_finish, re-arms) compiled into a small C++ driver, fed events, state checked after
every one of them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include "fused_mode.h"
    int main() {
        drh::FusedMode m;
        const char* names[] = {"ON", "YIELDED", "TIMED_OUT"};
        char line[128], ev[32];
        while (fgets(line, sizeof line, stdin)) {
            int arg = 0;
            if (sscanf(line, "%31s %d", ev, &arg) < 1) continue;
            bool changed = false;
            if (!strcmp(ev, "set")) changed = m.set_option(arg);
            else if (!strcmp(ev, "yield")) changed = m.yield();
            else if (!strcmp(ev, "look")) changed = m.look(arg);
            else if (!strcmp(ev, "timeout")) changed = m.timeout();
            else if (!strcmp(ev, "clean")) changed = m.clean_chain();
            else if (!strcmp(ev, "rearm_after")) m.rearm_after = arg;
            else { printf("unknown event %s\n", ev); return 1; }
            printf("%d %s %d %lld %lld %lld %d %d\n", m.active(), names[m.state], m.clean, (long long)m.yields,
                   (long long)m.fallbacks, (long long)m.rearms, (int)m.may_fuse(), (int)changed);
        }
        return 0;
    }
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("fused_mode")
    src = d / "fused_mode_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "fused_mode_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def run(driver, steps):
    """steps: (event, "active state clean yields fallbacks rearms may_fuse") after each event, from a new engine's state"""
    r = subprocess.run([driver], input="".join(ev + "\n" for ev, _ in steps), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(steps)
    active = 1                                      # a new engine fuses (fused_stack = 1)
    for (ev, want), got in zip(steps, lines):
        *state, changed = got.split()
        assert " ".join(state) == want, (ev, got, want)
        # every transition reports whether active() changed: the caller drops its captured chain exactly then
        assert int(changed) == (int(state[0]) != active), (ev, got)
        active = int(state[0])


def test_yield_and_rearm_by_looks(driver):
    run(driver, [
        ("look -1", "1 ON 0 0 0 0 1"),              # not looked (rate limit / undecided): nothing changes
        ("look 0",  "1 ON 0 0 0 0 1"),
        ("set 2",   "2 ON 0 0 0 0 1"),
        ("look 1",  "0 YIELDED 0 1 0 0 1"),         # another process is computing: yield
        ("look 0",  "0 YIELDED 1 1 0 0 1"),
        ("look 1",  "0 YIELDED 0 1 0 0 1"),         # a busy look starts the count again
        ("look 0",  "0 YIELDED 1 1 0 0 1"),
        ("look 0",  "2 ON 0 1 0 1 1"),              # two clean looks in a row: the caller's option comes back
        ("yield",   "0 YIELDED 0 2 0 1 1"),         # the yield itself (creation / after a capture go through look 1 too)
        ("yield",   "0 YIELDED 0 2 0 1 1"),         # (only an engine that fuses can yield)
        ("look 0",  "0 YIELDED 1 2 0 1 1"),
        ("look 0",  "2 ON 0 2 0 2 1"),
    ])


def test_a_not_looked_look_does_not_break_the_run_a_busy_one_does(driver):
    run(driver, [
        ("look 1",  "0 YIELDED 0 1 0 0 1"),
        ("look 0",  "0 YIELDED 1 1 0 0 1"),
        ("look -1", "0 YIELDED 1 1 0 0 1"),
        ("look 0",  "1 ON 0 1 0 1 1"),              # 0, -1, 0 re-arms
        ("look 1",  "0 YIELDED 0 2 0 1 1"),
        ("look 0",  "0 YIELDED 1 2 0 1 1"),
        ("look 1",  "0 YIELDED 0 2 0 1 1"),
        ("look 0",  "0 YIELDED 1 2 0 1 1"),         # 0, 1, 0 does not
    ])


def test_a_yielded_engine_may_fuse(driver):
    """dr_sample_checked keeps x_T whenever may_fuse(): a yielded engine can re-arm inside the dr_sample it calls and
    then issue fused launches, which can time out."""
    run(driver, [
        ("look 1",  "0 YIELDED 0 1 0 0 1"),
        ("look 0",  "0 YIELDED 1 1 0 0 1"),
        ("look 0",  "1 ON 0 1 0 1 1"),
    ])


def test_timeout_waits_for_fused_rearm(driver):
    run(driver, [
        ("timeout",       "0 TIMED_OUT 0 0 1 0 0"),
        ("look 0",        "0 TIMED_OUT 0 0 1 0 0"),  # looks do not re-arm after a time-out
        ("look 0",        "0 TIMED_OUT 0 0 1 0 0"),
        ("look 1",        "0 TIMED_OUT 0 0 1 0 0"),
        ("clean",         "0 TIMED_OUT 0 0 1 0 0"),  # fused_rearm = 0: never
        ("rearm_after 2", "0 TIMED_OUT 0 0 1 0 0"),
        ("clean",         "0 TIMED_OUT 1 0 1 0 0"),
        ("timeout",       "0 TIMED_OUT 0 0 2 0 0"),  # a second time-out starts the count again
        ("clean",         "0 TIMED_OUT 1 0 2 0 0"),
        ("clean",         "1 ON 0 0 2 1 1"),         # fused_rearm clean checked chains: the caller's option comes back
        ("clean",         "1 ON 0 0 2 1 1"),
        ("rearm_after 0", "1 ON 0 0 2 1 1"),
        ("timeout",       "0 TIMED_OUT 0 0 3 1 0"),
        ("clean",         "0 TIMED_OUT 0 0 3 1 0"),
    ])


def test_timeout_while_yielded_outranks_the_yield(driver):
    run(driver, [
        ("rearm_after 3", "1 ON 0 0 0 0 1"),
        ("set 2",         "2 ON 0 0 0 0 1"),
        ("look 1",        "0 YIELDED 0 1 0 0 1"),
        ("look 0",        "0 YIELDED 1 1 0 0 1"),
        ("timeout",       "0 TIMED_OUT 0 1 1 0 0"),
        ("look 0",        "0 TIMED_OUT 0 1 1 0 0"),  # two clean looks no longer re-arm ...
        ("look 0",        "0 TIMED_OUT 0 1 1 0 0"),
        ("clean",         "0 TIMED_OUT 1 1 1 0 0"),  # ... fused_rearm clean chains do
        ("clean",         "0 TIMED_OUT 2 1 1 0 0"),
        ("clean",         "2 ON 0 1 1 1 1"),
    ])


def test_set_option_forgets_a_pending_yield_or_heal(driver):
    run(driver, [
        ("set 1",         "1 ON 0 0 0 0 1"),         # same value: nothing to drop
        ("look 1",        "0 YIELDED 0 1 0 0 1"),
        ("look 0",        "0 YIELDED 1 1 0 0 1"),
        ("set 1",         "1 ON 0 1 0 0 1"),         # the caller's word: fused again, no re-arm counted
        ("rearm_after 1", "1 ON 0 1 0 0 1"),
        ("timeout",       "0 TIMED_OUT 0 1 1 0 0"),
        ("set 2",         "2 ON 0 1 1 0 1"),
        ("timeout",       "0 TIMED_OUT 0 1 2 0 0"),
        ("set 0",         "0 ON 0 1 2 0 0"),         # per phase by the caller's word: no heal pending
        ("clean",         "0 ON 0 1 2 0 0"),
        ("look 1",        "0 ON 0 1 2 0 0"),
        ("set 1",         "1 ON 0 1 2 0 1"),
    ])


def test_option_zero_never_yields_or_rearms(driver):
    run(driver, [
        ("set 0",         "0 ON 0 0 0 0 0"),
        ("look 1",        "0 ON 0 0 0 0 0"),
        ("yield",         "0 ON 0 0 0 0 0"),
        ("rearm_after 1", "0 ON 0 0 0 0 0"),
        ("timeout",       "0 ON 0 0 1 0 0"),         # counted, but there is nothing to heal back to
        ("clean",         "0 ON 0 0 1 0 0"),
        ("clean",         "0 ON 0 0 1 0 0"),
        ("look 0",        "0 ON 0 0 1 0 0"),
        ("look 0",        "0 ON 0 0 1 0 0"),
    ])
