"""csrc/captured_chain.h without a GPU: the owner of the captured reverse chain compiled against a stub hip/hip_runtime.h
that logs every graph, stream and capture call, counts live graphs, executables and streams and can fail the next begin,
end, instantiate or stream synchronisation.  A small C++ driver is fed commands; after each one it prints the result, the owner's state and what
the stub saw.  The key is an int (0 = no key)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r"""
    #pragma once
    #include <cstddef>
    #include <string>
    enum hipError_t { hipSuccess = 0, hipErrorUnknown = 999 };
    enum hipStreamCaptureMode { hipStreamCaptureModeThreadLocal = 1 };
    constexpr unsigned hipStreamNonBlocking = 1;
    struct ihipStream_t { int id; };
    struct ihipGraph { int id; };
    struct hipGraphExec { int id; };
    struct hipGraphNode;
    typedef ihipStream_t* hipStream_t;
    typedef ihipGraph* hipGraph_t;
    typedef hipGraphExec* hipGraphExec_t;
    typedef hipGraphNode* hipGraphNode_t;
    namespace stub {
    inline int graphs = 0, execs = 0, streams = 0;                  // live
    inline int next_graph = 1, next_exec = 1, next_stream = 1;
    inline int fail_begin = 0, fail_end = 0, fail_inst = 0, fail_sync = 0;      // fail the next such call with that error
    inline std::string log;
    inline void note(const std::string& ev) { log += (log.empty() ? "" : " ") + ev; }
    inline std::string n(int id) { return std::to_string(id); }
    inline int take(int& f) { int v = f; f = 0; return v; }
    }
    inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
        *s = new ihipStream_t{stub::next_stream++};
        ++stub::streams;
        stub::note("stream_create#" + stub::n((*s)->id) + (flags == hipStreamNonBlocking ? ":nonblocking" : ":?"));
        return hipSuccess;
    }
    inline hipError_t hipStreamDestroy(hipStream_t s) {
        stub::note("stream_destroy#" + stub::n(s->id));
        --stub::streams;
        delete s;
        return hipSuccess;
    }
    inline hipError_t hipStreamSynchronize(hipStream_t s) {
        if (int f = stub::take(stub::fail_sync)) { stub::note("sync#" + stub::n(s->id) + ":fail"); return (hipError_t)f; }
        stub::note("sync#" + stub::n(s->id));
        return hipSuccess;
    }
    inline hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode m) {
        if (int f = stub::take(stub::fail_begin)) { stub::note("begin#" + stub::n(s->id) + ":fail"); return (hipError_t)f; }
        stub::note("begin#" + stub::n(s->id) + (m == hipStreamCaptureModeThreadLocal ? ":threadlocal" : ":?"));
        return hipSuccess;
    }
    inline hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* g) {
        if (int f = stub::take(stub::fail_end)) { *g = nullptr; stub::note("end#" + stub::n(s->id) + ":fail"); return (hipError_t)f; }
        *g = new ihipGraph{stub::next_graph++};
        ++stub::graphs;
        stub::note("end#" + stub::n(s->id) + ":graph#" + stub::n((*g)->id));
        return hipSuccess;
    }
    inline hipError_t hipGraphInstantiate(hipGraphExec_t* x, hipGraph_t g, hipGraphNode_t*, char*, size_t) {
        if (int f = stub::take(stub::fail_inst)) { *x = nullptr; stub::note("instantiate#" + stub::n(g->id) + ":fail"); return (hipError_t)f; }
        *x = new hipGraphExec{stub::next_exec++};
        ++stub::execs;
        stub::note("instantiate#" + stub::n(g->id) + ":exec#" + stub::n((*x)->id));
        return hipSuccess;
    }
    inline hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t s) {
        stub::note("launch#" + stub::n(x->id) + ":on#" + stub::n(s->id));
        return hipSuccess;
    }
    inline hipError_t hipGraphExecDestroy(hipGraphExec_t x) {
        stub::note("exec_destroy#" + stub::n(x->id));
        --stub::execs;
        delete x;
        return hipSuccess;
    }
    inline hipError_t hipGraphDestroy(hipGraph_t g) {
        stub::note("graph_destroy#" + stub::n(g->id));
        --stub::graphs;
        delete g;
        return hipSuccess;
    }
    inline hipError_t hipGraphGetNodes(hipGraph_t g, hipGraphNode_t*, size_t* n) {
        stub::note("nodes#" + stub::n(g->id));
        *n = 400 + (size_t)g->id;
        return hipSuccess;
    }
"""

DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include <utility>
    #include "captured_chain.h"
    using Chain = drh::CapturedChain<int>;
    static ihipStream_t user[2] = {{101}, {102}};      // the caller's streams
    static const char* step_name(Chain::Step s) {
        switch (s) {
            case Chain::Step::OK: return "ok";
            case Chain::Step::WAIT: return "wait";
            case Chain::Step::STREAM: return "stream";
            case Chain::Step::BEGIN: return "begin";
            case Chain::Step::RECORD: return "record";
            case Chain::Step::END: return "end";
            default: return "instantiate";
        }
    }
    // captures under `key` with a recorder that returns `ret`; prints step, hip error and recorder's code
    static void capture(Chain& c, int key, int ret) {
        const bool before = c.capturing();
        auto r = c.capture(key, [&](hipStream_t s) {
            stub::note("record#" + stub::n(s->id) + ":capturing=" + stub::n(c.capturing()));
            return ret;
        });
        printf("%s %d %d %d%d '%s'", step_name(r.failed), (int)r.hip, r.rc, (int)before, (int)c.capturing(), r.call);
    }
    int main() {
        Chain a, b;
        char line[128], cmd[32];
        while (fgets(line, sizeof line, stdin)) {
            long n = 0, m = 0;
            if (sscanf(line, "%31s %ld %ld", cmd, &n, &m) < 1) continue;
            stub::log.clear();
            if (!strcmp(cmd, "capture")) capture(a, (int)n, (int)m);
            else if (!strcmp(cmd, "holds")) printf("%d", (int)a.holds((int)n));
            else if (!strcmp(cmd, "fail_begin")) stub::fail_begin = (int)n;
            else if (!strcmp(cmd, "fail_end")) stub::fail_end = (int)n;
            else if (!strcmp(cmd, "fail_inst")) stub::fail_inst = (int)n;
            else if (!strcmp(cmd, "fail_sync")) stub::fail_sync = (int)n;
            else if (!strcmp(cmd, "launch")) printf("%d", (int)a.launch(&user[n]));
            else if (!strcmp(cmd, "wait")) printf("%d", (int)a.wait());
            else if (!strcmp(cmd, "nodes")) printf("%zu", a.nodes());
            else if (!strcmp(cmd, "timed")) printf("%d", (int)(a.capture_seconds() > 0.0));
            else if (!strcmp(cmd, "move")) b = std::move(a);                 // a -> b (move assignment)
            else if (!strcmp(cmd, "back")) a = Chain(std::move(b));          // b -> a (move construction, then assignment)
            else if (!strcmp(cmd, "holds_b")) printf("%d", (int)b.holds((int)n));
            else if (!strcmp(cmd, "scope")) { Chain c; capture(c, (int)n, 0); (void)c.launch(&user[0]); }
            else { printf("unknown command %s\n", cmd); return 1; }
            // result | capturing | live graphs executables streams | stub log
            printf(" | %d | %d %d %d | %s\n", (int)a.capturing(), stub::graphs, stub::execs, stub::streams, stub::log.c_str());
        }
        { Chain gone(std::move(a)); Chain too(std::move(b)); }
        printf("live %d %d %d\n", stub::graphs, stub::execs, stub::streams);
        return 0;
    }
"""

BEGIN = "hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal)"
INST = "hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)"
SYNC = "hipStreamSynchronize(last_stream)"


def build_driver(d, extra=()):
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(STUB)
    src = d / "captured_chain_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "captured_chain_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", str(d), "-I", os.path.join(ROOT, "diffroll_amd", "csrc"),
           str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return build_driver(tmp_path_factory.mktemp("captured_chain"))


def run(driver, steps):
    """steps: (command, "result | capturing | live graphs executables streams | stub log") after each command"""
    r = subprocess.run([driver], input="".join(c + "\n" for c, _ in steps), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(steps) + 1
    for (c, want), got in zip(steps, lines):
        assert [f.strip() for f in got.split("|")] == [f.strip() for f in want.split("|")], (c, got, want)
    assert lines[-1] == "live 0 0 0"          # the destructors returned every graph, executable and stream


CAPTURE_7 = ("capture 7 0", "ok 0 0 00 '' | 0 | 1 1 1 | stream_create#1:nonblocking begin#1:threadlocal record#1:capturing=1 "
                            "end#1:graph#1 instantiate#1:exec#1")


def test_capture_holds_the_key_it_was_given(driver):
    run(driver, [
        ("holds 7",  "0 | 0 | 0 0 0 | "),
        ("holds 0",  "0 | 0 | 0 0 0 | "),              # the empty key is not held either: no executable
        CAPTURE_7,                                     # capturing() false before, true inside record, false after
        ("holds 7",  "1 | 0 | 1 1 1 | "),
        ("holds 8",  "0 | 0 | 1 1 1 | "),
        ("timed",    "1 | 0 | 1 1 1 | "),
        ("nodes",    "401 | 0 | 1 1 1 | nodes#1"),
    ])


def test_recorder_error_ends_the_capture_and_holds_nothing(driver):
    run(driver, [
        ("capture 7 -5", "record 0 -5 00 '' | 0 | 0 0 1 | stream_create#1:nonblocking begin#1:threadlocal record#1:capturing=1 "
                         "end#1:graph#1 graph_destroy#1"),
        ("holds 7",      "0 | 0 | 0 0 1 | "),
        ("nodes",        "0 | 0 | 0 0 1 | "),
        # ... and the recorder's error wins over a failing end of the capture
        ("fail_end 900", " | 0 | 0 0 1 | "),
        ("capture 7 -5", "record 0 -5 00 '' | 0 | 0 0 1 | begin#1:threadlocal record#1:capturing=1 end#1:fail"),
    ])


def test_failed_begin_end_and_instantiate_hold_nothing(driver):
    run(driver, [
        ("fail_begin 901", " | 0 | 0 0 0 | "),
        ("capture 7 0",    f"begin 901 0 00 '{BEGIN}' | 0 | 0 0 1 | stream_create#1:nonblocking begin#1:fail"),      # record never ran
        ("fail_end 900",   " | 0 | 0 0 1 | "),
        ("capture 7 0",    "end 900 0 00 'hipStreamEndCapture' | 0 | 0 0 1 | begin#1:threadlocal record#1:capturing=1 end#1:fail"),
        ("holds 7",        "0 | 0 | 0 0 1 | "),
        ("fail_inst 902",  " | 0 | 0 0 1 | "),
        ("capture 7 0",    f"instantiate 902 0 00 '{INST}' | 0 | 0 0 1 | begin#1:threadlocal record#1:capturing=1 end#1:graph#1 "
                           "instantiate#1:fail graph_destroy#1"),
        ("holds 7",        "0 | 0 | 0 0 1 | "),
        ("wait",           "0 | 0 | 0 0 1 | "),
        ("capture 7 0",    "ok 0 0 00 '' | 0 | 1 1 1 | begin#1:threadlocal record#1:capturing=1 end#1:graph#2 instantiate#2:exec#1"),
        ("holds 7",        "1 | 0 | 1 1 1 | "),
    ])


def test_a_failed_capture_drops_what_was_held(driver):
    run(driver, [
        CAPTURE_7,
        ("fail_inst 902",  " | 0 | 1 1 1 | "),
        ("capture 8 0",    f"instantiate 902 0 00 '{INST}' | 0 | 0 0 1 | exec_destroy#1 graph_destroy#1 begin#1:threadlocal "
                           "record#1:capturing=1 end#1:graph#2 instantiate#2:fail graph_destroy#2"),
        ("holds 7",        "0 | 0 | 0 0 1 | "),
        ("holds 8",        "0 | 0 | 0 0 1 | "),
    ])


def test_recapture_after_drop_reuses_the_stream(driver):
    run(driver, [
        CAPTURE_7,
        # capture drops what it holds first: the old pair is gone before the new one exists; no second stream
        ("capture 8 0",  "ok 0 0 00 '' | 0 | 1 1 1 | exec_destroy#1 graph_destroy#1 begin#1:threadlocal record#1:capturing=1 "
                         "end#1:graph#2 instantiate#2:exec#2"),
        ("holds 8",      "1 | 0 | 1 1 1 | "),
        ("holds 7",      "0 | 0 | 1 1 1 | "),
        ("capture 9 0",  "ok 0 0 00 '' | 0 | 1 1 1 | exec_destroy#2 graph_destroy#2 begin#1:threadlocal record#1:capturing=1 "
                         "end#1:graph#3 instantiate#3:exec#3"),
    ])


def test_wait_synchronises_the_stream_of_the_last_launch(driver):
    run(driver, [
        ("wait",      "0 | 0 | 0 0 0 | "),
        CAPTURE_7,
        ("wait",      "0 | 0 | 1 1 1 | "),                       # never launched: nothing to wait for
        ("launch 0",  "0 | 0 | 1 1 1 | launch#1:on#101"),
        ("wait",      "0 | 0 | 1 1 1 | sync#101"),
        ("launch 1",  "0 | 0 | 1 1 1 | launch#1:on#102"),
        ("wait",      "0 | 0 | 1 1 1 | sync#102"),
        # a capture over a launched chain waits for the stream of its last launch before it destroys it ...
        ("capture 8 0", "ok 0 0 00 '' | 0 | 1 1 1 | sync#102 exec_destroy#1 graph_destroy#1 begin#1:threadlocal "
                        "record#1:capturing=1 end#1:graph#2 instantiate#2:exec#2"),
        ("wait",      "0 | 0 | 1 1 1 | "),                       # ... and the new chain was never launched
        # a capture over a never-launched chain waits for nothing
        ("capture 9 0", "ok 0 0 00 '' | 0 | 1 1 1 | exec_destroy#2 graph_destroy#2 begin#1:threadlocal record#1:capturing=1 "
                        "end#1:graph#3 instantiate#3:exec#3"),
    ])


def test_a_failing_wait_destroys_nothing_and_keeps_the_old_key(driver):
    run(driver, [
        CAPTURE_7,
        ("launch 0",      "0 | 0 | 1 1 1 | launch#1:on#101"),
        ("fail_sync 903", " | 0 | 1 1 1 | "),
        ("capture 8 0",   f"wait 903 0 00 '{SYNC}' | 0 | 1 1 1 | sync#101:fail"),      # no begin, record never ran
        ("holds 7",       "1 | 0 | 1 1 1 | "),
        ("holds 8",       "0 | 0 | 1 1 1 | "),
        ("nodes",         "401 | 0 | 1 1 1 | nodes#1"),
        ("wait",          "0 | 0 | 1 1 1 | sync#101"),           # still launched, still waited for
        ("capture 8 0",   "ok 0 0 00 '' | 0 | 1 1 1 | sync#101 exec_destroy#1 graph_destroy#1 begin#1:threadlocal "
                          "record#1:capturing=1 end#1:graph#2 instantiate#2:exec#2"),
        ("holds 8",       "1 | 0 | 1 1 1 | "),
    ])


def test_drop_on_an_empty_owner_does_nothing(driver):
    # (drop is private: move assignment releases what its target holds, and is the way to an empty owner)
    run(driver, [
        ("move",  " | 0 | 0 0 0 | "),                            # empty onto empty
        CAPTURE_7,
        ("move",  " | 0 | 1 1 1 | "),                            # onto an empty owner: nothing to destroy
        ("move",  " | 0 | 0 0 0 | exec_destroy#1 graph_destroy#1 stream_destroy#1"),      # empty onto the holder
        ("move",  " | 0 | 0 0 0 | "),
    ])


def test_destructor_destroys_executable_graph_stream_in_that_order(driver):
    run(driver, [
        ("scope 7", "ok 0 0 00 '' | 0 | 0 0 0 | stream_create#1:nonblocking begin#1:threadlocal record#1:capturing=1 end#1:graph#1 "
                    "instantiate#1:exec#1 launch#1:on#101 exec_destroy#1 graph_destroy#1 stream_destroy#1"),
    ])


def test_moves_transfer_ownership_without_a_destroy(driver):
    run(driver, [
        CAPTURE_7,
        ("launch 1",   "0 | 0 | 1 1 1 | launch#1:on#102"),
        ("move",       " | 0 | 1 1 1 | "),
        ("holds 7",    "0 | 0 | 1 1 1 | "),
        ("holds_b 7",  "1 | 0 | 1 1 1 | "),
        ("wait",       "0 | 0 | 1 1 1 | "),                      # the source holds nothing: nothing to wait for
        ("back",       " | 0 | 1 1 1 | "),
        ("holds 7",    "1 | 0 | 1 1 1 | "),
        ("holds_b 7",  "0 | 0 | 1 1 1 | "),
        ("wait",       "0 | 0 | 1 1 1 | sync#102"),              # the stream of the last launch moved along
        ("nodes",      "401 | 0 | 1 1 1 | nodes#1"),
        # move assignment onto an owner that holds a chain releases that chain, and its stream, first
        ("move",       " | 0 | 1 1 1 | "),
        ("capture 8 0", "ok 0 0 00 '' | 0 | 2 2 2 | stream_create#2:nonblocking begin#2:threadlocal record#2:capturing=1 "
                        "end#2:graph#2 instantiate#2:exec#2"),
        ("move",       " | 0 | 1 1 1 | exec_destroy#1 graph_destroy#1 stream_destroy#1"),
        ("holds_b 8",  "1 | 0 | 1 1 1 | "),
    ])
