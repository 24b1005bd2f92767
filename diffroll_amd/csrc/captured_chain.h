// The owner of one captured launch sequence of the host runtime - the reverse chain of dr_sample as a hipGraph (host code
// only, nothing of the engine: it compiles against a stub hip/hip_runtime.h, tests/test_captured_chain_cpu.py).  It holds the
// graph, its executable, the key the sequence was captured under, the non-blocking stream captures happen on (created
// on first use: the caller's stream may be the null stream), the stream of the last launch and the seconds the last
// capture + instantiation took.  Move-only; the destructor destroys the executable, then the graph, then the stream.
// An executable is destroyed only by the capture that replaces it, which waits for its last launch first, and by the
// destructor and move-assignment, whose callers have waited.  Every graph and capture call of the runtime is in this file.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <utility>

namespace drh {

template <class Key>
class CapturedChain {
public:
    // What capture() reports: the step that failed and what it failed with - `hip` and `call` (the HIP call as written
    // below) for a step of this file, `rc` for RECORD (the error is the recorder's own, wherever it left its text)
    enum class Step { OK, WAIT, STREAM, BEGIN, RECORD, END, INSTANTIATE };
    struct Captured {
        Step failed = Step::OK;
        hipError_t hip = hipSuccess;
        int rc = 0;
        const char* call = "";
        explicit operator bool() const { return failed == Step::OK; }
    };

    CapturedChain() = default;
    ~CapturedChain() { release(); }
    CapturedChain(CapturedChain&& o) noexcept { steal(o); }
    CapturedChain& operator=(CapturedChain&& o) noexcept {
        if (this != &o) { release(); steal(o); }
        return *this;
    }
    CapturedChain(const CapturedChain&) = delete;
    CapturedChain& operator=(const CapturedChain&) = delete;

    // an executable exists and was captured under an equal key
    bool holds(const Key& key) const { return exec_ && key_ == key; }
    // true exactly while capture() runs its recorder: what is launched now is a node of the graph, not work
    bool capturing() const { return capturing_; }

    // Captures what record(stream) launches on the capture stream (thread-local mode: other host threads keep launching) and
    // instantiates it under `key`.  What was held before is waited for, then destroyed, first: a failing wait (WAIT) touches
    // nothing, what was held still is.  The capture is ended whatever record returned; a failure of any later step leaves
    // nothing held.
    template <class Record>
    Captured capture(const Key& key, Record&& record) {
        Captured c;
        auto failed = [&](Step s, hipError_t st, const char* call) { c.failed = s; c.hip = st; c.call = call; return c; };
        hipError_t st;
        if ((st = wait()) != hipSuccess) return failed(Step::WAIT, st, "hipStreamSynchronize(last_stream)");
        drop();
        if (!cap_stream_ && (st = hipStreamCreateWithFlags(&cap_stream_, hipStreamNonBlocking)) != hipSuccess) {
            cap_stream_ = nullptr;
            return failed(Step::STREAM, st, "hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking)");
        }
        const auto t0 = std::chrono::steady_clock::now();
        if ((st = hipStreamBeginCapture(cap_stream_, hipStreamCaptureModeThreadLocal)) != hipSuccess)
            return failed(Step::BEGIN, st, "hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal)");
        capturing_ = true;
        c.rc = record(cap_stream_);
        capturing_ = false;
        st = hipStreamEndCapture(cap_stream_, &graph_);
        if (c.rc != 0) {
            c.failed = Step::RECORD;
        } else if (st != hipSuccess) {
            failed(Step::END, st, "hipStreamEndCapture");
        } else if ((st = hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0)) != hipSuccess) {
            exec_ = nullptr;
            failed(Step::INSTANTIATE, st, "hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)");
        }
        if (!c) { drop(); return c; }
        key_ = key;
        capture_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return c;
    }

    hipError_t launch(hipStream_t stream) {
        hipError_t st = hipGraphLaunch(exec_, stream);
        if (st == hipSuccess) { last_stream_ = stream; launched_ = true; }
        return st;
    }
    // the held chain may still be running, on the stream it was last launched on: wait for it (never launched: nothing to
    // wait for).  What capture() does before it destroys, and what a caller does before it frees a buffer the chain reads.
    hipError_t wait() const { return exec_ && launched_ ? hipStreamSynchronize(last_stream_) : hipSuccess; }

    double capture_seconds() const { return capture_s_; }      // of the last successful capture + instantiation
    size_t nodes() const {                                     // of the held graph (0: none)
        size_t n = 0;
        if (graph_ && hipGraphGetNodes(graph_, nullptr, &n) != hipSuccess) n = 0;
        return n;
    }

private:
    // Destroys executable and graph and resets the key; waits for nothing (see the top); nothing to do on an empty owner
    void drop() {
        if (exec_) { (void)hipGraphExecDestroy(exec_); exec_ = nullptr; }
        if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }
        key_ = Key{};
        launched_ = false;
    }
    void release() {
        drop();
        if (cap_stream_) { (void)hipStreamDestroy(cap_stream_); cap_stream_ = nullptr; }
    }
    void steal(CapturedChain& o) {
        graph_ = std::exchange(o.graph_, nullptr);
        exec_ = std::exchange(o.exec_, nullptr);
        cap_stream_ = std::exchange(o.cap_stream_, nullptr);
        key_ = std::exchange(o.key_, Key{});
        last_stream_ = o.last_stream_;
        launched_ = std::exchange(o.launched_, false);
        capture_s_ = o.capture_s_;
    }

    hipGraph_t graph_ = nullptr;
    hipGraphExec_t exec_ = nullptr;
    hipStream_t cap_stream_ = nullptr;
    Key key_{};
    hipStream_t last_stream_ = nullptr;
    bool launched_ = false;
    bool capturing_ = false;
    double capture_s_ = 0.0;
};

}  // namespace drh
