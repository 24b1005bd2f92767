// One owning device allocation of the host runtime (host code only: no kernel translation unit includes it).  Move-only; the
// destructor frees.  It converts to T*, so a kernel argument is written as if it were the raw pointer.
#pragma once
#include <hip/hip_runtime.h>

namespace drh {

template <class T>
class DevBuf {
public:
    DevBuf() = default;
    ~DevBuf() { reset(); }
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;

    operator T*() const { return p_; }
    size_t size() const { return n_; }                 // elements asked for by the last ensure
    bool fits(size_t n) const { return p_ && n <= n_; }

    // Grow-only: keeps the block when n elements fit, else frees it BEFORE allocating the new one (peak memory is one
    // block), at least 16 bytes, zero-filled when asked.  On failure the buffer is left empty.
    hipError_t ensure(size_t n, bool zero) {
        if (fits(n)) return hipSuccess;
        reset();
        const size_t bytes = n * sizeof(T) < 16 ? 16 : n * sizeof(T);
        void* q = nullptr;
        hipError_t st = hipMalloc(&q, bytes);
        if (st == hipSuccess && zero) st = hipMemset(q, 0, bytes);
        if (st != hipSuccess) {
            if (q) (void)hipFree(q);
            return st;
        }
        p_ = static_cast<T*>(q);
        n_ = n;
        return hipSuccess;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace drh
