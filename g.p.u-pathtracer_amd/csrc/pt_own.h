// pt_own.h — the owners of device resources: one allocation (DevBuf), the temporaries of one build (DevTemp), an event, a stream.
// The only file of libptmi.so that names the runtime's allocate / free / create / destroy calls (tests/test_own.py); includes
// nothing of the project, so csrc/pt_own_check.cpp exercises it on the host over stubs of those calls.
//
// An owner releases what it holds when it is destroyed, assigned to or reset; it is move-only and a moved-from owner is empty.
// No owner ever waits on a stream: whoever replaces or shrinks a resource that launches may still use waits first, for the streams
// that resource is used on (quiesce, pt_ctx.h, for the scene; the caller's stream for the grow-only buffers).  DESIGN.md §10 f1c.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace ptmi {

// memory the caller of the C ABI owns (pt_malloc, pt_free): no owner on this side
inline hipError_t device_alloc(void** out, size_t bytes) { return hipMalloc(out, bytes); }
inline hipError_t device_free(void* p) { return hipFree(p); }

// One device allocation of count() elements; empty: get() == nullptr, count() == 0.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // releases what it holds, THEN allocates `count` elements (0: stays empty): never two blocks at once.  Empty on failure.
    hipError_t alloc(size_t count) {
        reset();
        if (count == 0) return hipSuccess;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = (T*)p;
        n_ = count;
        return hipSuccess;
    }
    // grow-only: allocates only when `count` exceeds what it holds (the contents are not kept)
    hipError_t reserve(size_t count) { return count > n_ ? alloc(count) : hipSuccess; }
};

// The temporaries of one build, released together.
class DevTemp {
    std::vector<void*> ptrs;

public:
    DevTemp() = default;
    DevTemp(const DevTemp&) = delete;
    DevTemp& operator=(const DevTemp&) = delete;
    ~DevTemp() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t get(T** out, size_t count) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(p);
        *out = (T*)p;
        return e;
    }
};

// An event, made on first use.
class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return e_; }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    // creates the event with `flags` unless it exists already (then the flags it was made with stand)
    hipError_t ensure(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc == hipSuccess) e_ = e;
        return rc;
    }
};

// A stream of the library's own, plain or with a priority.
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            reset();
            s_ = std::exchange(o.s_, nullptr);
        }
        return *this;
    }
    ~Stream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    hipError_t create(unsigned flags) {
        reset();
        hipStream_t s = nullptr;
        const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
        if (rc == hipSuccess) s_ = s;
        return rc;
    }
    hipError_t create(unsigned flags, int priority) {
        reset();
        hipStream_t s = nullptr;
        const hipError_t rc = hipStreamCreateWithPriority(&s, flags, priority);
        if (rc == hipSuccess) s_ = s;
        return rc;
    }
};

}  // namespace ptmi
