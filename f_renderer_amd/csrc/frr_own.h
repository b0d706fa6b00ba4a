// frr_own.h -- who frees what on the host side of libfrr_hip.so (frr_api.hip only; user shaders never see this file):
// DevBuf<T>, one hipMalloc allocation with its capacity, and Event, one hipEvent_t.  Each is freed by its destructor, so a
// struct that holds them needs no entry in any clean-up list.  Streams are not owned: they are recycled (g_stream_pool).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <utility>

namespace frr {

// One device allocation of cap() elements of T; empty (nullptr, 0) by default, after a move and after a failed reset().
template <typename T> class DevBuf {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { (void)release(); swap(o); } return *this; }
    ~DevBuf() { (void)release(); }
    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    T *get() const { return p_; }
    operator T *() const { return p_; }   // (kernel arguments and views are raw pointers)
    size_t cap() const { return cap_; }   // elements
    // free (hipFree waits for the device): the pointer is cleared first, so that no failure leaves it dangling
    hipError_t release() { T *q = std::exchange(p_, nullptr); cap_ = 0; return q ? hipFree(q) : hipSuccess; }
    // free what it holds, then allocate n elements (n == 0: 16 bytes, a valid pointer nobody reads)
    hipError_t reset(size_t n)
    {
        hipError_t e = release();
        void *q = nullptr;
        if (e == hipSuccess && (e = hipMalloc(&q, n ? n * sizeof(T) : 16)) == hipSuccess) { p_ = (T *)q; cap_ = n; }
        return e;
    }
};

// One event; empty until create(), after a move and after a failed create().
class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event &) = delete; Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept { std::swap(e_, o.e_); }
    Event &operator=(Event &&o) noexcept { if (this != &o) { destroy(); std::swap(e_, o.e_); } return *this; }
    ~Event() { destroy(); }
    operator hipEvent_t() const { return e_; }
    // timing: an event hipEventElapsedTime can read; otherwise one that only orders streams (hipEventDisableTiming)
    hipError_t create(bool timing = false)
    {
        destroy();
        hipEvent_t q = nullptr;
        const hipError_t e = hipEventCreateWithFlags(&q, timing ? hipEventDefault : hipEventDisableTiming);
        if (e == hipSuccess) e_ = q;   // (only then: whatever a failed call left in q is dropped)
        return e;
    }
    void destroy() { if (hipEvent_t q = std::exchange(e_, nullptr)) (void)hipEventDestroy(q); }
};

} // namespace frr
