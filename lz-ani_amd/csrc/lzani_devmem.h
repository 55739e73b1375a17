// lzani_devmem.h -- the one owner of device memory (and of pinned host memory) and of events on the host side of the engine.
// Host only: no kernel sees it, and it is not among the sources a run-time compile embeds (lzani_rtc.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace lzani {

// The allocation fault of the tests (lzani_debug_alloc_fault): three process-wide counters, inert unless armed.  Every
// allocation attempt, device or pinned, takes the next attempt number (a relaxed add) and reads `first` (a relaxed load);
// armed -- first > 0 -- the attempts numbered first .. first + count - 1 are refused.  The numbers start again at 1 with
// every alloc_fault_arm.  Threads share the counters: which of two concurrent attempts gets a number is not fixed.
inline std::atomic<uint64_t> g_alloc_seen{0}, g_alloc_first{0}, g_alloc_count{0};

// Whether this attempt is to be refused.
inline bool alloc_refused()
{
    const uint64_t k = g_alloc_seen.fetch_add(1, std::memory_order_relaxed) + 1;
    const uint64_t lo = g_alloc_first.load(std::memory_order_relaxed);
    return lo && k >= lo && k - lo < g_alloc_count.load(std::memory_order_relaxed);
}
// first > 0: the first-th attempt from now is refused, and the count - 1 behind it; first == 0: none is.  Returns the
// attempts counted since the previous call.
inline uint64_t alloc_fault_arm(uint64_t first, uint64_t count)
{
    g_alloc_first.store(0, std::memory_order_relaxed);           // (nothing is refused while the range changes)
    g_alloc_count.store(first ? count : 0, std::memory_order_relaxed);
    const uint64_t before = g_alloc_seen.exchange(0, std::memory_order_relaxed);
    g_alloc_first.store(first, std::memory_order_relaxed);
    return before;
}

// `capacity()` elements of T on the device (PINNED: in page-locked host memory), released by the destructor.  Move-only,
// empty by default.  Sizes are counts of T; a count of 0 allocates one element, so that a live buffer is never null.
template <class T, bool PINNED = false>
class DevMem {
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevMem& operator=(DevMem&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }

    void reset()
    {
        if (p_) { if constexpr (PINNED) (void)hipHostFree(p_); else (void)hipFree(p_); }
        p_ = nullptr; cap_ = 0;
    }
    // A fresh buffer of exactly `count` elements; what it held is released first.  Empty where it cannot be had.
    hipError_t alloc(size_t count)
    {
        reset();
        count = std::max<size_t>(count, 1);
        if (alloc_refused()) return hipErrorOutOfMemory;       // (the runtime is not asked: nothing is exhausted, no sticky error)
        hipError_t e;
        if constexpr (PINNED) e = hipHostMalloc((void**)&p_, count * sizeof(T), hipHostMallocDefault);
        else e = hipMalloc((void**)&p_, count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr; else cap_ = count;
        return e;
    }
    // At least `count` elements: kept if it is large enough already, else released and allocated anew (the contents are
    // not carried over).
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : alloc(count); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
};
template <class T>
using PinMem = DevMem<T, true>;

// A HIP event, destroyed by the destructor.  Move-only, empty by default.
class DevEvent {
    hipEvent_t e_ = nullptr;

public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept { std::swap(e_, o.e_); return *this; }
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { reset(); }

    void reset()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipError_t create(unsigned flags = hipEventDefault)
    {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    operator hipEvent_t() const { return e_; }
};

// The device time of a stretch of a stream's work: begin and end are recorded on the stream (the events are made by the
// first begin and used again by the later ones), elapsed waits for the end and reads the time between them.
struct StreamSpan {
    DevEvent ev[2];
    hipError_t begin(hipStream_t s)
    {
        for (DevEvent& e : ev)
            if (!e) { const hipError_t rc = e.create(); if (rc != hipSuccess) return rc; }
        return hipEventRecord(ev[0], s);
    }
    hipError_t end(hipStream_t s) { return hipEventRecord(ev[1], s); }
    hipError_t elapsed(float& ms)
    {
        const hipError_t rc = hipEventSynchronize(ev[1]);
        return rc != hipSuccess ? rc : hipEventElapsedTime(&ms, ev[0], ev[1]);
    }
};

// For the callers that fall back instead of failing: whether the allocation succeeded; the runtime's sticky error is
// cleared where it did not.
inline bool got(hipError_t e)
{
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace lzani
