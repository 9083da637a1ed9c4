// hip_owning.h -- what the host side of the three translation units (ldso_ba.hip, ldso_ct.hip,
// ldso_lc.hip) builds its contexts from: fail / HIP_TRY, the owning device and pinned buffers, the
// owning event, StreamBorrow (the one place where two contexts' streams are ordered with each other),
// and the kernel timer.  Every member of a context frees what it owns when the context is deleted.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ldso_ba_internal.h"

namespace {

inline int fail(int code, const std::string &msg) { return ldso_ba::set_error(code, msg); }

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(-2, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// DevBuf's default OnRealloc: nobody is told when the buffer's address changes
struct NoReallocHook {
    static void changed() {}
};

// A device buffer of n elements.  OnRealloc::changed() runs whenever the address may change (alloc,
// release): ba_context.h's GraphBuf uses it to invalidate captured graphs.
template <typename T, typename OnRealloc = NoReallocHook>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {  // a context's buffers go with it
        if (p) release();
    }
    int alloc(size_t count) {
        OnRealloc::changed();
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (count == 0) return 0;
        hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(-3, std::string("hipMalloc failed: ") + hipGetErrorString(e));
        }
        n = count;  // only a successful allocation counts as capacity
        return 0;
    }
    int ensure(size_t count) { return n >= count && p ? 0 : alloc(count); }  // keeps the pointer if it fits
    void release() {
        OnRealloc::changed();
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    size_t bytes() const { return n * sizeof(T); }
};

// Grow-only pinned host staging of n elements (the address is kept while it fits), freed with the
// context.  With hipHostMallocMapped in kFlags the device reads or writes it directly through dev.
template <typename T, unsigned kFlags = hipHostMallocDefault>
struct PinBuf {
    T *p = nullptr, *dev = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    // the caller has made sure that nothing still uses the old buffer
    int ensure(size_t count, size_t min_bytes = 64) {
        if (p && n >= count) return 0;
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        n = 0;
        const size_t bytes = std::max(count * sizeof(T), min_bytes);
        T *q = nullptr;
        HIP_TRY(hipHostMalloc((void **)&q, bytes, kFlags));
        if (kFlags & hipHostMallocMapped) {
            void *d = nullptr;
            const hipError_t e = hipHostGetDevicePointer(&d, q, 0);
            if (e != hipSuccess) {
                (void)hipHostFree(q);
                return fail(-2, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
            }
            dev = static_cast<T *>(d);
        }
        p = q;
        n = bytes / sizeof(T);  // only a successful allocation counts as capacity
        return 0;
    }
};
// coherent host memory the device addresses: its stores are visible to the host once the stream has
// synchronised, and the host's stores to a launch that follows them
template <typename T>
using PinMappedOf = PinBuf<T, hipHostMallocCoherent | hipHostMallocMapped>;
using PinMapped = PinMappedOf<char>;

// an event created at first use and destroyed with its owner
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    int ensure(unsigned flags) {
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, flags));
        return 0;
    }
    void release() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};

// Reading another context's device memory on my stream: between begin and end, what is enqueued on
// `mine` runs behind everything `theirs` holds at begin, and whatever `theirs` is given after end runs
// behind it.  The two events are created by the first begin, both or neither.  Not for use inside a
// stream capture: event creation is not captured.
struct StreamBorrow {
    Event taken, given;  // recorded on theirs at begin; on mine at end
    int begin(hipStream_t mine, hipStream_t theirs) {
        int rc;
        if ((rc = taken.ensure(hipEventDisableTiming)) || (rc = given.ensure(hipEventDisableTiming))) {
            taken.release();
            given.release();
            return rc;
        }
        HIP_TRY(hipEventRecord(taken.e, theirs));
        HIP_TRY(hipStreamWaitEvent(mine, taken.e, 0));
        return 0;
    }
    int end(hipStream_t mine, hipStream_t theirs) {
        HIP_TRY(hipEventRecord(given.e, mine));
        HIP_TRY(hipStreamWaitEvent(theirs, given.e, 0));
        return 0;
    }
};

struct PendingEv {
    int slot;
    hipEvent_t a, b;
};
// the events of the timed launches, created ahead of them and reused (KernelTimer::drain returns them)
struct EventPool {
    std::vector<hipEvent_t> free;
    EventPool() = default;
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool() {
        for (hipEvent_t e : free) (void)hipEventDestroy(e);
    }
};

// The kernel timing of one context (ldso_*_set_kernel_timing / _get_kernel_times): the events around
// its timed launches and the time and launch count they have measured per slot.  The owner
// synchronises its stream, calls drain() and then reads ms / count.
template <int kSlots>
struct KernelTimer {
    const unsigned flags;      // the events' creation flags
    const char *const *names;  // [kSlots], for the error text of a failed launch
    bool on = false;
    double ms[kSlots] = {0};
    long long count[kSlots] = {0};
    std::vector<PendingEv> pending;
    EventPool pool;
    KernelTimer(unsigned event_flags, const char *const *slot_names) : flags(event_flags), names(slot_names) {}
    ~KernelTimer() {  // whatever the owner did not drain
        for (const PendingEv &pe : pending) {
            pool.free.push_back(pe.a);
            pool.free.push_back(pe.b);
        }
    }
    void reset() {
        for (int i = 0; i < kSlots; i++) {
            ms[i] = 0;
            count[i] = 0;
        }
    }
    // events created ahead of the launches: hipEventCreate is a host call of tens of us, which inside
    // a timed loop would stall the launches (kept in the pool across calls)
    void reserve(size_t n) {
        while (pool.free.size() < n) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, flags) != hipSuccess) break;
            pool.free.push_back(e);
        }
    }
    hipEvent_t get_event() {
        if (!pool.free.empty()) {
            hipEvent_t e = pool.free.back();
            pool.free.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) e = nullptr;
        return e;
    }
    // the pending launches have completed: their times go to the slots, their events to the pool
    void drain() {
        for (const PendingEv &pe : pending) {
            (void)hipEventSynchronize(pe.b);
            float t = 0;
            (void)hipEventElapsedTime(&t, pe.a, pe.b);
            ms[pe.slot] += t;
            count[pe.slot] += 1;
            pool.free.push_back(pe.a);
            pool.free.push_back(pe.b);
        }
        pending.clear();
    }
    // One launch into slot `slot`.  timed: two events from the pool are handed to fn(a, b) and queued
    // for drain(); else fn(nullptr, nullptr).  record_on: the stream on which the events are recorded
    // around the launch, or nullptr when the launch stamps them itself.  The launch's error becomes
    // the call's, and then the events go back to the pool.
    template <typename F>
    int launch(int slot, bool timed, hipStream_t record_on, F &&fn) {
        hipEvent_t a = nullptr, b = nullptr;
        if (timed) {
            a = get_event();
            b = get_event();
            if (!a || !b) {
                if (a) pool.free.push_back(a);
                return fail(-2, "hipEventCreateWithFlags failed");
            }
            if (record_on) (void)hipEventRecord(a, record_on);
        }
        fn(a, b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            if (timed) {
                pool.free.push_back(a);
                pool.free.push_back(b);
            }
            return fail(-2, std::string("launch ") + names[slot] + ": " + hipGetErrorString(e));
        }
        if (timed) {
            if (record_on) (void)hipEventRecord(b, record_on);
            pending.push_back({slot, a, b});
        }
        return 0;
    }
};

}  // namespace
