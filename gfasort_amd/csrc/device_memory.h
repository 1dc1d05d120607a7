// device_memory.h — the two owners of the library's host code: gfs::Buffer for one allocation (gfs::Array<T>: the same, read as a
// T *) and gfs::EventPair for a pair of events.  Every hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipEventCreate /
// hipEventDestroy of the library is in here.  HIP only; nothing here is exported from the shared object.
#pragma once
#include "../../include/gfasort_hip.h"
#include "capi_error.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>

#define GFS_LOCAL __attribute__((visibility("hidden")))       // not exported from the shared object

namespace gfs {
// One allocation, device memory or (pinned) page-locked host memory, freed when its owner goes — or a caller's pointer, borrowed
// and never freed.  The caller has set the device.
struct GFS_LOCAL Buffer {
    void *p = nullptr;
    uint64_t bytes = 0;                // (0 while borrowed: the caller knows the size)
    bool pinned = false, borrowed = false;
    explicit Buffer(bool pinned_ = false) : pinned(pinned_) {}
    Buffer(Buffer &&o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned), borrowed(o.borrowed) { o.p = nullptr; o.bytes = 0; o.borrowed = false; }   // (move-only)
    ~Buffer() { reset(); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    hipError_t release() {
        const hipError_t e = !p || borrowed ? hipSuccess : pinned ? hipHostFree(p) : hipFree(p);
        p = nullptr; bytes = 0; borrowed = false;
        return e;
    }
    void reset() { (void)release(); }
    // Holds the caller's pointer from here on; what the buffer owned is freed first.
    hipError_t borrow(void *theirs) {
        const hipError_t e = release();
        p = theirs; borrowed = theirs != nullptr;
        return e;
    }
    // At least `need` bytes.  Only grows, and what the buffer held is lost: it frees (a synchronisation point) before it allocates.
    hipError_t grow(uint64_t need) {
        if (bytes >= need) return hipSuccess;
        hipError_t e = release();
        if (e == hipSuccess) e = pinned ? hipHostMalloc(&p, need, hipHostMallocDefault) : hipMalloc(&p, need);
        if (e != hipSuccess) p = nullptr; else bytes = need;
        return e;
    }
    int reserve(uint64_t need, const char *what = nullptr) {               // grow, reported through the error slot
        const hipError_t e = grow(need);
        if (e == hipSuccess) return GFS_OK;
        return gfs_set_error(GFS_E_HIP, std::string(what ? what : pinned ? "hipHostMalloc" : "hipMalloc") + ": " + hipGetErrorString(e));
    }
};
// A Buffer of T: reads as the T * it holds, so that kernel arguments, pointer arithmetic and null tests stay what they were.
template <typename T> struct GFS_LOCAL Array : Buffer {
    operator T *() const { return static_cast<T *>(p); }
};

// Two events that bracket work on a stream, created on first use (or by create) and destroyed with their owner.
struct GFS_LOCAL EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(EventPair &&o) noexcept : e0(o.e0), e1(o.e1) { o.e0 = o.e1 = nullptr; }   // (move-only)
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    hipError_t create() {
        const hipError_t e = e0 ? hipSuccess : hipEventCreate(&e0);
        return e == hipSuccess && !e1 ? hipEventCreate(&e1) : e;
    }
    int ready() {                                                          // create, reported through the error slot
        const hipError_t e = create();
        return e == hipSuccess ? GFS_OK : gfs_set_error(GFS_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    hipError_t start(hipStream_t st) { const hipError_t e = create(); return e == hipSuccess ? hipEventRecord(e0, st) : e; }
    hipError_t stop(hipStream_t st) { return e1 ? hipEventRecord(e1, st) : hipSuccess; }            // (never started: nothing to stop)
    bool elapsed(float *ms) const { return e0 && e1 && hipEventElapsedTime(ms, e0, e1) == hipSuccess; }   // after both were reached
};

template <typename T> constexpr bool sole_owner =
    !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value && std::is_nothrow_move_constructible<T>::value;
static_assert(sole_owner<Buffer> && sole_owner<Array<double>> && sole_owner<EventPair>, "not copyable; moves without throwing (std::vector)");
}  // namespace gfs
