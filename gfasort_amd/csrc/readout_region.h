// readout_region.h — the byte map of the one allocation a read-out works in (capi.hip: a context's K7 scratch; capi_batch.hip: a
// batch's device buffer, and the pinned staging that mirrors its front): [what goes up | what comes back | scratch that never leaves].
// Host only and free of HIP: tests/test_readout_region_host.py builds every entry's map in a program of its own under the address
// and undefined-behaviour sanitizers and holds it to the formula written out.
#pragma once
#include <stdint.h>

namespace gfs {
struct Region {
    // A part of `bytes` bytes behind the parts so far, on the next 8-byte boundary (the one rounding rule): its offset.  A part of no
    // bytes takes no room: it starts where the next one does.
    uint64_t add(uint64_t bytes) {
        const uint64_t at = (end_ + 7) / 8 * 8;
        if (bytes) end_ = at + bytes;
        return at;
    }
    void end_upload() { uploaded_ = end_; }               // the two marks, set while building: the parts so far are what the host sends,
    void end_staging() { staged_ = end_; }                // ... are what the pinned staging mirrors
    uint64_t uploaded() const { return uploaded_; }       // the end of what goes up
    uint64_t staged() const { return staged_; }           // the end of what the staging holds: its size
    uint64_t bytes() const { return end_; }               // the end of everything: what the device buffer is reserved with
    template <typename T> static T *at(void *base, uint64_t part) { return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + part); }

private:
    uint64_t end_ = 0, uploaded_ = 0, staged_ = 0;
};
}  // namespace gfs
