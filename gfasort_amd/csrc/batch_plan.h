// batch_plan.h — how gfs_batch_plan cuts a list of items into launches (include/gfasort_hip.h).  Host only and free of HIP, so
// that it can be compiled into a program of its own (tests/test_batch_host.py builds it with the address and undefined-behaviour
// sanitizers).
#pragma once
#include <stdint.h>

namespace gfs {

// Greedy, in the given order: an item goes into the current launch while the launch's workgroups stay within max_blocks (an
// exact fit is taken), else it opens the next one; an item never straddles two launches.  Returns the index of the first item
// that alone exceeds max_blocks, or n where there is none; launch_of_item[0..n) and *n_launches are complete only then.
inline uint64_t batch_plan(const uint64_t *blocks_of_item, uint64_t n, uint64_t max_blocks, uint32_t *launch_of_item, uint32_t *n_launches) {
    uint32_t launch = 0;
    uint64_t used = 0;
    bool open = false;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = blocks_of_item[i];
        if (b > max_blocks) { *n_launches = 0; return i; }
        if (open && b > max_blocks - used) { ++launch; used = 0; }     // (used <= max_blocks: no overflow)
        launch_of_item[i] = launch;
        used += b;
        open = true;
    }
    *n_launches = open ? launch + 1 : 0;
    return n;
}

}  // namespace gfs
