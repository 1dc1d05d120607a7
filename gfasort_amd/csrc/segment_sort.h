// segment_sort.h — the arithmetic of K6b's sorting network (batch_readout_kernels.hip): which element meets which at stage (k, j),
// which of the two keeps the smaller pair, and what a segment is padded with.  Free of HIP, so that the host can run the very
// schedule the kernel runs, serially (tests/test_batch_readout_host.py builds it with the address and undefined-behaviour
// sanitizers); the kernel takes every index and every decision from here.
//
// The network is the bitonic sorter over P = segment_padded(n) elements: for k = 2, 4 .. P and j = k/2, k/4 .. 1, element t meets
// t ^ j, and the lower of the two keeps the smaller pair where (t & k) == 0 (an ascending run), the larger otherwise.  Elements are
// pairs (key, index) compared by key, then index: real pairs are distinct (the index is the dense node index), so the order is
// total and the result is the one a stable sort by key gives.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFS_SEG_HD __host__ __device__ inline
#else
#define GFS_SEG_HD inline
#endif

namespace gfs {

constexpr uint32_t SEGMENT_SORT_CAP = 8192;               // nodes of the largest segment sorted in LDS: 8192 * (8 + 4) B = 96 KiB
constexpr uint32_t SEGMENT_WAVE = 64;                     // partner distances below this stay inside a wave
constexpr uint64_t SEGMENT_PAD_KEY = 0xFFFFFFFFFFFFFFFFull;   // above every real pair, NaNs (the all-ones key) included: a dense
constexpr uint32_t SEGMENT_PAD_INDEX = 0xFFFFFFFFu;           // index is below 2^31

// elements of the network for a segment of n nodes: the next power of two, and whole waves
GFS_SEG_HD uint32_t segment_padded(uint32_t n) {
    uint32_t p = SEGMENT_WAVE;
    while (p < n) p <<= 1;
    return p;
}
GFS_SEG_HD uint64_t segment_lds_bytes(uint32_t padded) { return (uint64_t)padded * (sizeof(uint64_t) + sizeof(uint32_t)); }
// workgroup size of a segment's launch: two elements per thread up to the 1024 threads of a workgroup
GFS_SEG_HD uint32_t segment_block(uint32_t padded) { return padded / 2 < 1024u ? (padded / 2 < SEGMENT_WAVE ? SEGMENT_WAVE : padded / 2) : 1024u; }

GFS_SEG_HD bool segment_pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }
GFS_SEG_HD uint32_t segment_partner(uint32_t t, uint32_t j) { return t ^ j; }
// the lower element of the q-th compare-exchange of a stage with partner distance j (q in 0 .. P/2): q with a 0 put in at bit log2 j
GFS_SEG_HD uint32_t segment_pair_low(uint32_t q, uint32_t j) { return ((q & ~(j - 1)) << 1) | (q & (j - 1)); }
// whether element t leaves stage (k, j) with the smaller of the two pairs
GFS_SEG_HD bool segment_keeps_min(uint32_t t, uint32_t k, uint32_t j) { return ((t & j) == 0) == ((t & k) == 0); }
// element t holds `mine` and its partner holds `other`: whether t leaves the stage with the partner's pair.  (Two padding
// pairs are equal; either answer leaves the same bits.)
GFS_SEG_HD bool segment_takes_other(uint32_t t, uint32_t k, uint32_t j, uint64_t k_mine, uint32_t i_mine, uint64_t k_other, uint32_t i_other) {
    const bool other_less = segment_pair_less(k_other, i_other, k_mine, i_mine);
    return segment_keeps_min(t, k, j) ? other_less : !other_less;
}

// The kernel's schedule, one element at a time.  keys / index: padded elements, the first n real, the rest written here;
// scratch_keys / scratch_index: padded elements (what the other lanes of a wave hold while a lane decides).  Stages with
// j >= SEGMENT_WAVE go pair by pair (the kernel: through LDS, a barrier per stage); the others element by element on a copy of
// the stage's input (the kernel: registers and wave shuffles).
inline void segment_sort_serial(uint64_t *keys, uint32_t *index, uint32_t n, uint32_t padded, uint64_t *scratch_keys, uint32_t *scratch_index) {
    for (uint32_t t = n; t < padded; ++t) { keys[t] = SEGMENT_PAD_KEY; index[t] = SEGMENT_PAD_INDEX; }
    for (uint32_t k = 2; k <= padded; k <<= 1) {
        uint32_t j = k >> 1;
        for (; j >= SEGMENT_WAVE; j >>= 1) {
            for (uint32_t q = 0; q < padded / 2; ++q) {
                const uint32_t lo = segment_pair_low(q, j), hi = segment_partner(lo, j);
                if (segment_takes_other(lo, k, j, keys[lo], index[lo], keys[hi], index[hi])) {
                    const uint64_t kk = keys[lo]; keys[lo] = keys[hi]; keys[hi] = kk;
                    const uint32_t ii = index[lo]; index[lo] = index[hi]; index[hi] = ii;
                }
            }
        }
        for (; j >= 1; j >>= 1) {
            for (uint32_t t = 0; t < padded; ++t) { scratch_keys[t] = keys[t]; scratch_index[t] = index[t]; }
            for (uint32_t t = 0; t < padded; ++t) {
                const uint32_t o = segment_partner(t, j);
                if (segment_takes_other(t, k, j, scratch_keys[t], scratch_index[t], scratch_keys[o], scratch_index[o])) {
                    keys[t] = scratch_keys[o]; index[t] = scratch_index[o];
                }
            }
        }
    }
}

}  // namespace gfs
