// edge_list_dev.hpp -- device code shared by the kernels that read a finished run's edge list (pulses.hip,
// symbols.hip): the list as a kernel sees it, the two clamps that keep every load inside it, and the wave's
// aggregated histogram add.  The host side of the same readers is edge_pass.hpp.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_pass.hpp"

namespace ookd {

// The first member of a reader's kernel parameters
struct EdgeListView {
    const uint64_t *edges;          // the run's one edge list, capture-major
    uint64_t edge_capacity;         // elements of it that exist: nothing at or beyond is read
    const uint32_t *blk_offset;     // capture c's edges are [blk_offset[c * blocks_per_cap], blk_offset[(c + 1) * blocks_per_cap])
    uint32_t blocks_per_cap;
    uint32_t num_captures;
};
static_assert(sizeof(EdgeListView) == 32, "the readers' kernel arguments begin with these 32 bytes");

inline EdgeListView edge_list_view(const EdgeRun &run) {
    return EdgeListView{run.d_edges, run.edge_capacity, run.d_blk_offset, run.blocks_per_cap, run.captures};
}

// the list's end: the prefix's last word, and never beyond what the list can hold (the host refuses a run whose list
// overflowed; this keeps the loads inside the allocation whatever it was given)
__device__ __forceinline__ uint64_t edge_list_total(const EdgeListView &v) {
    const uint64_t total = v.blk_offset[(size_t)v.num_captures * v.blocks_per_cap];
    return total > v.edge_capacity ? v.edge_capacity : total;
}

// capture c's edges [lo, hi), inside [0, total]
__device__ __forceinline__ void edge_list_range(const EdgeListView &v, uint32_t c, uint64_t total, uint64_t &lo, uint64_t &hi) {
    lo = v.blk_offset[(size_t)c * v.blocks_per_cap];
    hi = v.blk_offset[(size_t)(c + 1u) * v.blocks_per_cap];
    if (hi > total) hi = total;
    if (lo > hi) lo = hi;
}

constexpr int kEdgePeelRounds = 6;      // distinct keys a wave looks at before its lanes add for themselves
constexpr uint32_t kEdgePeelMin = 8;    // a key held by fewer lanes is not worth the reduction: its lanes add for themselves

// sum over the wave (every lane calls it; lanes outside the group pass 0)
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, s);
    return v;
}

// Every lane of the wave calls this together.  An OOK capture puts nearly all runs of a level into a handful of bins
// and nearly all symbols into two or three kinds, so most lanes of a wave hold the same key: the wave finds the lanes
// that share the first pending lane's key, and that lane alone adds their count to the workgroup's histogram -- one
// LDS add per distinct key instead of up to 64 on one address.  A key held by few lanes (a rare timing; a capture
// whose runs spread over many bins) gains nothing from the reduction: its lanes step aside to add for themselves and
// the rounds go on with the next pending key, so a rare key in the first lane does not end them.
// kSum: hist holds (count, sum of len) per key, and the lanes' lengths are summed across the wave as well;
// otherwise one count per key, and len is not looked at.
template <bool kSum>
__device__ __forceinline__ void wave_peel_add(unsigned long long *hist, bool valid, uint32_t key, uint64_t len) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(valid), self = 0ull;
#pragma unroll 1
    for (int r = 0; r < kEdgePeelRounds && todo; ++r) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader);
        const bool mine = valid && key == lk;
        const uint64_t same = __ballot(mine) & todo;
        const uint32_t n = (uint32_t)__popcll(same);
        todo &= ~same;
        if (n < kEdgePeelMin) {                 // (wave-uniform)
            self |= same;
            continue;
        }
        if (kSum) {
            const uint64_t total = wave_sum_u64(mine ? len : 0ull);
            if ((int)lane == leader) {
                atomicAdd(&hist[2u * lk], (unsigned long long)n);
                atomicAdd(&hist[2u * lk + 1u], (unsigned long long)total);
            }
        } else if ((int)lane == leader) {
            atomicAdd(&hist[lk], (unsigned long long)n);
        }
    }
    self |= todo;
    if ((self >> lane) & 1ull) {
        if (kSum) {
            atomicAdd(&hist[2u * key], 1ull);
            atomicAdd(&hist[2u * key + 1u], (unsigned long long)len);
        } else {
            atomicAdd(&hist[key], 1ull);
        }
    }
}

}  // namespace ookd
