// run_tiles_dev.hpp -- device code shared by the kernels that join a finished run's edge list with the capture it came
// from, tile by tile (run_levels.hip, run_moments.hip): the search in the list, and what a tile knows about the list
// before it looks at a sample.  The walk itself is described in run_levels.hip.
#pragma once

#include "edge_list_dev.hpp"
#include "kernels.hpp"

#include <hip/hip_runtime.h>

namespace ookd {

constexpr int kRunLevelThreads = 256;
constexpr int kRunLevelWaves = kRunLevelThreads / 64;
constexpr uint32_t kRunLevelSegs = (uint32_t)(kRunLevelWaves * kLevelBins);     // the segment table: the survey's histogram space
constexpr uint32_t kNoSeg = 0xffffffffu;

// first index in [lo, hi) whose edge is > pos (kAbove) or >= pos
template <bool kAbove>
__device__ __forceinline__ uint64_t edge_search(const uint64_t *edges, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t e = edges[mid];
        if (kAbove ? e <= pos : e < pos) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// What a tile knows about the list before it looks at a sample (all of it workgroup-uniform)
struct TileRuns {
    uint64_t t_lo, t_hi;        // the capture's edges inside (j0, j0 + len): list indices
    uint64_t k1;                // the capture's edges at or below j0: its parity is the level of output j0
    uint32_t nseg;              // on-run segments inside the tile, each of at least one output
};

// Fills `t` for the tile of `len` outputs at j0 (a tile never straddles two blocks: it is a power of two up to 1024
// outputs) from the edges of its block, kept inside the capture's range [lo_c, hi_c); a list with one block per
// capture (a cleaned list) is searched whole.  -> the tile holds an on output.  A tile that is off at its first output
// and has no edge behind it is all off.
__device__ __forceinline__ bool tile_runs(const EdgeListView &list, const uint32_t *blk, uint64_t lo_c, uint64_t hi_c,
                                          uint64_t j0, uint32_t len, TileRuns &t) {
    uint64_t b = j0 >> kBlockShift;
    if (b >= list.blocks_per_cap) b = list.blocks_per_cap - 1u;
    uint64_t b_lo = blk[b], b_hi = blk[b + 1u];
    if (b_hi > hi_c) b_hi = hi_c;
    if (b_lo < lo_c) b_lo = lo_c;
    if (b_lo > b_hi) b_lo = b_hi;
    t.t_lo = edge_search<true>(list.edges, b_lo, b_hi, j0);
    t.t_hi = edge_search<false>(list.edges, t.t_lo, b_hi, j0 + len);
    t.k1 = t.t_lo - lo_c;
    const uint32_t on0 = (uint32_t)(t.k1 & 1ull);
    const uint64_t inside = t.t_hi - t.t_lo;
    const uint64_t nseg = on0 ? 1u + inside / 2u : (inside + 1u) / 2u;
    t.nseg = nseg > kRunLevelSegs ? kRunLevelSegs : (uint32_t)nseg;     // (<= 512 for an increasing list)
    return on0 != 0u || inside != 0u;
}

}  // namespace ookd
