// clean.hpp -- edge cleaning: what clean.hip (the kernels) and clean.cpp (their C ABI and the host rule) share -- the
// tile, the aggregates, the kernels' parameters and their launch -- and what the two clean readers (pulses.cpp,
// symbols.cpp) ask of clean.cpp: the cleaned list of the last run as an EdgeRun.  The contract is in
// include/ookiedokie_amd.h ("Edge cleaning"); what rx.cpp shares with clean.cpp is in edge_pass.hpp -- and, for a
// debounced context whose runs clean their list in their own chain ("Debounced decode"), at the end of this file.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "edge_list_dev.hpp"

namespace ookd {

constexpr uint32_t kCleanThreads = 256;
constexpr uint32_t kCleanPerThread = 8;                 // consecutive runs (and edges) of one lane
constexpr uint32_t kCleanTile = kCleanThreads * kCleanPerThread;       // edges of a tile; a tile lies inside one capture
constexpr uint32_t kCleanMaxGroups = 2048;              // (the grid strides beyond)
constexpr uint32_t kCleanScanPerThread = 8;             // consecutive tile aggregates of one lane of the aggregate scan

// the result in device memory, 64-bit words per capture, zero at launch: edges_in, edges_out, deleted[0], deleted[1],
// then what the aggregate scan keeps between its two halves (the sums in front of the capture's first tile)
constexpr uint32_t kCleanWordIn = 0, kCleanWordOut = 1, kCleanWordDel = 2, kCleanWordBegin = 4;
constexpr uint32_t kCleanWords = 8;

// A map of one bit, d in front of a stretch of runs -> d behind it: bit 0 = the answer to 0, bit 1 = the answer to 1.
// The recurrence d(i) = short(i) && !d(i-1) is `not` at a short run and `const 0` at any other.
enum : uint32_t { kMapConst0 = 0u, kMapNot = 1u, kMapId = 2u, kMapConst1 = 3u };
// (f, then g)
__host__ __device__ __forceinline__ uint32_t map_then(uint32_t f, uint32_t g) {
    return ((g >> (f & 1u)) & 1u) | (((g >> ((f >> 1) & 1u)) & 1u) << 1);
}

// What a tile says to what follows it, for both possible d in front of it ([x] = that d)
struct CleanAgg {
    uint32_t kept[2];               // edges of the tile that stay
    uint32_t del[2][2];             // [x][level]: runs of the tile that are deleted
    uint32_t map;                   // kMap*: d behind the tile's last run
    uint32_t capture;               // whose tile it is; bit 31: the capture's first tile, bit 30: its last
};
static_assert(sizeof(CleanAgg) == 32, "one aggregate is two 16-byte words");
constexpr uint32_t kCleanFirst = 1u << 31, kCleanLast = 1u << 30;

// What lies in front of a tile
struct CleanCarry {
    uint32_t d;                     // d of the run before the tile's first (0 at a capture's first tile)
    uint32_t offset;                // cleaned edges in front of the tile, over all captures
};

struct CleanParams {
    EdgeListView list;
    uint64_t min_len[2];            // [level]: a run of that level shorter than this is short
    uint32_t num_tiles_cap;         // tiles agg / carry hold: no tile at or beyond is written
    uint32_t blk_prefix_capacity;   // words blk_prefix holds: nothing at or beyond is written
    uint64_t out_capacity;          // elements `out` holds: nothing at or beyond is written
    unsigned long long *result;     // [list.num_captures][kCleanWords], zero at launch
    CleanAgg *agg;                  // [num_tiles_cap]
    CleanCarry *carry;              // [num_tiles_cap]
    uint64_t *out;                  // the cleaned list, capture-major and compact
    uint32_t *out_prefix;           // [list.num_captures + 1]: capture c's cleaned edges are [out_prefix[c], out_prefix[c + 1])
    // the debounced decode only (null: the pass is its three kernels): the cleaned list's prefix over the run's own
    // blocks, [list.num_captures * list.blocks_per_cap + 1] -- entry (c, b) is the index in `out` of capture c's first
    // cleaned edge at or beyond b << kBlockShift (kernels.hpp), the last word the total: what FsmParams::blk_offset
    // is to the run's own list
    uint32_t *blk_prefix;
};

// tiles a run of `edges` edges in `captures` captures has at most (every capture may end with a partial tile)
inline uint64_t clean_tiles_of(uint64_t edges, uint32_t captures) {
    return (edges + kCleanTile - 1u) / kCleanTile + captures;
}

// expect_edges sizes the grids only (the host's count of the run's edges, or a bound of it); the kernels read every
// range on the device.  With p.blk_prefix set a fourth launch follows the three: the per-block prefix.
hipError_t launch_clean_edges(const CleanParams &p, uint64_t expect_edges, hipStream_t stream);

// For the clean readers: when the context's clean pass has answered the run `run` describes, puts the cleaned list in
// the place of the run's own (list, prefix with one block per capture, capacity, edge count) and returns true.
bool clean_run_view(ookd_rx *rx, EdgeRun &run);

// The debounced decode (rx.cpp): the clean pass as part of a run's chain.
// What the state machine reads in the place of the run's own list
struct CleanChainView {
    const uint64_t *edges = nullptr;        // the cleaned list
    const uint32_t *blk_prefix = nullptr;   // its per-block prefix (CleanParams::blk_prefix)
};
// Makes the context's clean pass if there is none and allocates everything a run of `captures` captures of `blocks`
// blocks each with up to `edge_capacity` edges needs; the addresses hold for the life of the context.  `view` is
// what the pass holds when the call returns, on failure too (then possibly null: the caller turns the debounce off).
// When a buffer a finished pass wrote had to be replaced, that pass's list is gone: the context has no cleaned list of
// the last run until the next run or ookd_rx_clean_edges makes one.
int clean_chain_reserve(ookd_rx *rx, int dev, uint64_t edge_capacity, uint32_t captures, uint32_t blocks, CleanChainView &view);
// Queues the pass for the run being queued (`run`: as ookd_rx_edge_run gives it now) behind its edge stage on
// run.stream and returns: no wait, no copy.  The list becomes the context's cleaned list of that run; the counts are
// fetched by the first reader that needs them.
hipError_t clean_chain_queue(ookd_rx *rx, const EdgeRun &run, uint64_t min_on, uint64_t min_off);

}  // namespace ookd
