// bursts.hpp -- burst extraction: what bursts.hip (the kernels) and bursts.cpp (their C ABI and the host rule
// ookd_find_bursts) share.  The contract is in include/ookiedokie_amd.h ("Burst extraction"), the design in
// DESIGN.md 4.22.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "edge_list_dev.hpp"

namespace ookd {

// ---- the table pass: a scan over every capture's on-runs, in clean.hip's three launches ------------------------

constexpr uint32_t kBurstThreads = 256;
constexpr uint32_t kBurstRunsPerThread = 4;             // consecutive on-runs (eight edges) of one lane
constexpr uint32_t kBurstTileRuns = kBurstThreads * kBurstRunsPerThread;
constexpr uint32_t kBurstTile = 2u * kBurstTileRuns;    // edges of a tile; a tile lies inside one capture
constexpr uint32_t kBurstMaxGroups = 2048;              // (the grid strides beyond)
constexpr uint32_t kBurstScanPerThread = 8;             // consecutive tile aggregates of one lane of the aggregate scan

// The result in device memory, 64-bit words per capture, zero at launch: bursts, total samples, E, the list index of
// the capture's first edge, then what the aggregate scan keeps between its two halves (the sums in front of the
// capture's first tile).
constexpr uint32_t kBurstWordCount = 0, kBurstWordTotal = 1, kBurstWordEdges = 2, kBurstWordLo = 3, kBurstWordBegin = 4;
constexpr uint32_t kBurstWords = 8;

// One burst as the table pass leaves it in device memory and as the copy reads it.  Two lanes write one entry -- the
// one at the burst's first run and the one at its last -- and neither knows what the other holds, so the entry keeps
// the ends and the host takes the differences (ookd_burst: num_samples = end_offset - offset, num_runs = end_run -
// first_run).
struct BurstDev {
    uint64_t first_sample;
    uint64_t end_offset;            // offset + num_samples
    uint64_t offset;
    uint64_t first_run;
    uint64_t end_run;               // r1 + 1
};
static_assert(sizeof(BurstDev) == 40, "five 64-bit words, as ookd_burst");

// Where capture c's bursts begin in the table, in entries: lo = the list index of its first edge.  A capture has at
// most ceil(E_c / 2) bursts and floor((lo + E_c + c + 1) / 2) - floor((lo + c) / 2) >= ceil(E_c / 2), so no two
// captures share an entry (run_levels.hpp places its peaks the same way).
__host__ __device__ __forceinline__ uint64_t burst_table_base(uint64_t lo, uint32_t c) { return (lo + c) >> 1; }
// entries that hold the table of a run of `edges` edges in `captures` captures
inline uint64_t burst_table_slots(uint64_t edges, uint32_t captures) { return ((edges + captures) >> 1) + 1u; }

// min(n, x * D) without the product overflowing
__host__ __device__ __forceinline__ uint64_t burst_scale(uint64_t x, uint64_t D, uint64_t n) {
    if (x > n / D) return n;
    const uint64_t y = x * D;
    return y < n ? y : n;
}
// min(n_out, f + post) without the sum overflowing
__host__ __device__ __forceinline__ uint64_t burst_hi(uint64_t f, uint64_t post, uint64_t n_out) {
    if (f >= n_out) return n_out;
    return post >= n_out - f ? n_out : f + post;
}

// What a tile says to what follows it
struct BurstAgg {
    uint64_t samples;               // sum of its runs' contributions
    uint32_t starts;                // bursts that begin in it
    uint32_t capture;               // whose tile it is; bit 31: the capture's first tile, bit 30: its last
};
static_assert(sizeof(BurstAgg) == 16, "one aggregate is one 16-byte word");
constexpr uint32_t kBurstFirst = 1u << 31, kBurstLast = 1u << 30;

// What lies in front of a tile, over all captures (the capture's own begin is in its result words)
struct BurstCarry {
    uint64_t samples;
    uint64_t starts;
};

struct BurstParams {
    EdgeListView list;
    uint64_t n_out, D, n;           // decimated samples per capture, total decimation (>= 1), input samples that exist
    uint64_t pre, post, max_gap;
    uint32_t num_tiles_cap;         // tiles agg / carry hold: no tile at or beyond is written
    uint32_t reserved;
    uint64_t table_slots;           // entries `table` holds: nothing at or beyond is written
    unsigned long long *result;     // [list.num_captures][kBurstWords], zero at launch
    BurstAgg *agg;                  // [num_tiles_cap]
    BurstCarry *carry;              // [num_tiles_cap]
    BurstDev *table;                // capture c's entries at burst_table_base(lo_c, c)
};

// tiles a run of `edges` edges in `captures` captures has at most (every capture may end with a partial tile)
inline uint64_t burst_tiles_of(uint64_t edges, uint32_t captures) {
    return (edges + kBurstTile - 1u) / kBurstTile + captures;
}

// expect_edges sizes the grids only (the host's count of the run's edges); the kernels read every range on the device
hipError_t launch_burst_table(const BurstParams &p, uint64_t expect_edges, hipStream_t stream);

// ---- the copy: the cut of one capture, in 16-byte vectors ------------------------------------------------------

constexpr uint32_t kBurstCopyThreads = 256;
constexpr uint32_t kBurstCopyVecPerThread = 16;         // a workgroup's span is 4096 vectors = 64 KiB of the cut
constexpr uint32_t kBurstCopySpan = kBurstCopyThreads * kBurstCopyVecPerThread;

struct BurstCopyParams {
    const BurstDev *table;          // the capture's entries
    uint64_t num_bursts;
    uint64_t total;                 // samples of the cut: nothing at or beyond is written
    const void *src;                // the capture's first sample
    uint64_t n;                     // samples of it that exist: nothing at or beyond is read
    void *dst;
    uint32_t sample_bytes;          // 4 or 2
    uint32_t reserved;
};

// nothing to launch for total = 0
hipError_t launch_burst_copy(const BurstCopyParams &p, hipStream_t stream);

// ---- the table as another reader of it (burst_spectra.cpp) sees it ---------------------------------------------

struct EdgeRun;
struct BurstTableRef {
    const BurstDev *d_table = nullptr;  // the capture's entries in device memory
    const BurstDev *table = nullptr;    // and on the host
    uint64_t num_bursts = 0, total = 0;
    uint64_t made = 0;                  // counts the tables made: the same number is the same table
    bool clean = false;                 // of the cleaned list
};
// The table the context's copy calls are about (the form ookd_rx_bursts was last called with for the last run) for
// `capture`, and the last run; false + error without one.
bool burst_table_ref(const char *who, const ookd_rx *rx, uint32_t capture, EdgeRun &run, BurstTableRef &out);

}  // namespace ookd
