// symbols.hpp -- symbol survey: what symbols.hip (the kernels) and symbols.cpp (their C ABI and the host-only coding
// and device rules) share: the result's layout in device memory, the kernels' parameters and their launch.  The
// contract is in include/ookiedokie_amd.h; what rx.cpp shares with symbols.cpp is in edge_pass.hpp.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "edge_list_dev.hpp"

namespace ookd {

constexpr uint32_t kSymClasses = 16;                    // OOKD_SYMBOL_MAX_CLASSES; class 16 = none
constexpr uint32_t kSymSide = kSymClasses + 1u;         // OOKD_SYMBOL_KINDS
constexpr uint32_t kSymKinds = kSymSide * kSymSide;     // key = on class * 17 + off class
constexpr uint32_t kFrameBins = 512;                    // OOKD_FRAME_BINS
enum : uint8_t { kRoleOther = 0, kRoleSync = 1, kRoleZero = 2, kRoleOne = 3 };

// the result in device memory, 64-bit words, zero at launch
constexpr uint32_t kSymWordS = 0;                       // S
constexpr uint32_t kSymWordKinds = 1;                   // [kSymKinds]
constexpr uint32_t kSymWordSyncs = kSymWordKinds + kSymKinds;   // num_syncs, head_symbols, tail_symbols
constexpr uint32_t kSymWordFrames = kSymWordSyncs + 3u;         // [2][kFrameBins]
constexpr uint32_t kSymWords = kSymWordFrames + 2u * kFrameBins;

constexpr uint32_t kSymThreads = 256;
constexpr uint32_t kSymPerThread = 4;                   // consecutive symbols of one lane
constexpr uint32_t kSymTile = kSymThreads * kSymPerThread;      // symbols a workgroup takes per step
constexpr uint32_t kSymTilesPerGroup = 8;               // steps a workgroup is sized for (the grid strides beyond)
constexpr uint32_t kSymMaxGroups = 2048;
constexpr uint32_t kSymScanThreads = 256;               // aggregates the scan takes per step
constexpr uint32_t kSymNoSync = 0xffffffffu;

// What a stretch of symbols says to what follows it: the position of its last sync (kSymNoSync: it has none) and the
// symbols of role OTHER behind that sync (in all of it, without one).  first / syncs serve the totals only.
struct SymAgg {
    uint32_t last, others, first, syncs;
};
// the same for everything in front of a tile
struct SymCarry {
    uint32_t last, others;
};

struct SymParams {
    EdgeListView list;
    uint32_t capture;               // the one asked about
    uint32_t num_tiles_cap;         // tiles agg / carry hold: no tile at or beyond is written
    unsigned long long *result;     // [kSymWords], zero at launch
    SymAgg *agg;                    // [num_tiles_cap]
    SymCarry *carry;                // [num_tiles_cap]
    uint32_t num_classes[2];        // [level]
    uint64_t lower[2][kSymClasses], upper[2][kSymClasses];
    uint8_t role[kSymKinds + 7u];   // by key
};

// tiles a list of `edges` edges has at most
inline uint32_t sym_tiles_of(uint64_t edges) {
    const uint64_t s = edges < 3u ? 0u : (edges - 1u) / 2u;
    return (uint32_t)((s + kSymTile - 1u) / kSymTile);
}

// expect_edges sizes the grids only (the host's count of the run's edges, no fewer than the capture's); the kernels
// read the capture's range on the device.  with_roles = false: the kinds alone, one launch.
hipError_t launch_symbol_survey(const SymParams &p, bool with_roles, uint64_t expect_edges, hipStream_t stream);

}  // namespace ookd
