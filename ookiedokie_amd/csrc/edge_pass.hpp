// edge_pass.hpp -- what the readers of a finished run's edge list (pulses.cpp, symbols.cpp, run_levels.cpp, bursts.cpp,
// run_moments.cpp, burst_spectra.cpp, burst_baseband.cpp) have in common on the host, and what they share with rx.cpp, the context whose edge list it is: the last run as a reader sees it, the
// refusals, and the timed pass with its result buffer.  `who` names the entry point in the messages.  No device code:
// the kernels' side is edge_list_dev.hpp.
#pragma once

#include <cstdint>
#include <functional>
#include <memory>

#include <hip/hip_runtime_api.h>

#include "common.hpp"

namespace ookd {

// The last run of an rx context as an edge-list reader sees it (rx.cpp fills it: ookd_rx is its own)
struct EdgeRun {
    int dev = 0;
    hipStream_t stream = nullptr;
    uint64_t serial = 0;            // counts the context's runs, 0 = none yet
    bool in_flight = false;         // submitted, not waited for
    bool valid = false;             // the run got as far as its edge count: the prefix and the list are this run's
    bool shard = false, pipelined = false, overflow = false;
    uint32_t captures = 0, blocks_per_cap = 0;
    uint64_t n_out = 0, num_edges = 0, edge_capacity = 0;
    const uint64_t *d_edges = nullptr;
    const uint32_t *d_blk_offset = nullptr;
};

// A reader's pass over the list: its result buffer on the device, the event pair that times it, and which run it last
// answered.  Made by the reader's first call, destroyed with the rx context (which has made its device current).  A
// reader derives from it and adds what it alone keeps.
struct EdgePass {
    unsigned long long *d_result = nullptr;
    size_t capacity = 0;            // 64-bit words d_result holds (grown, never shrunk)
    hipEvent_t t0 = nullptr, t1 = nullptr;
    uint64_t serial = 0;            // the run the last finished pass was about (EdgeRun::serial), 0 = none
    float kernel_ms = 0.0f;         // of that pass

    EdgePass() = default;
    EdgePass(const EdgePass &) = delete;
    EdgePass &operator=(const EdgePass &) = delete;
    virtual ~EdgePass();

    // One timed pass on run.stream: record t0, zero `words` words of d_result, `queue(d_result)` (the reader's
    // kernels), record t1, copy the words to `host`, synchronise.  OOKD_OK with serial and kernel_ms set, or an error
    // code + error with both zero.
    int run(const char *who, const EdgeRun &run, size_t words, uint64_t *host,
            const std::function<hipError_t(unsigned long long *)> &queue);
    // d_result holds `words` words from here on (what run() does first; a pass queued in a run's chain reserves ahead)
    int reserve_result(const char *who, int dev, size_t words);
};

// kEdgePassClean writes the cleaned list (clean.cpp); the two after it are the surveys' passes over that list
enum EdgePassId {
    kEdgePassPulse = 0,
    kEdgePassSymbol = 1,
    kEdgePassClean = 2,
    kEdgePassCleanPulse = 3,
    kEdgePassCleanSymbol = 4,
    kEdgePassLevels = 5,            // the pulse levels (run_levels.cpp) over the run's list, and over the cleaned one
    kEdgePassCleanLevels = 6,
    kEdgePassBursts = 7,            // the burst table (bursts.cpp) of the run's list, and of the cleaned one
    kEdgePassCleanBursts = 8,
    kEdgePassMoments = 9,           // the pulse moments (run_moments.cpp) over the run's list, and over the cleaned one
    kEdgePassCleanMoments = 10,
    kEdgePassBurstSpectra = 11,     // the burst spectra (burst_spectra.cpp) of the raw burst table, and of the clean one
    kEdgePassCleanBurstSpectra = 12,
    kEdgePassBaseband = 13,         // the burst basebands (burst_baseband.cpp) of the raw burst table, and of the clean one
    kEdgePassCleanBaseband = 14,
    kEdgePasses = 15
};

// The refusals every reader shares, after its own argument checks: fills `run`, then OOKD_OK, or OOKD_ERR_ARG (no
// finished run, a shard run, a pipelined run, capture out of range) or OOKD_ERR_CAPACITY (the list overflowed) + error.
int edge_run_check(const char *who, const ookd_rx *rx, uint32_t capture, EdgeRun &run);
// kernel_ms of the context's pass `id` when it answered the context's last run, else 0 (rx may be null)
float edge_pass_kernel_ms(const ookd_rx *rx, EdgePassId id);

}  // namespace ookd

// rx.cpp: the last run, and where the context keeps a reader's pass (null until the reader's first call)
void ookd_rx_edge_run(const ookd_rx *rx, ookd::EdgeRun *out);
std::unique_ptr<ookd::EdgePass> &ookd_rx_edge_pass(ookd_rx *rx, ookd::EdgePassId id);
