// pulse_run.hpp -- pulse survey, host side only: what rx.cpp (the context whose edge list the survey reads) and
// pulses.cpp share.  No device code: the kernel's side is pulses.hpp.
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "common.hpp"

namespace ookd {

// The last run of an rx context as the pulse survey sees it (rx.cpp fills it: ookd_rx is its own)
struct PulseRun {
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
struct PulseCtx;                    // the survey's buffers and cached results, made by the first ookd_rx_pulse_hist
void pulse_ctx_free(PulseCtx *p);   // (the caller has made the context's device current)

}  // namespace ookd

void ookd_rx_pulse_run(const ookd_rx *rx, ookd::PulseRun *out);
ookd::PulseCtx **ookd_rx_pulse_ctx(ookd_rx *rx);
