// pulses.hpp -- pulse survey: what pulses.hip (the kernel) and pulses.cpp (its C ABI and the host-only class rule)
// share: the bin rule, the kernel's parameters and its launch.  The contract is in include/ookiedokie_amd.h; what
// rx.cpp shares with pulses.cpp is in edge_pass.hpp.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "edge_list_dev.hpp"

namespace ookd {

constexpr int kPulseBins = 512;                 // OOKD_PULSE_BINS
constexpr uint32_t kPulseKeys = 2u * kPulseBins;        // (level, bin) pairs: key = level * kPulseBins + bin
// per capture in device memory: (count, sum) per key, then E, e[0], e[E-1] and a spare word
constexpr uint32_t kPulseMetaWord = 2u * kPulseKeys;
constexpr uint32_t kPulseWords = kPulseMetaWord + 4u;

// the header's bin rule; 0 for a length of 0 (no run has it)
__host__ __device__ __forceinline__ uint32_t pulse_bin_of(uint64_t d) {
    if (d < 32u) return (uint32_t)d;
    const uint32_t o = 63u - (uint32_t)__builtin_clzll(d);
    const uint32_t b = 32u + 16u * (o - 5u) + ((uint32_t)(d >> (o - 4u)) & 15u);
    return b > (uint32_t)(kPulseBins - 1) ? (uint32_t)(kPulseBins - 1) : b;
}

struct PulseParams {
    EdgeListView list;
    unsigned long long *result;     // [list.num_captures][kPulseWords], zero at launch
};
constexpr uint32_t kPulseThreads = 256;
constexpr uint32_t kPulseEdgesPerStep = 2u * kPulseThreads;     // a workgroup's step: two edges per lane
constexpr uint32_t kPulseStepsPerGroup = 16;                    // steps a workgroup is sized for (the grid strides beyond)
constexpr uint32_t kPulseMaxGroups = 2048;
// expect_edges sizes the grid only (the host's count of the run's edges); the kernel reads every range on the device
hipError_t launch_pulse_hist(const PulseParams &p, uint64_t expect_edges, hipStream_t stream);

}  // namespace ookd
