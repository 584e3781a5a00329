// run_moments.hpp -- pulse moments: what run_moments.hip (the kernel) and run_moments.cpp (its C ABI, the contract on
// the host and the host-only message rule) share.  The contract is in include/ookiedokie_amd.h ("Pulse moments"), the
// design in DESIGN.md 4.23.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_list_dev.hpp"
#include "kernels.hpp"
#include "run_levels.hpp"

namespace ookd {

// The result in device memory, zero at launch: per capture kRunMomentWords 64-bit words -- [0] = E, [1] = tiles
// filtered, [2] = list index of the first edge -- and behind all captures three int64 per on-run (power, lag_re,
// lag_im), capture c's at slot run_peak_base(lo_c, c) (run_levels.hpp: the levels' slots).
constexpr uint32_t kRunMomentWords = 3;
constexpr uint32_t kRunMomentSums = 3;

// Segments of a tile that are summed in LDS and leave the tile as one global add each; a tile's later segments go to
// global memory from every wave.  64: a tile of pulses holds a handful.
constexpr uint32_t kRunMomentTableSegs = 64;

// q of the contract: v clamped to [-2^32, 2^32] (a NaN is 0), times 2^30 in double -- exact --, to the nearest
// integer, ties to even.  As uint64 so that the sums wrap modulo 2^64 by definition.
__host__ __device__ __forceinline__ unsigned long long moment_q(float v) {
    const float lim = 4294967296.0f;
    float w = v != v ? 0.0f : v;
    w = w > lim ? lim : (w < -lim ? -lim : w);
    return (unsigned long long)(long long)__builtin_rint((double)w * 1073741824.0);
}

struct RunMomentParams {
    EdgeListView list;
    // as RunLevelParams::sv, with the LDS geometry of survey_tile_lag: lds_hist_off is the segment table
    SurveyParams sv;
    uint64_t n_valid;               // samples of a capture that exist in memory
    uint32_t one_source;            // a carrier context: every list reads capture 0 of iq
    uint32_t ctap_floats;           // floats from one list's complex taps to the next list's (0: all lists share them)
    const float *ctaps;             // (re, im) pairs, stage s at 2 * tap_off, or null: real taps (sv.taps)
    unsigned long long *result;     // [list.num_captures][kRunMomentWords]
    unsigned long long *moments;    // [slots][kRunMomentSums]
    uint64_t slots;                 // nothing at or beyond is written
    uint32_t table_segs;            // <= kRunMomentTableSegs; 0: every wave adds to global memory
};

// The sparse pass.  lds_bytes: survey_tile_lag's for kRunMomentTableSegs * kRunMomentSums words.
hipError_t launch_run_moments(const RunMomentParams &p, size_t lds_bytes, hipStream_t stream);

}  // namespace ookd
