// burst_baseband.hpp -- burst basebands: what burst_baseband.hip (the kernels) and burst_baseband.cpp (their C ABI, the
// table rule and the contract on the host) share.  The contract is in include/ookiedokie_amd.h ("Burst basebands"),
// the design in DESIGN.md 4.25.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "bursts.hpp"
#include "kernels.hpp"

namespace ookd {

constexpr uint32_t kBasebandCf32 = 0, kBasebandSc16 = 1;    // OOKD_BASEBAND_*

// One burst of the baseband table as the filtering kernel searches it: the ends, like BurstDev, so that one compare
// answers "does the burst end behind output j".  Bursts ascend and never overlap; a burst without outputs has
// first_output == end_output == ceil(n / D), behind every burst that has outputs.
struct BasebandDev {
    uint64_t first_output;
    uint64_t end_output;            // first_output + num_outputs
    uint64_t offset;                // element of the cut the burst begins at
};
static_assert(sizeof(BasebandDev) == 24, "three 64-bit words, as ookd_baseband_burst");

// ceil(x / D) for D >= 1, without the sum overflowing
__host__ __device__ __forceinline__ uint64_t baseband_ceil(uint64_t x, uint64_t D) { return x / D + (x % D ? 1u : 0u); }

// s of the contract: one rail of an SC16Q11 element -- v * 2048 in float32, a NaN is 0, clamped to [-32768, 32767],
// to the nearest integer, ties to even.
__host__ __device__ __forceinline__ int32_t baseband_q16(float v) {
    float w = v * 2048.0f;
    w = w != w ? 0.0f : w;
    w = w > 32767.0f ? 32767.0f : (w < -32768.0f ? -32768.0f : w);
    return (int32_t)__builtin_rintf(w);
}

// The result in device memory, zero at launch: [0] = tiles filtered.
constexpr uint32_t kBasebandWords = 1;

struct BasebandParams {
    // the survey's view of the filter and of the capture, as RunLevelParams::sv (survey_tile's LDS geometry; the
    // histogram space is not used)
    SurveyParams sv;
    uint64_t n_valid;               // samples of a capture that exist in memory
    uint32_t capture;               // the capture or carrier list the table belongs to (blockIdx.y is added)
    uint32_t one_source;            // a carrier context: every list reads capture 0 of iq
    uint32_t ctap_floats;           // floats from one list's complex taps to the next list's (0: all lists share them)
    uint32_t format;                // kBasebandCf32 / kBasebandSc16
    const float *ctaps;             // (re, im) pairs, stage s at 2 * tap_off, or null: real taps (sv.taps)
    const BasebandDev *table;       // the capture's entries
    uint64_t num_bursts;
    uint64_t total;                 // elements of the cut: nothing at or beyond is written
    void *out;                      // float2[total] or int16[total][2]
    unsigned long long *result;     // [kBasebandWords]
};

// One thread per entry of the raw table: `out` receives the capture's baseband table (D >= 1).
hipError_t launch_baseband_table(const BurstDev *table, uint64_t num_bursts, uint64_t D, BasebandDev *out, hipStream_t stream);

// The sparse pass over one capture.  lds_bytes: survey_tile's.  Nothing to launch for total = 0.
hipError_t launch_burst_baseband(const BasebandParams &p, size_t lds_bytes, hipStream_t stream);

}  // namespace ookd
