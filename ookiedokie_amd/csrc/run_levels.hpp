// run_levels.hpp -- pulse levels: what run_levels.hip (the kernels) and run_levels.cpp (their C ABI and the host-only
// message rule) share.  The contract is in include/ookiedokie_amd.h ("Pulse levels"), the design in DESIGN.md 4.21.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_list_dev.hpp"
#include "kernels.hpp"

namespace ookd {

// The result in device memory, zero at launch: per capture kRunLevelWords 64-bit words -- the histogram of its peaks,
// then E and the tiles the kernel filtered -- and behind all captures the peaks, one uint32 bit pattern per on-run.
constexpr uint32_t kRunLevelMetaWord = kLevelBins;      // [0] = E, [1] = tiles filtered, [2] = list index of the first edge
constexpr uint32_t kRunLevelWords = kLevelBins + 3;

// Where capture c's peaks begin, in runs: lo = the list index of its first edge.  Capture c has ceil(E_c / 2) runs and
// floor((lo + E_c + c + 1) / 2) - floor((lo + c) / 2) >= ceil(E_c / 2), so no two captures share a slot.
__host__ __device__ __forceinline__ uint64_t run_peak_base(uint64_t lo, uint32_t c) { return (lo + c) >> 1; }
// slots that hold the peaks of a run of `edges` edges in `captures` captures
inline uint64_t run_peak_slots(uint64_t edges, uint32_t captures) { return ((edges + captures) >> 1) + 1u; }

struct RunLevelParams {
    EdgeListView list;
    // the survey's view of the filter and of the capture (survey_tile filled the LDS geometry): iq, sample_fmt,
    // cap_stride, n_out, stages, taps, tile, num_tiles; n_out counts the padding to whole buffers here, and inputs at
    // or beyond n_valid are zeros that are never loaded
    SurveyParams sv;
    uint64_t n_valid;               // samples of a capture that exist in memory
    uint32_t one_source;            // a carrier context: every list reads capture 0 of iq
    uint32_t ctap_floats;           // floats from one list's complex taps to the next list's (0: all lists share them)
    const float *ctaps;             // (re, im) pairs, stage s at 2 * tap_off, or null: real taps (sv.taps)
    unsigned long long *result;     // [list.num_captures][kRunLevelWords]
    uint32_t *peaks;                // [peak_slots]: capture c's at run_peak_base(lo_c, c)
    uint64_t peak_slots;            // nothing at or beyond is written
};

// The sparse pass and, behind it, the histogram of the peaks.  lds_bytes: survey_tile's.
hipError_t launch_run_levels(const RunLevelParams &p, size_t lds_bytes, hipStream_t stream);

struct FrontPlan;

// What the pass reads again of the context's last run besides its edge list (rx.cpp fills it: ookd_rx is its own)
struct RunLevelSource {
    const FrontPlan *plan = nullptr;    // stages, real taps, and a tuned or carrier context's complex taps
    const void *iq = nullptr;           // the capture as submitted (ookd_rx_process_host: the context's staging copy)
    uint64_t stride = 0;                // samples between captures
    uint64_t n_valid = 0;               // samples per capture
};

}  // namespace ookd

void ookd_rx_level_source(const ookd_rx *rx, ookd::RunLevelSource *out);
