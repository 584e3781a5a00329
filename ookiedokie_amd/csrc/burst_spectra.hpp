// burst_spectra.hpp -- burst spectra: what burst_spectra.hip (the kernels) and burst_spectra.cpp (their C ABI and the
// host rule ookd_suggest_burst_carriers) share.  The contract is in include/ookiedokie_amd.h ("Burst spectra"), the
// design in DESIGN.md 4.24.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "bursts.hpp"
#include "kernels.hpp"

namespace ookd {

constexpr uint32_t kBurstSpecMinSpan = 32;              // OOKD_BURST_SPECTRA_MIN_SPAN
constexpr uint64_t kBurstSpecMaxRows = 8192;            // OOKD_BURST_SPECTRA_MAX_ROWS: 64 MiB of 8 KiB rows
constexpr uint64_t kBurstSpecAll = ~0ull;               // BurstSpectraParams::only: every burst

// One burst's summary as the kernels store it: ookd_burst_spectrum
struct BurstSpecSummary {
    uint64_t frames;
    double total, dc, peak;
    uint32_t peak_bin, reserved;
};
static_assert(sizeof(BurstSpecSummary) == 40, "ookd_burst_spectrum");

struct BurstSpectraParams {
    const BurstDev *table;          // the capture's entries
    uint64_t num_bursts;
    uint64_t total;                 // samples of the cut
    const void *src;                // the capture's first sample
    uint64_t n;                     // samples of it that exist: nothing at or beyond is read
    uint32_t sample_fmt;            // kFmt*
    uint32_t span_frames;           // S
    uint64_t spans;                 // ceil(total / (1024 S)): rows holds 2 * spans rows, keyed_rows spans rows
    uint64_t only;                  // kBurstSpecAll, or the one burst whose 1024 doubles go to `one`
    const float2 *twiddle;          // SpectrumParams' tables
    const float *window;
    double *rows;                   // [2 spans][1024]: row 2 g for the burst that began before span g, 2 g + 1 for the
                                    // one that begins in it and runs on
    double *keyed_rows;             // [spans][1024]: all a workgroup summed (not written with `only`)
    BurstSpecSummary *summary;      // [num_bursts], zero at launch (a burst of no frames stays zero)
    double *keyed;                  // [1024], zero at launch
    double *one;                    // [1024], zero at launch (with `only`)
};

// spans a cut of `total` samples has at span S
inline uint64_t burst_spec_spans(uint64_t total, uint32_t S) {
    const uint64_t w = (uint64_t)S * kSpecBins;
    return total / w + (total % w ? 1u : 0u);
}

// The first kernel, then (for the bursts across spans) the second, then -- without `only` -- the keyed sum.  `mid`,
// when not null, is recorded between the first kernel and the rest.  Nothing to launch for spans = 0.
hipError_t launch_burst_spectra(const BurstSpectraParams &p, hipEvent_t mid, hipStream_t stream);
// The same kernels over burst p.only alone, whose frames lie in spans [first_span, first_span + num_spans): its 1024
// doubles go to p.one.  Nothing to launch for num_spans = 0 (a burst of no frames).
hipError_t launch_burst_spectrum_one(const BurstSpectraParams &p, uint64_t first_span, uint64_t num_spans, hipStream_t stream);

}  // namespace ookd
