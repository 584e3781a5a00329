// front_plan.hpp -- the front end of an rx context as its creation arguments decide it: taps, bands, bounds
// and the kernel that runs.  Pure host code (front_plan.cpp makes no HIP runtime call); rx.cpp uploads a plan
// once (FrontDev) and reads everything about the front end from it.
#pragma once

#include <cmath>

#include "common.hpp"
#include "kernels.hpp"

namespace ookd {

// Whether the filter takes the matrix cores (fir_mfma.hip), and when it stays on the packed-VALU loop, why.
// None of these is a failure.
enum class MfmaUse : uint32_t {
    kTaken = 0,
    kNotConsidered,     // no filter, OOKD_RX_EXACT_FIR, or a tuned / carrier context
    kValuAsked,         // OOKD_RX_FIR_VALU / OOKD_FIR_VALU
    kShape,             // neither 1 stage x decimation 1 (<= 256 taps) nor the folded 2 x decimate-by-2, or taps the split refuses
    kBandScale,         // a band edge leaves the normal floats in accumulator units (mfma_scale_band)
    kThresholdRange,    // p_star outside [2^-100, 2^100]
};

// One carrier of a tuned (one record) or carrier context (fir_tuned.hip)
struct CarrierPlan {
    double nu = 0.0;
    float threshold = 0, p_star = 0, p_lo = 0, p_hi = 0, quiet_a = INFINITY, quiet_b = INFINITY;
    double err_valu = 0.0;
    uint32_t tap_off = 0;       // floats from the start of ctaps to this carrier's image
};

struct FrontPlan {
    // Every FrontParams field that is constant for the life of a context: stages, p_star and bands, quiet_lsb,
    // the matrix-core scale / bands / grid shape, sample format, tune mode, a tuned context's quiet weights.
    // Pointers are null; FrontDev::upload fills its copy with the device addresses of the images below.
    FrontParams fp{};
    uint32_t total_decim = 1;
    uint64_t halo_needed = 0;
    bool exact = false;
    std::vector<float> taps;            // all stages' real taps, stage s at tap_off, zero padded to ntaps_pad
    // matrix-core form: ksteps and delta are the split's even where it was refused after the split (front_info
    // reports them); the image is empty unless mfma_use == kTaken
    MfmaTaps mfma;
    MfmaUse mfma_use = MfmaUse::kNotConsidered;
    // forward bounds the bands were built from, per component, output units (err_valu: of an untuned context;
    // a carrier's is in its record)
    double err_n = 0, err_w = 0, err_valu = 0;
    // A context tuned to nu != 0 is one record and no table; a carrier context K records, their taps one after
    // the other in ctaps (each in the layout of `taps`, as (re, im) pairs) and the fused kernel's table.
    std::vector<CarrierPlan> carriers;
    std::vector<float> ctaps;
    std::vector<TunedCarrierDev> carrier_tab;
    // what launch_front / launch_carriers run for this plan: OOKD_FRONT_* as a run reports it, the bits per
    // wave tile (0 = a generic kernel) and whether that kernel honours FrontParams::sparse
    uint32_t form = 0, tile_bits = 0;
    bool sparse_capable = false;
    uint32_t gen_tile = 0;      // final outputs per workgroup of a generic form (generic_tile), 0 for every other form

    bool carrier_context() const { return !carrier_tab.empty(); }
};

// filter: null = none.  nu != 0: a tuned context; num_carriers != 0: a carrier context (nu is ignored).
// false: the arguments are refused, error text set.
bool plan_front(uint32_t flags, float threshold, const ookd_filter *filter, double nu, const ookd_rx_carrier *carriers,
                uint32_t num_carriers, FrontPlan &out);

// A filter the generic kernels serve must leave room for their smallest tile (generic_tile, kernels.hpp).  false:
// it does not; the error text (starting with `who`) names the total decimation, the tap counts and the limit.
bool generic_tile_fits(const FirStageDev *stage, uint32_t num_stages, const char *who);

// ookd_rx_get_front_info / ookd_rx_get_carrier_front_info (k: the carrier, 0 without carriers)
ookd_front_info front_info(const FrontPlan &plan, uint32_t k);

inline uint64_t fnv1a(uint64_t h, const void *data, size_t bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

}  // namespace ookd

// Test aid, not in the public header: plan_front without a device.
struct ookd_front_plan_digest_out {
    uint32_t num_records;               // carriers, 1 for every other context
    uint32_t form, tile_bits, sparse_capable, mfma_g, mfma_xcd;
    int32_t quiet_lsb;
    uint32_t mfma_use;
    uint32_t band_bits[4];              // p_lo_n, p_hi_n, p_lo_w, p_hi_w as bit patterns
    uint64_t image_fnv[4];              // 64-bit FNV-1a of the real taps, the A-fragment image, the complex taps, the carrier table
    ookd_front_info info[OOKD_RX_MAX_CARRIERS];
    uint32_t quiet_bits[OOKD_RX_MAX_CARRIERS][2];       // quiet_a, quiet_b as bit patterns
    uint32_t gen_tile;                  // the generic kernels' tile for this filter, 0 when another kernel runs
};
extern "C" int ookd_front_plan_digest(uint32_t flags, float threshold, const ookd_filter *filter, double nu,
                                      const ookd_rx_carrier *carriers, uint32_t num_carriers,
                                      ookd_front_plan_digest_out *out);
