// survey.hip -- envelope survey: histogram of the post-filter power of whole captures (gfx950, wave64).
//
//   unpack (complexf.h:68-77) -> FIR stages in the reference's order (fir.c:302-395: taps newest first,
//   a separately rounded multiply and add per tap, stage s+1 fed by the decimated output of stage s)
//   -> p = re*re + im*im (complexf.h:43-46) -> bin (kernels.hpp: level_bin_of_bits) -> count.
//
// The filter is fir_generic_kernel's (kernels.hip) with another epilogue: one workgroup of four waves takes
// tiles of `tile` final outputs, builds the slice of every level a tile needs in LDS, ping-ponging between two
// buffers, and bins the last level instead of slicing it.  The taps are copied to LDS once per workgroup and read
// from there (one broadcast read per tap).  Only outputs 0 .. floor(n / D) - 1 exist, so no
// input at or beyond n is ever read: nothing is padded.  Inputs in front of the capture are the zero history.
//
// Counting.  Every wave owns a 256-counter histogram in LDS.  A wave first aggregates its 64 bins among the
// lanes: up to kPeelRounds times the lowest lane still to be counted broadcasts its bin, a ballot finds every
// lane with the same bin, and that one lane adds the popcount -- a capture that is mostly silence or mostly
// carrier is counted in one or two rounds whatever the lane count.  What is left after the rounds (the tail of
// a noisy wave, spread over many bins) goes to the wave's counters as single LDS adds, which then rarely
// collide.  A workgroup walks many tiles and flushes once at its end: 256 lanes sum the four waves' counters
// and issue one 64-bit vector atomic per non-zero bin to the capture's histogram in HBM.
//
// survey_kernel<FMT, TUNED>: TUNED = false is the above.  TUNED = true is the tuned survey for any shape
// (OOKD_SURVEY_TUNED_GENERIC): the same walk with complex taps -- (re, im) pairs in LDS -- and the tuned contract's
// four statements per tap (tuned_step, front_dev.hpp); a tuned survey always has a filter.  The register-blocked
// tuned form is in survey_tuned.hip.
//
// Compiled with -ffp-contract=off like every kernel of the library.
#include "kernels.hpp"
#include "common.hpp"
#include "survey_dev.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr int kSurveyThreads = 256;
constexpr int kSurveyWaves = kSurveyThreads / 64;
constexpr uint64_t kMaxTilesPerGroup = 1ull << 20;  // x 1024 outputs: a 32-bit LDS counter cannot wrap

template <int FMT, bool TUNED>
__global__ __launch_bounds__(kSurveyThreads) void survey_kernel(const SurveyParams p, const float *ctaps) {
    typedef typename std::conditional<TUNED, float2, float>::type tap_t;    // one tap in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // one LDS base and offsets from it (a pointer picked from an array would be a generic one: flat loads)
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem_raw + p.lds_hist_off);
    tap_t *ltaps = reinterpret_cast<tap_t *>(smem_raw + p.lds_taps_off);

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)p.num_stages;
    uint32_t *wave_hist = hist + (tid >> 6) * kLevelBins;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);

    for (uint32_t i = tid; i < (uint32_t)(kSurveyWaves * kLevelBins); i += kSurveyThreads) hist[i] = 0u;
    for (uint32_t i = tid; i < p.num_taps; i += kSurveyThreads) {
        if constexpr (TUNED) ltaps[i] = make_float2(ctaps[2 * i], ctaps[2 * i + 1]);
        else ltaps[i] = p.taps[i];
    }
    __syncthreads();

    for (uint64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t j0 = (int64_t)(tile * p.tile);
        const uint64_t left = p.n_out - (uint64_t)j0;
        const uint32_t len = left < p.tile ? (uint32_t)left : p.tile;
        if (!TUNED && S == 0) {         // the samples themselves
            for (uint32_t base = 0; base < len; base += kSurveyThreads) {
                const uint32_t i = base + tid;
                const bool valid = i < len;
                uint32_t bin = 0;
                if (valid) {
                    const float2 x = survey_sample<FMT>(src, j0 + (int64_t)i);
                    bin = survey_bin(x.x, x.y);
                }
                wave_count(wave_hist, valid, bin);
            }
            continue;
        }
        int64_t a[kMaxStages + 1];
        uint32_t n[kMaxStages + 1];
        survey_levels(p, j0, len, a, n);
        // level 0: index a[0] + n[0] - 1 = D (j0 + len) - 1 < D n_out <= samples in the capture
        for (uint32_t i = tid; i < n[0]; i += kSurveyThreads) {
            const int64_t g = a[0] + (int64_t)i;
            lds[i] = g < 0 ? make_float2(0.0f, 0.0f) : survey_sample<FMT>(src, g);
        }
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const float2 *in = lds + ((s & 1) ? p.lds_b_off : 0u);
            float2 *out = lds + ((s & 1) ? 0u : p.lds_b_off);
            const tap_t *taps = ltaps + p.stage[s].tap_off;
            const int64_t D = p.stage[s].decim;
            const uint32_t T = p.stage[s].ntaps;
            const bool last = (s == S - 1);
            const uint32_t cnt = n[s + 1];
            for (uint32_t base = 0; base < cnt; base += kSurveyThreads) {
                const uint32_t i = base + tid;
                const bool valid = i < cnt;
                float re = 0.0f, im = 0.0f;
                if (valid) {
                    // output a[s+1] + i reads level-s inputs D (a[s+1] + i) + D - 1 - k
                    // (= D i + T - 1 within the slice: the oldest input read is D i >= 0)
                    const float2 *x0 = in + ((uint32_t)D * i + T - 1u);
#pragma unroll 4
                    for (uint32_t k = 0; k < T; ++k) {
                        if constexpr (TUNED) {
                            const float2 c = taps[k];
                            tuned_step(re, im, c.x, c.y, x0[-(int)k]);
                        } else {
                            const float2 x = x0[-(int)k];
                            const float t = taps[k];
                            const float pr = t * x.x;
                            const float pi = t * x.y;
                            re = re + pr;
                            im = im + pi;
                        }
                    }
                }
                if (!last) {
                    // outputs in front of the capture do not exist: the next stage's history is zero there
                    if (valid) out[i] = (a[s + 1] + (int64_t)i) < 0 ? make_float2(0.0f, 0.0f) : make_float2(re, im);
                } else {
                    wave_count(wave_hist, valid, valid ? survey_bin(re, im) : 0u);
                }
            }
            __syncthreads();
        }
    }

    __syncthreads();
    {
        uint32_t sum = 0;
        for (int w = 0; w < kSurveyWaves; ++w) sum += hist[w * kLevelBins + tid];
        if (sum) atomicAdd(p.hist + (uint64_t)cap * kLevelBins + tid, (unsigned long long)sum);
    }
}

}  // namespace

uint32_t survey_tile(SurveyParams &p, size_t *lds_bytes, uint32_t tap_floats) {
    const size_t hist_bytes = (size_t)kSurveyWaves * kLevelBins * sizeof(uint32_t);
    uint64_t num_taps = 0;
    for (uint32_t s = 0; s < p.num_stages; ++s) num_taps += p.stage[s].ntaps;
    if (num_taps * tap_floats * sizeof(float) > kSurveyLdsBudget) return 0;
    const size_t taps_bytes = (size_t)((num_taps * tap_floats + 3) & ~3ull) * sizeof(float);
    for (uint32_t tile = 1024; tile >= 1; tile >>= 1) {
        int64_t a[kMaxStages + 1];
        uint32_t n[kMaxStages + 1];
        uint64_t even = 0, odd = 0;
        bool fits = true;
        if (p.num_stages) {
            // lengths in 64 bits first: a deep decimation chain can overflow survey_levels' 32-bit ones
            uint64_t len = tile;
            for (int s = (int)p.num_stages - 1; s >= 0 && fits; --s) {
                len = (uint64_t)p.stage[s].decim * (len - 1) + p.stage[s].ntaps;
                fits = len * sizeof(float2) <= kSurveyLdsBudget;
            }
            if (!fits) continue;
            survey_levels(p, 0, tile, a, n);
            for (uint32_t s = 0; s <= p.num_stages; ++s) {
                uint64_t &m = (s & 1) ? odd : even;
                if (n[s] > m) m = n[s];
            }
        }
        even = (even + 1) & ~1ull;      // keeps the second buffer and the histograms 16-byte aligned
        odd = (odd + 1) & ~1ull;
        const size_t total = (size_t)(even + odd) * sizeof(float2) + hist_bytes + taps_bytes;
        if (total > kSurveyLdsBudget) continue;
        p.tile = tile;
        p.lds_b_off = (uint32_t)even;
        p.lds_hist_off = (uint32_t)((even + odd) * sizeof(float2));
        p.lds_taps_off = p.lds_hist_off + (uint32_t)hist_bytes;
        p.num_taps = (uint32_t)num_taps;
        if (lds_bytes) *lds_bytes = total;
        return tile;
    }
    return 0;
}

uint32_t survey_tile_lag(SurveyParams &p, size_t *lds_bytes, uint32_t tap_floats, size_t table_bytes) {
    uint64_t num_taps = 0;
    for (uint32_t s = 0; s < p.num_stages; ++s) num_taps += p.stage[s].ntaps;
    if (num_taps * tap_floats * sizeof(float) > kSurveyLdsBudget) return 0;
    const size_t taps_bytes = (size_t)((num_taps * tap_floats + 3) & ~3ull) * sizeof(float);
    table_bytes = (table_bytes + 15u) & ~(size_t)15u;
    for (uint32_t tile = 1024; tile >= 1; tile >>= 1) {
        int64_t a[kMaxStages + 1];
        uint32_t n[kMaxStages + 1];
        uint64_t even = 0, odd = 0;
        bool fits = true;
        if (p.num_stages) {
            // tile + 1 outputs: the one in front of the tile, which the first lag product reads
            uint64_t len = (uint64_t)tile + 1u;
            for (int s = (int)p.num_stages - 1; s >= 0 && fits; --s) {
                len = (uint64_t)p.stage[s].decim * (len - 1) + p.stage[s].ntaps;
                fits = len * sizeof(float2) <= kSurveyLdsBudget;
            }
            if (!fits) continue;
            survey_levels(p, 0, tile + 1u, a, n);
            for (uint32_t s = 0; s <= p.num_stages; ++s) {      // (the last level is kept as well: s = num_stages)
                uint64_t &m = (s & 1) ? odd : even;
                if (n[s] > m) m = n[s];
            }
        }
        even = (even + 1) & ~1ull;
        odd = (odd + 1) & ~1ull;
        const size_t total = (size_t)(even + odd) * sizeof(float2) + table_bytes + taps_bytes;
        if (total > kSurveyLdsBudget) continue;
        p.tile = tile;
        p.lds_b_off = (uint32_t)even;
        p.lds_hist_off = (uint32_t)((even + odd) * sizeof(float2));
        p.lds_taps_off = p.lds_hist_off + (uint32_t)table_bytes;
        p.num_taps = (uint32_t)num_taps;
        if (lds_bytes) *lds_bytes = total;
        return tile;
    }
    return 0;
}

hipError_t survey_device_cus(int *cus) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    return e != hipSuccess ? e : hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
}

template <bool TUNED>
static const void *survey_kernel_of(uint32_t fmt) {
    switch (fmt) {
    case kFmtSc16: return reinterpret_cast<const void *>(&survey_kernel<(int)kFmtSc16, TUNED>);
    case kFmtCs8: return reinterpret_cast<const void *>(&survey_kernel<(int)kFmtCs8, TUNED>);
    case kFmtCu8: return reinterpret_cast<const void *>(&survey_kernel<(int)kFmtCu8, TUNED>);
    default: return nullptr;
    }
}

hipError_t launch_survey(const SurveyParams &p, const float *ctaps, uint32_t num_captures, size_t lds_bytes,
                         hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    if (ctaps && p.num_stages == 0) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    // as many workgroups as fit the device at once, each walking its share of the tiles and flushing once
    uint64_t per_cu = (160 * 1024) / lds_bytes;
    if (per_cu > 2048 / kSurveyThreads) per_cu = 2048 / kSurveyThreads;
    if (per_cu < 1) per_cu = 1;
    uint64_t gx = ((uint64_t)cus * per_cu + num_captures - 1) / num_captures;
    const uint64_t least = (p.num_tiles + kMaxTilesPerGroup - 1) / kMaxTilesPerGroup;
    if (gx < least) gx = least;
    if (gx > p.num_tiles) gx = p.num_tiles;
    if (gx > 0x7fffffffull || num_captures > 65535u) return hipErrorInvalidValue;
    const void *fn = ctaps ? survey_kernel_of<true>(p.sample_fmt) : survey_kernel_of<false>(p.sample_fmt);
    if (!fn) return hipErrorInvalidValue;
    SurveyParams pp = p;
    void *args[] = {&pp, &ctaps};
    e = hipLaunchKernel(fn, dim3((uint32_t)gx, num_captures), dim3(kSurveyThreads), args, lds_bytes, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace ookd
