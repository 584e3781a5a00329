// burst_baseband.hip -- burst basebands: the filter's complex output over every burst of a burst table, densely
// packed per burst (gfx950, wave64; the contract is in include/ookiedokie_amd.h, the design in DESIGN.md 4.25).
//
// The walk is run_levels.hip's: the survey's tiles (survey_tile: the same LDS geometry), 64 tiles asked per ballot,
// only the tiles that hold an output of a burst are filtered, the same arithmetic as survey_kernel so that y is the
// survey contract's bit for bit.  What differs is the question a tile asks and what it does with its last level.
//
// The question goes to the baseband table, not to the edge list: a small kernel derives it from the burst table on
// the device, one thread per entry -- {first_output, end_output, offset}, the ceil-divisions by D done once.  Bursts
// ascend and never overlap (touching would do), so "the first burst that ends behind output j" is a binary search; a
// workgroup finds its chunk's range of bursts that way, a lane its tile's range inside the chunk's, and an output its
// burst inside the tile's.  Bursts without outputs all sit at ceil(n / D), behind every burst that has some, so the
// first burst that ends behind a tile's first output decides whether the tile is filtered.
//
// The epilogue needs no scan and no atomic: output j of burst b goes to out[offset_b + j - first_output_b], straight
// from the registers of the last stage -- one 8-byte store (CF32) or one 4-byte store (SC16Q11) per lane,
// neighbouring lanes to neighbouring elements inside a burst.  Outputs of a filtered tile that lie in no burst are
// computed and dropped; nothing at or beyond `total` is written.  Every element has exactly one writer, so no
// workgroup waits for another and two calls leave the same bytes.
//
// Inputs in front of the capture are the zero history; inputs at or beyond n_valid are the zero padding to whole
// buffers and are never loaded.  All positions are 64-bit.  Compiled with -ffp-contract=off like every kernel of the
// library.
#include "burst_baseband.hpp"
#include "common.hpp"
#include "run_tiles_dev.hpp"
#include "survey_dev.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr int kBasebandThreads = kRunLevelThreads;

// first index in [lo, hi) whose burst ends behind `pos` (end_output > pos)
__device__ __forceinline__ uint64_t burst_search(const BasebandDev *table, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (table[mid].end_output <= pos) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The bursts of [lo, hi) that outputs [j0, j0 + len) can meet: [b_lo, b_hi) -- b_lo the first burst that ends behind
// j0, b_hi the first at or behind it that begins at or beyond j0 + len.  -> the span holds an output of a burst.
__device__ __forceinline__ bool span_bursts(const BasebandDev *table, uint64_t lo, uint64_t hi, uint64_t j0, uint64_t len,
                                            uint64_t &b_lo, uint64_t &b_hi) {
    b_lo = burst_search(table, lo, hi, j0);
    b_hi = b_lo;
    if (b_lo >= hi) return false;
    const BasebandDev first = table[b_lo];
    if (first.first_output >= j0 + len || first.end_output <= first.first_output) return false;
    // (a burst that ends at or behind the span's last output ends the range)
    b_hi = burst_search(table, b_lo, hi, j0 + len - 1u);
    if (b_hi < hi && table[b_hi].first_output < j0 + len) ++b_hi;
    return true;
}

template <uint32_t FORMAT>
__device__ __forceinline__ void store_output(const BasebandParams &p, uint64_t b_lo, uint64_t b_hi, uint64_t j, float re, float im) {
    const uint64_t b = burst_search(p.table, b_lo, b_hi, j);
    if (b >= b_hi) return;
    const BasebandDev e = p.table[b];
    if (j < e.first_output) return;
    const uint64_t at = e.offset + (j - e.first_output);
    if (at >= p.total) return;
    if constexpr (FORMAT == kBasebandCf32) {
        reinterpret_cast<float2 *>(p.out)[at] = make_float2(re, im);
    } else {
        const uint32_t lo = (uint32_t)baseband_q16(re) & 0xffffu, hi = (uint32_t)baseband_q16(im) & 0xffffu;
        reinterpret_cast<uint32_t *>(p.out)[at] = lo | (hi << 16);
    }
}

template <int FMT, bool TUNED, uint32_t FORMAT>
__global__ __launch_bounds__(kBasebandThreads) void burst_baseband_kernel(const BasebandParams p) {
    typedef typename std::conditional<TUNED, float2, float>::type tap_t;    // one tap in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SurveyParams &sv = p.sv;
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    tap_t *ltaps = reinterpret_cast<tap_t *>(smem_raw + sv.lds_taps_off);

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = p.capture + blockIdx.y;
    const int S = (int)sv.num_stages;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(sv.iq) +
                               (uint64_t)(p.one_source ? 0u : cap) * sv.cap_stride * sample_bytes((uint32_t)FMT);
    const int64_t n_valid = (int64_t)p.n_valid;

    for (uint32_t i = tid; i < sv.num_taps; i += kBasebandThreads) {
        if constexpr (TUNED) {
            const float *ct = p.ctaps + (size_t)cap * p.ctap_floats;
            ltaps[i] = make_float2(ct[2 * i], ct[2 * i + 1]);
        } else {
            ltaps[i] = sv.taps[i];
        }
    }
    uint32_t filtered = 0;
    __syncthreads();

    // (the ballot over 64 neighbouring tiles: run_levels_kernel)
    const uint64_t num_chunks = (sv.num_tiles + 63u) / 64u;
    uint64_t behind = 0;                    // the bursts in front of it end at or below the chunks this workgroup has walked
    for (uint64_t chunk = blockIdx.x; chunk < num_chunks; chunk += gridDim.x) {
        // The whole table is searched once per chunk, uniformly -- two searches of log2(bursts) dependent loads, where
        // the edge list has its block prefix --; the 64 lanes and the tiles then search the chunk's few bursts.
        uint64_t c_lo, c_hi;
        if (!span_bursts(p.table, behind, p.num_bursts, chunk * 64u * sv.tile, 64ull * sv.tile, c_lo, c_hi)) {
            behind = c_lo;
            continue;
        }
        behind = c_lo;
        uint64_t m_lo, m_hi;
        const uint64_t my_tile = chunk * 64u + (tid & 63u);
        uint64_t todo = __ballot(my_tile < sv.num_tiles &&
                                 span_bursts(p.table, c_lo, c_hi, my_tile * sv.tile, sv.tile, m_lo, m_hi));
        while (todo) {
            const uint64_t tile = chunk * 64u + (uint64_t)(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1u;
            const int64_t j0 = (int64_t)(tile * sv.tile);
            const uint64_t left = sv.n_out - (uint64_t)j0;
            const uint32_t len = left < sv.tile ? (uint32_t)left : sv.tile;
            // once more, uniform this time (run_levels_kernel says why)
            uint64_t b_lo, b_hi;
            (void)span_bursts(p.table, c_lo, c_hi, (uint64_t)j0, len, b_lo, b_hi);
            ++filtered;

            if (S == 0) {                   // the samples themselves
                for (uint32_t i = tid; i < len; i += kBasebandThreads) {
                    const int64_t j = j0 + (int64_t)i;
                    const float2 y = j < n_valid ? survey_sample<FMT>(src, j) : make_float2(0.0f, 0.0f);
                    store_output<FORMAT>(p, b_lo, b_hi, (uint64_t)j, y.x, y.y);
                }
            } else {
                int64_t a[kMaxStages + 1];
                uint32_t n[kMaxStages + 1];
                survey_levels(sv, j0, len, a, n);
                for (uint32_t i = tid; i < n[0]; i += kBasebandThreads) {
                    const int64_t g = a[0] + (int64_t)i;
                    lds[i] = (g < 0 || g >= n_valid) ? make_float2(0.0f, 0.0f) : survey_sample<FMT>(src, g);
                }
                __syncthreads();
                for (int s = 0; s < S; ++s) {
                    const float2 *in = lds + ((s & 1) ? sv.lds_b_off : 0u);
                    float2 *out = lds + ((s & 1) ? 0u : sv.lds_b_off);
                    const tap_t *taps = ltaps + sv.stage[s].tap_off;
                    const int64_t D = sv.stage[s].decim;
                    const uint32_t T = sv.stage[s].ntaps;
                    const bool last = (s == S - 1);
                    const uint32_t cnt = n[s + 1];
                    for (uint32_t i = tid; i < cnt; i += kBasebandThreads) {
                        float re = 0.0f, im = 0.0f;
                        // output a[s+1] + i reads level-s inputs D (a[s+1] + i) + D - 1 - k (survey_kernel's walk)
                        const float2 *x0 = in + ((uint32_t)D * i + T - 1u);
#pragma unroll 4
                        for (uint32_t k = 0; k < T; ++k) {
                            if constexpr (TUNED) {
                                const float2 c = taps[k];
                                tuned_step(re, im, c.x, c.y, x0[-(int)k]);
                            } else {
                                const float2 x = x0[-(int)k];
                                const float tk = taps[k];
                                const float pr = tk * x.x;
                                const float pi = tk * x.y;
                                re = re + pr;
                                im = im + pi;
                            }
                        }
                        if (!last) {
                            // outputs in front of the capture do not exist: the next stage's history is zero there
                            out[i] = (a[s + 1] + (int64_t)i) < 0 ? make_float2(0.0f, 0.0f) : make_float2(re, im);
                        } else {
                            store_output<FORMAT>(p, b_lo, b_hi, (uint64_t)j0 + i, re, im);
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
    if (filtered) {
        // (every lane counted the same tiles)
        if (tid == 0) atomicAdd(&p.result[0], (unsigned long long)filtered);
    }
}

__global__ __launch_bounds__(256) void baseband_table_kernel(const BurstDev *table, uint64_t num_bursts, uint64_t D, BasebandDev *out) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= num_bursts) return;
    const BurstDev e = table[b];
    BasebandDev o;
    o.first_output = baseband_ceil(e.first_sample, D);
    o.end_output = baseband_ceil(e.first_sample + (e.end_offset - e.offset), D);
    o.offset = baseband_ceil(e.offset, D);      // (of a burst with outputs: every burst in front of it is whole)
    out[b] = o;
}

template <bool TUNED, uint32_t FORMAT>
const void *baseband_kernel_of(uint32_t fmt) {
    switch (fmt) {
    case kFmtSc16: return reinterpret_cast<const void *>(&burst_baseband_kernel<(int)kFmtSc16, TUNED, FORMAT>);
    case kFmtCs8: return reinterpret_cast<const void *>(&burst_baseband_kernel<(int)kFmtCs8, TUNED, FORMAT>);
    case kFmtCu8: return reinterpret_cast<const void *>(&burst_baseband_kernel<(int)kFmtCu8, TUNED, FORMAT>);
    default: return nullptr;
    }
}

}  // namespace

hipError_t launch_baseband_table(const BurstDev *table, uint64_t num_bursts, uint64_t D, BasebandDev *out, hipStream_t stream) {
    if (num_bursts == 0) return hipSuccess;
    if (!table || !out || D == 0 || num_bursts > 256ull * 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(baseband_table_kernel, dim3((uint32_t)((num_bursts + 255u) / 256u)), dim3(256), 0, stream, table,
                       num_bursts, D, out);
    return hipGetLastError();
}

hipError_t launch_burst_baseband(const BasebandParams &p, size_t lds_bytes, hipStream_t stream) {
    if (p.sv.num_tiles == 0 || p.total == 0 || p.num_bursts == 0) return hipSuccess;
    if ((p.ctaps && p.sv.num_stages == 0) || !p.table || !p.out || !p.result) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    // as many workgroups as fit the device at once, each walking its share of the tiles (launch_run_moments' sizing)
    uint64_t per_cu = (160 * 1024) / (lds_bytes ? lds_bytes : 1);
    if (per_cu > 2048 / kBasebandThreads) per_cu = 2048 / kBasebandThreads;
    if (per_cu < 1) per_cu = 1;
    uint64_t gx = (uint64_t)cus * per_cu;
    const uint64_t chunks = (p.sv.num_tiles + 63u) / 64u;       // a workgroup takes 64 tiles at a time
    if (gx > chunks) gx = chunks;
    if (gx < 1) gx = 1;
    const bool sc16 = p.format == kBasebandSc16;
    if (!sc16 && p.format != kBasebandCf32) return hipErrorInvalidValue;
    const void *fn = p.ctaps ? (sc16 ? baseband_kernel_of<true, kBasebandSc16>(p.sv.sample_fmt) : baseband_kernel_of<true, kBasebandCf32>(p.sv.sample_fmt))
                             : (sc16 ? baseband_kernel_of<false, kBasebandSc16>(p.sv.sample_fmt) : baseband_kernel_of<false, kBasebandCf32>(p.sv.sample_fmt));
    if (!fn) return hipErrorInvalidValue;
    BasebandParams pp = p;
    void *args[] = {&pp};
    return hipLaunchKernel(fn, dim3((uint32_t)gx, 1), dim3(kBasebandThreads), args, lds_bytes, stream);
}

}  // namespace ookd
