// run_levels.hip -- pulse levels: the peak power of every on-run of a finished run (gfx950, wave64; the contract is
// in include/ookiedokie_amd.h, the design in DESIGN.md 4.21).
//
// One sparse pass joins the run's edge list with the capture it came from.  The output axis is walked in the
// survey's tiles (survey_tile: the same LDS geometry, the same arithmetic as survey_kernel in survey.hip, so the
// powers are the survey contract's bit for bit).  A tile first asks the list whether any of its outputs is on: the
// block prefix gives the edges of its 4096-output block, two searches in them the edges inside the tile, and the
// parity of the capture's edges up to the tile's first output its level there.  A tile without an on output ends
// here -- on an OOK capture that is most of them, and the whole saving; the lanes of a wave ask for 64 tiles at once.
// Any other tile builds its levels in LDS and reduces the last one per on-run segment: a segmented maximum over the
// wave's lanes (the lanes of one run are neighbours), one LDS atomic per wave and segment into the tile's segment
// table, and from there ONE global atomicMax per segment and tile into peak[run].  A run that spans many tiles is
// met by many workgroups; the maximum of non-negative floats as uint32 patterns is exact and needs no order, so no
// workgroup waits for another.
//
// A second small kernel bins the peaks (wave_count, survey_dev.hpp).
//
// Inputs in front of the capture are the zero history; inputs at or beyond n_valid are the zero padding to whole
// buffers and are never loaded.  All positions are 64-bit.  Compiled with -ffp-contract=off like every kernel of the
// library.
#include "run_levels.hpp"
#include "common.hpp"
#include "run_tiles_dev.hpp"
#include "survey_dev.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace ookd {

namespace {

// Every wave calls this together with the power bits of its 64 neighbouring outputs (valid: the output exists).
__device__ __forceinline__ void segment_max(uint32_t *seg, const uint64_t *edges, const TileRuns &t, uint64_t lo_c,
                                            bool valid, uint64_t j, uint32_t bits) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t key = kNoSeg;
    if (valid) {
        // edges of the capture at or below j: odd = on, and then run (k - 1) / 2
        const uint64_t k = (t.t_hi == t.t_lo ? t.t_lo : edge_search<true>(edges, t.t_lo, t.t_hi, j)) - lo_c;
        if (k & 1ull) key = (uint32_t)(((k - 1u) >> 1) - (t.k1 >> 1));
    }
    uint32_t v = bits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ov = (uint32_t)__shfl_up((int)v, d);
        const uint32_t ok = (uint32_t)__shfl_up((int)key, d);
        if ((int)lane >= d && ok == key && ov > v) v = ov;
    }
    const uint32_t next = (uint32_t)__shfl_down((int)key, 1);
    if (key < t.nseg && (lane == 63u || next != key)) atomicMax(&seg[key], v);
}

template <int FMT, bool TUNED>
__global__ __launch_bounds__(kRunLevelThreads) void run_levels_kernel(const RunLevelParams p) {
    typedef typename std::conditional<TUNED, float2, float>::type tap_t;    // one tap in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SurveyParams &sv = p.sv;
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    uint32_t *seg = reinterpret_cast<uint32_t *>(smem_raw + sv.lds_hist_off);
    tap_t *ltaps = reinterpret_cast<tap_t *>(smem_raw + sv.lds_taps_off);

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)sv.num_stages;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(sv.iq) +
                               (uint64_t)(p.one_source ? 0u : cap) * sv.cap_stride * sample_bytes((uint32_t)FMT);
    const int64_t n_valid = (int64_t)p.n_valid;

    for (uint32_t i = tid; i < sv.num_taps; i += kRunLevelThreads) {
        if constexpr (TUNED) {
            const float *ct = p.ctaps + (size_t)cap * p.ctap_floats;
            ltaps[i] = make_float2(ct[2 * i], ct[2 * i + 1]);
        } else {
            ltaps[i] = sv.taps[i];
        }
    }

    const EdgeListView &list = p.list;
    const uint64_t total = edge_list_total(list);
    uint64_t lo_c, hi_c;
    edge_list_range(list, cap, total, lo_c, hi_c);
    const uint64_t peak_base = run_peak_base(lo_c, cap);
    const uint32_t *blk = list.blk_offset + (size_t)cap * list.blocks_per_cap;
    if (blockIdx.x == 0 && tid == 0) {
        p.result[(size_t)cap * kRunLevelWords + kRunLevelMetaWord] = hi_c - lo_c;
        p.result[(size_t)cap * kRunLevelWords + kRunLevelMetaWord + 2u] = lo_c;
    }
    uint32_t filtered = 0;
    __syncthreads();

    // 64 neighbouring tiles at a time: every lane asks the list about one of them (each of the four waves for itself:
    // the same loads, the same answer, so the mask is uniform over the workgroup without a barrier), and the workgroup
    // then walks the tiles that answered yes.  An empty stretch costs one look per 64 tiles, not 64.
    const uint64_t num_chunks = (sv.num_tiles + 63u) / 64u;
    for (uint64_t chunk = blockIdx.x; chunk < num_chunks; chunk += gridDim.x) {
        TileRuns mine;
        const uint64_t my_tile = chunk * 64u + (tid & 63u);
        uint64_t todo = __ballot(my_tile < sv.num_tiles &&
                                 tile_runs(list, blk, lo_c, hi_c, my_tile * sv.tile, sv.tile, mine));
        while (todo) {
            const uint64_t tile = chunk * 64u + (uint64_t)(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1u;
            const int64_t j0 = (int64_t)(tile * sv.tile);
            const uint64_t left = sv.n_out - (uint64_t)j0;
            const uint32_t len = left < sv.tile ? (uint32_t)left : sv.tile;
            // once more, uniform this time: scalar loads, and nothing of the 64 answers is kept in registers (handing
            // the asking lane's answer over through shuffles takes the kernel past 128 VGPRs, four waves per SIMD)
            TileRuns t;
            (void)tile_runs(list, blk, lo_c, hi_c, (uint64_t)j0, len, t);
            ++filtered;
            for (uint32_t i = tid; i < t.nseg; i += kRunLevelThreads) seg[i] = 0u;

            if (S == 0) {                   // the samples themselves
                __syncthreads();
                for (uint32_t base = 0; base < len; base += kRunLevelThreads) {
                    const uint32_t i = base + tid;
                    const bool valid = i < len;
                    const int64_t j = j0 + (int64_t)i;
                    uint32_t bits = 0u;
                    if (valid && j < n_valid) {
                        const float2 x = survey_sample<FMT>(src, j);
                        const float rr = x.x * x.x;
                        const float ii = x.y * x.y;
                        bits = __float_as_uint(rr + ii);
                    }
                    segment_max(seg, list.edges, t, lo_c, valid, (uint64_t)j, bits);
                }
                __syncthreads();
            } else {
                int64_t a[kMaxStages + 1];
                uint32_t n[kMaxStages + 1];
                survey_levels(sv, j0, len, a, n);
                for (uint32_t i = tid; i < n[0]; i += kRunLevelThreads) {
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
                    for (uint32_t base = 0; base < cnt; base += kRunLevelThreads) {
                        const uint32_t i = base + tid;
                        const bool valid = i < cnt;
                        float re = 0.0f, im = 0.0f;
                        if (valid) {
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
                        }
                        if (!last) {
                            // outputs in front of the capture do not exist: the next stage's history is zero there
                            if (valid) out[i] = (a[s + 1] + (int64_t)i) < 0 ? make_float2(0.0f, 0.0f) : make_float2(re, im);
                        } else {
                            const float rr = re * re;
                            const float ii = im * im;
                            segment_max(seg, list.edges, t, lo_c, valid, (uint64_t)j0 + i, __float_as_uint(rr + ii));
                        }
                    }
                    __syncthreads();
                }
            }
            // one atomic per segment of the tile (a lane zeroes only the table entries it flushed: no barrier behind this)
            for (uint32_t i = tid; i < t.nseg; i += kRunLevelThreads) {
                const uint32_t v = seg[i];
                const uint64_t slot = peak_base + (t.k1 >> 1) + i;
                // (a peak only grows: a run that many tiles share takes the atomic only from the tiles that raise it; a
                //  stale look costs one atomic that changes nothing)
                if (v && slot < p.peak_slots &&
                    __hip_atomic_load(&p.peaks[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) {
                    atomicMax(&p.peaks[slot], v);
                }
            }
        }
    }
    if (filtered) {
        // (every lane counted the same tiles)
        if (tid == 0) atomicAdd(&p.result[(size_t)cap * kRunLevelWords + kRunLevelMetaWord + 1u], (unsigned long long)filtered);
    }
}

// the histogram of capture blockIdx.y's peaks
__global__ __launch_bounds__(kRunLevelThreads) void run_level_hist_kernel(const RunLevelParams p) {
    __shared__ uint32_t hist[kRunLevelWaves * kLevelBins];
    const uint32_t tid = threadIdx.x, cap = blockIdx.y;
    for (uint32_t i = tid; i < (uint32_t)(kRunLevelWaves * kLevelBins); i += kRunLevelThreads) hist[i] = 0u;
    __syncthreads();
    const uint64_t total = edge_list_total(p.list);
    uint64_t lo_c, hi_c;
    edge_list_range(p.list, cap, total, lo_c, hi_c);
    const uint64_t runs = (hi_c - lo_c + 1u) >> 1;
    const uint64_t peak_base = run_peak_base(lo_c, cap);
    uint32_t *wave_hist = hist + (tid >> 6) * kLevelBins;
    for (uint64_t base = (uint64_t)blockIdx.x * kRunLevelThreads; base < runs; base += (uint64_t)gridDim.x * kRunLevelThreads) {
        const uint64_t r = base + tid;
        const bool valid = r < runs && peak_base + r < p.peak_slots;
        wave_count(wave_hist, valid, valid ? level_bin_of_bits(p.peaks[peak_base + r]) : 0u);
    }
    __syncthreads();
    uint32_t sum = 0;
    for (int w = 0; w < kRunLevelWaves; ++w) sum += hist[w * kLevelBins + tid];
    if (sum) atomicAdd(p.result + (size_t)cap * kRunLevelWords + tid, (unsigned long long)sum);
}

template <bool TUNED>
const void *run_levels_kernel_of(uint32_t fmt) {
    switch (fmt) {
    case kFmtSc16: return reinterpret_cast<const void *>(&run_levels_kernel<(int)kFmtSc16, TUNED>);
    case kFmtCs8: return reinterpret_cast<const void *>(&run_levels_kernel<(int)kFmtCs8, TUNED>);
    case kFmtCu8: return reinterpret_cast<const void *>(&run_levels_kernel<(int)kFmtCu8, TUNED>);
    default: return nullptr;
    }
}

}  // namespace

hipError_t launch_run_levels(const RunLevelParams &p, size_t lds_bytes, hipStream_t stream) {
    const uint32_t caps = p.list.num_captures;
    if (p.sv.num_tiles == 0 || caps == 0) return hipSuccess;
    if ((p.ctaps && p.sv.num_stages == 0) || caps > 65535u) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    // as many workgroups as fit the device at once, each walking its share of the tiles (launch_survey's sizing)
    uint64_t per_cu = (160 * 1024) / (lds_bytes ? lds_bytes : 1);
    if (per_cu > 2048 / kRunLevelThreads) per_cu = 2048 / kRunLevelThreads;
    if (per_cu < 1) per_cu = 1;
    uint64_t gx = ((uint64_t)cus * per_cu + caps - 1) / caps;
    const uint64_t chunks = (p.sv.num_tiles + 63u) / 64u;      // a workgroup takes 64 tiles at a time
    if (gx > chunks) gx = chunks;
    if (gx < 1) gx = 1;
    const void *fn = p.ctaps ? run_levels_kernel_of<true>(p.sv.sample_fmt) : run_levels_kernel_of<false>(p.sv.sample_fmt);
    if (!fn) return hipErrorInvalidValue;
    RunLevelParams pp = p;
    void *args[] = {&pp};
    e = hipLaunchKernel(fn, dim3((uint32_t)gx, caps), dim3(kRunLevelThreads), args, lds_bytes, stream);
    if (e != hipSuccess) return e;
    uint64_t hx = (p.peak_slots + 16u * kRunLevelThreads - 1) / (16u * kRunLevelThreads);
    if (hx > (uint64_t)cus * 4u) hx = (uint64_t)cus * 4u;
    if (hx < 1) hx = 1;
    hipLaunchKernelGGL(run_level_hist_kernel, dim3((uint32_t)hx, caps), dim3(kRunLevelThreads), 0, stream, pp);
    return hipGetLastError();
}

}  // namespace ookd
