// run_moments.hip -- pulse moments: the summed power and the summed lag-1 product of every on-run of a finished run
// (gfx950, wave64; the contract is in include/ookiedokie_amd.h, the design in DESIGN.md 4.23).
//
// The walk is run_levels.hip's: the survey's tiles, 64 tiles asked per ballot, only the tiles that hold an on output
// are filtered, the same arithmetic as survey_kernel so the filter's outputs are the survey contract's bit for bit.
// What differs is what a tile does with its last level.  It keeps the complex outputs y in the level buffer the last
// stage writes, and with them the output in front of the tile (survey_tile_lag sizes the buffers for tile + 1 outputs),
// so that every on output j that is not a rise finds y_{j-1}: the pair (j - 1, j) is counted by the tile that holds
// j, once.  Tile 0 of a capture computes no extra output; captures are blockIdx.y, so no pair crosses two of them.
//
// Per on output three int64 terms -- q(p_j), q(zr_j), q(zi_j), fixed point with 30 fraction bits -- are summed over
// the lanes of one run: a segmented inclusive scan over the wave's lanes with the run as the key (the lanes of one
// run are neighbours), then the segment's last lane adds the three sums to the tile's segment table in LDS, and from
// there ONE global 64-bit atomicAdd per sum, segment and tile goes to moments[run].  The table holds the tile's first
// kRunMomentTableSegs segments; a tile of chatter adds its later ones to global memory from every wave.  Integer sums
// need no order: a run that many workgroups share is exact whoever comes first, and no workgroup waits for another.
//
// Inputs in front of the capture are the zero history; inputs at or beyond n_valid are the zero padding to whole
// buffers and are never loaded.  All positions are 64-bit.  Compiled with -ffp-contract=off like every kernel of the
// library: the lag product keeps its two rounded products and its rounded sum.
#include "run_moments.hpp"
#include "common.hpp"
#include "run_tiles_dev.hpp"
#include "survey_dev.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr int kRunMomentThreads = kRunLevelThreads;

// Every wave calls this together: output j of the tile (valid: it exists) with its y and the output before it (which
// is read only when j is on and not a rise).  `seg`: the tile's table of table_segs x 3 sums; slot0: the global slot
// of the tile's segment 0.
__device__ __forceinline__ void segment_add(unsigned long long *seg, const RunMomentParams &p, const TileRuns &t,
                                            uint64_t lo_c, uint64_t slot0, bool valid, uint64_t j, float2 y, float2 yp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t *edges = p.list.edges;
    uint32_t key = kNoSeg;
    unsigned long long s0 = 0ull, s1 = 0ull, s2 = 0ull;
    if (valid) {
        // edges of the capture at or below j: odd = on, and then run (k - 1) / 2
        const uint64_t at = t.t_hi == t.t_lo ? t.t_lo : edge_search<true>(edges, t.t_lo, t.t_hi, j);
        const uint64_t k = at - lo_c;
        if (k & 1ull) {
            key = (uint32_t)(((k - 1u) >> 1) - (t.k1 >> 1));
            const float rr = y.x * y.x;
            const float ii = y.y * y.y;
            s0 = moment_q(rr + ii);
            if (edges[at - 1u] != j) {          // not the run's first output: the pair (j - 1, j) is this lane's
                const float a = y.x * yp.x;
                const float b = y.y * yp.y;
                const float c = y.y * yp.x;
                const float d = y.x * yp.y;
                s1 = moment_q(a + b);
                s2 = moment_q(c - d);
            }
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ok = (uint32_t)__shfl_up((int)key, d);
        const unsigned long long o0 = __shfl_up(s0, d);
        const unsigned long long o1 = __shfl_up(s1, d);
        const unsigned long long o2 = __shfl_up(s2, d);
        if ((int)lane >= d && ok == key) {
            s0 += o0;
            s1 += o1;
            s2 += o2;
        }
    }
    const uint32_t next = (uint32_t)__shfl_down((int)key, 1);
    if (key != kNoSeg && (lane == 63u || next != key)) {
        if (key < p.table_segs) {
            unsigned long long *to = seg + (size_t)key * kRunMomentSums;
            atomicAdd(&to[0], s0);
            if (s1) atomicAdd(&to[1], s1);
            if (s2) atomicAdd(&to[2], s2);
        } else {
            const uint64_t slot = slot0 + key;
            if (slot < p.slots) {
                unsigned long long *to = p.moments + slot * kRunMomentSums;
                if (s0) atomicAdd(&to[0], s0);
                if (s1) atomicAdd(&to[1], s1);
                if (s2) atomicAdd(&to[2], s2);
            }
        }
    }
}

template <int FMT, bool TUNED>
__global__ __launch_bounds__(kRunMomentThreads) void run_moments_kernel(const RunMomentParams p) {
    typedef typename std::conditional<TUNED, float2, float>::type tap_t;    // one tap in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SurveyParams &sv = p.sv;
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    unsigned long long *seg = reinterpret_cast<unsigned long long *>(smem_raw + sv.lds_hist_off);
    tap_t *ltaps = reinterpret_cast<tap_t *>(smem_raw + sv.lds_taps_off);

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)sv.num_stages;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(sv.iq) +
                               (uint64_t)(p.one_source ? 0u : cap) * sv.cap_stride * sample_bytes((uint32_t)FMT);
    const int64_t n_valid = (int64_t)p.n_valid;

    for (uint32_t i = tid; i < sv.num_taps; i += kRunMomentThreads) {
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
    const uint64_t base = run_peak_base(lo_c, cap);
    const uint32_t *blk = list.blk_offset + (size_t)cap * list.blocks_per_cap;
    if (blockIdx.x == 0 && tid == 0) {
        p.result[(size_t)cap * kRunMomentWords] = hi_c - lo_c;
        p.result[(size_t)cap * kRunMomentWords + 2u] = lo_c;
    }
    uint32_t filtered = 0;
    __syncthreads();

    // (the ballot over 64 neighbouring tiles: run_levels_kernel)
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
            TileRuns t;
            (void)tile_runs(list, blk, lo_c, hi_c, (uint64_t)j0, len, t);
            ++filtered;
            const uint32_t in_table = t.nseg < p.table_segs ? t.nseg : p.table_segs;
            const uint64_t slot0 = base + (t.k1 >> 1);
            for (uint32_t i = tid; i < in_table * kRunMomentSums; i += kRunMomentThreads) seg[i] = 0ull;

            if (S == 0) {                   // the samples themselves; the one before comes from memory again
                __syncthreads();
                for (uint32_t b = 0; b < len; b += kRunMomentThreads) {
                    const uint32_t i = b + tid;
                    const bool valid = i < len;
                    const int64_t j = j0 + (int64_t)i;
                    float2 y = make_float2(0.0f, 0.0f), yp = make_float2(0.0f, 0.0f);
                    if (valid) {
                        if (j < n_valid) y = survey_sample<FMT>(src, j);
                        if (j > 0 && j - 1 < n_valid) yp = survey_sample<FMT>(src, j - 1);
                    }
                    segment_add(seg, p, t, lo_c, slot0, valid, (uint64_t)j, y, yp);
                }
            } else {
                // outputs [j0 - ext, j0 + len): the one in front of the tile too, unless the capture begins here
                const uint32_t ext = j0 > 0 ? 1u : 0u;
                int64_t a[kMaxStages + 1];
                uint32_t n[kMaxStages + 1];
                survey_levels(sv, j0 - (int64_t)ext, len + ext, a, n);
                for (uint32_t i = tid; i < n[0]; i += kRunMomentThreads) {
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
                    const uint32_t cnt = n[s + 1];
                    for (uint32_t i = tid; i < cnt; i += kRunMomentThreads) {
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
                        // outputs in front of the capture do not exist: the next stage's history is zero there
                        out[i] = (a[s + 1] + (int64_t)i) < 0 ? make_float2(0.0f, 0.0f) : make_float2(re, im);
                    }
                    __syncthreads();
                }
                // the last level, in the buffer its stage wrote: y[ext + i] is output j0 + i
                const float2 *y = lds + (((S - 1) & 1) ? 0u : sv.lds_b_off);
                for (uint32_t b = 0; b < len; b += kRunMomentThreads) {
                    const uint32_t i = b + tid;
                    const bool valid = i < len;
                    float2 yj = make_float2(0.0f, 0.0f), yp = make_float2(0.0f, 0.0f);
                    if (valid) {
                        yj = y[ext + i];
                        if (ext + i > 0u) yp = y[ext + i - 1u];
                    }
                    segment_add(seg, p, t, lo_c, slot0, valid, (uint64_t)j0 + i, yj, yp);
                }
            }
            __syncthreads();                // the table is whole, and nobody reads the last level any more
            // one atomic per sum and segment of the tile (a lane zeroes the entries it flushes at the next tile's
            // start: no barrier behind this)
            for (uint32_t i = tid; i < in_table * kRunMomentSums; i += kRunMomentThreads) {
                const unsigned long long v = seg[i];
                const uint64_t slot = slot0 + i / kRunMomentSums;
                if (v && slot < p.slots) atomicAdd(&p.moments[slot * kRunMomentSums + i % kRunMomentSums], v);
            }
        }
    }
    if (filtered) {
        // (every lane counted the same tiles)
        if (tid == 0) atomicAdd(&p.result[(size_t)cap * kRunMomentWords + 1u], (unsigned long long)filtered);
    }
}

template <bool TUNED>
const void *run_moments_kernel_of(uint32_t fmt) {
    switch (fmt) {
    case kFmtSc16: return reinterpret_cast<const void *>(&run_moments_kernel<(int)kFmtSc16, TUNED>);
    case kFmtCs8: return reinterpret_cast<const void *>(&run_moments_kernel<(int)kFmtCs8, TUNED>);
    case kFmtCu8: return reinterpret_cast<const void *>(&run_moments_kernel<(int)kFmtCu8, TUNED>);
    default: return nullptr;
    }
}

}  // namespace

hipError_t launch_run_moments(const RunMomentParams &p, size_t lds_bytes, hipStream_t stream) {
    const uint32_t caps = p.list.num_captures;
    if (p.sv.num_tiles == 0 || caps == 0) return hipSuccess;
    if ((p.ctaps && p.sv.num_stages == 0) || caps > 65535u || p.table_segs > kRunMomentTableSegs) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    // as many workgroups as fit the device at once, each walking its share of the tiles (launch_run_levels' sizing)
    uint64_t per_cu = (160 * 1024) / (lds_bytes ? lds_bytes : 1);
    if (per_cu > 2048 / kRunMomentThreads) per_cu = 2048 / kRunMomentThreads;
    if (per_cu < 1) per_cu = 1;
    uint64_t gx = ((uint64_t)cus * per_cu + caps - 1) / caps;
    const uint64_t chunks = (p.sv.num_tiles + 63u) / 64u;      // a workgroup takes 64 tiles at a time
    if (gx > chunks) gx = chunks;
    if (gx < 1) gx = 1;
    const void *fn = p.ctaps ? run_moments_kernel_of<true>(p.sv.sample_fmt) : run_moments_kernel_of<false>(p.sv.sample_fmt);
    if (!fn) return hipErrorInvalidValue;
    RunMomentParams pp = p;
    void *args[] = {&pp};
    return hipLaunchKernel(fn, dim3((uint32_t)gx, caps), dim3(kRunMomentThreads), args, lds_bytes, stream);
}

}  // namespace ookd
