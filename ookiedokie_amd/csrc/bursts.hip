// bursts.hip -- burst extraction: the burst table of every capture's edge list, and the cut of one capture (the
// contract is in include/ookiedokie_amd.h, the design in DESIGN.md 4.22).
//
// 1. The table.  "Run r begins a burst" depends on run r and the one before it alone, but a burst's index and its
// offset in the cut are sums over everything in front of it: a scan along a capture's on-runs, done like clean.hip's
// in three dependent launches on one stream -- aggregates per tile, one workgroup that scans the aggregates, and the
// tiles once more with their carry-in, which write the table.  No workgroup ever waits for another inside a kernel.
// A tile is kBurstTile edges (kBurstTileRuns on-runs) of ONE capture, staged in LDS with plain 8-byte loads.
//
// The scan carries two sums.  The count of burst starts is the burst index.  The second is a sample count that
// telescopes: run r contributes [begin_r, end_r) input samples, begin_r = the burst's `first` at a burst start and
// min(n, f_{r-1} D) otherwise, end_r = the burst's `end` at a burst's last run and min(n, f_r D) otherwise -- the
// contributions of a burst's runs add up to its num_samples, and the sum in front of its first run is its offset.
//
// 2. The copy.  The grid runs over the cut in 16-byte vectors; a workgroup finds the bursts of its span's two ends by
// a search over `offset` and its lanes walk the table between them.  A vector inside one burst is one load (only
// sample-aligned) and one aligned store; every other vector goes sample by sample.
#include <type_traits>

#include "bursts.hpp"

namespace ookd {

namespace {

// a tile's edges in LDS: slot i holds edge base - 1 + i of the capture, i <= kBurstTile + 1 (the edge in front of the
// tile closes the run before its first, the edge behind it begins the run after its last).  One spare word per eight
// keeps the lanes' 64-byte strides off the same banks.
constexpr uint32_t kBurstTileEdges = kBurstTile + 2u;
__device__ __forceinline__ uint32_t edge_slot(uint32_t i) { return i + (i >> 3); }
constexpr uint32_t kBurstEdgeSlots = kBurstTileEdges + (kBurstTileEdges >> 3) + 1u;
constexpr uint32_t kBurstWaves = kBurstThreads / 64u;

// the capture that owns tile t of the run: (c, its range, its first tile, its tiles).  t only grows from call to call.
struct TileCursor {
    uint32_t c;
    uint64_t lo, hi;
    uint64_t tile0, tiles;
};
__device__ __forceinline__ uint64_t tiles_of(uint64_t lo, uint64_t hi) { return (hi - lo + kBurstTile - 1u) / kBurstTile; }

__device__ __forceinline__ TileCursor cursor_begin(const EdgeListView &v, uint64_t total) {
    TileCursor k;
    k.c = 0u;
    edge_list_range(v, 0u, total, k.lo, k.hi);
    k.tile0 = 0ull;
    k.tiles = tiles_of(k.lo, k.hi);
    return k;
}
// false: the run has no tile t
__device__ __forceinline__ bool cursor_seek(TileCursor &k, const EdgeListView &v, uint64_t total, uint64_t t) {
    while (t >= k.tile0 + k.tiles && k.c + 1u < v.num_captures) {
        ++k.c;
        k.tile0 += k.tiles;
        edge_list_range(v, k.c, total, k.lo, k.hi);
        k.tiles = tiles_of(k.lo, k.hi);
    }
    return t < k.tile0 + k.tiles;
}

// the tile's edges into LDS (the caller synchronises before and after); every load lies inside the capture's own list
__device__ __forceinline__ void stage_edges(uint64_t *edge, const EdgeListView &v, const TileCursor &k, uint64_t base) {
    const uint64_t E = k.hi - k.lo;
    for (uint32_t i = threadIdx.x; i < kBurstTileEdges; i += kBurstThreads) {
        const uint64_t el = base + i;           // (edge el - 1)
        edge[edge_slot(i)] = el >= 1u && el - 1u < E ? v.edges[k.lo + el - 1u] : 0ull;
    }
}

// This lane's runs base / 2 + kBurstRunsPerThread tid + q of a capture of E edges: bit q of `starts` / `lasts` = the
// run exists and begins / ends a burst; begin[q], end[q] = its contribution (equal for a run that does not exist).
struct LaneRuns {
    uint32_t starts, lasts;
    uint64_t begin[kBurstRunsPerThread], end[kBurstRunsPerThread];
};
__device__ __forceinline__ LaneRuns lane_runs(const uint64_t *edge, const BurstParams &p, uint64_t base, uint64_t E) {
    LaneRuns out;
    out.starts = out.lasts = 0u;
    const uint32_t j0 = 2u * kBurstRunsPerThread * threadIdx.x;     // this lane's first edge, from the tile's first
#pragma unroll
    for (uint32_t q = 0; q < kBurstRunsPerThread; ++q) {
        const uint32_t j = j0 + 2u * q;
        const uint64_t i = base + j;            // the run's rising edge in the capture
        out.begin[q] = out.end[q] = 0ull;
        if (i < E) {
            const uint64_t f_prev = edge[edge_slot(j)], a = edge[edge_slot(j + 1u)];
            const uint64_t f = i + 1u < E ? edge[edge_slot(j + 2u)] : p.n_out;
            const bool start = i == 0u || a - f_prev > p.max_gap;
            const bool last = i + 2u >= E || edge[edge_slot(j + 3u)] - f > p.max_gap;
            out.begin[q] = burst_scale(start ? a - (a < p.pre ? a : p.pre) : f_prev, p.D, p.n);
            out.end[q] = burst_scale(last ? burst_hi(f, p.post, p.n_out) : f, p.D, p.n);
            out.starts |= (start ? 1u : 0u) << q;
            out.lasts |= (last ? 1u : 0u) << q;
        }
    }
    return out;
}

// Workgroup-wide: leaves with the sum of the threads in front; `all` receives the workgroup's sum (uniform).  ws: LDS,
// one word per wave; the caller synchronises before it is used again.
__device__ __forceinline__ uint64_t block_sum_exclusive(uint64_t v, uint64_t *ws, uint64_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint64_t prev = (uint64_t)__shfl_up((unsigned long long)inc, s);
        if (lane >= s) inc += prev;
    }
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    uint64_t pre = 0ull;
    all = 0ull;
    for (uint32_t w = 0; w < kBurstWaves; ++w) {
        const uint64_t sw = ws[w];
        if (w < wave) pre += sw;
        all += sw;
    }
    return pre + inc - v;
}

}  // namespace

// ---- 1. every tile's aggregate ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kBurstThreads) void burst_agg_kernel(BurstParams p) {
    __shared__ uint64_t edge[kBurstEdgeSlots];
    __shared__ uint64_t ws[2][kBurstWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const EdgeListView &list = p.list;
    if (list.num_captures == 0u) return;
    const uint64_t total = edge_list_total(list);
    TileCursor cur = cursor_begin(list, total);

    for (uint64_t t = blockIdx.x; t < p.num_tiles_cap; t += gridDim.x) {
        if (!cursor_seek(cur, list, total, t)) break;           // (uniform)
        const uint64_t k = t - cur.tile0, base = k * kBurstTile, E = cur.hi - cur.lo;
        __syncthreads();
        stage_edges(edge, list, cur, base);
        __syncthreads();

        const LaneRuns r = lane_runs(edge, p, base, E);
        uint64_t samples = 0ull;
#pragma unroll
        for (uint32_t q = 0; q < kBurstRunsPerThread; ++q) samples += r.end[q] - r.begin[q];
        samples = wave_sum_u64(samples);
        const uint64_t starts = wave_sum_u64((uint64_t)__popc(r.starts));
        if (lane == 0u) {
            ws[0][wave] = samples;
            ws[1][wave] = starts;
        }
        __syncthreads();
        if (tid == 0u) {
            BurstAgg a;
            a.samples = 0ull;
            a.starts = 0u;
            for (uint32_t w = 0; w < kBurstWaves; ++w) {
                a.samples += ws[0][w];
                a.starts += (uint32_t)ws[1][w];
            }
            a.capture = cur.c | (k == 0u ? kBurstFirst : 0u) | (k + 1u == cur.tiles ? kBurstLast : 0u);
            p.agg[t] = a;
        }
    }
}

// ---- 2. one workgroup: the sums in front of every tile, every capture's counts ---------------------------------

__global__ __launch_bounds__(kBurstThreads) void burst_scan_kernel(BurstParams p) {
    __shared__ uint64_t ws[2][kBurstWaves];
    __shared__ unsigned long long t_tiles;
    const uint32_t tid = threadIdx.x;
    const EdgeListView &list = p.list;
    const uint64_t total = edge_list_total(list);
    if (tid == 0u) t_tiles = 0ull;
    __syncthreads();
    {
        unsigned long long mine = 0ull;
        for (uint32_t c = tid; c < list.num_captures; c += kBurstThreads) {
            uint64_t lo, hi;
            edge_list_range(list, c, total, lo, hi);
            mine += tiles_of(lo, hi);
        }
        if (mine) atomicAdd(&t_tiles, mine);
    }
    __syncthreads();
    const uint32_t tiles = (uint32_t)(t_tiles < p.num_tiles_cap ? t_tiles : p.num_tiles_cap);

    // A lane takes kBurstScanPerThread consecutive aggregates -- their loads are in flight together -- folds them, and
    // the workgroup scans the lanes' folds: one step covers 2048 tiles.  The sums run over all captures; a capture's
    // own begin goes into its result words and the third kernel takes the difference.
    uint64_t carry[2] = {0ull, 0ull};           // (uniform) samples, starts
    for (uint32_t chunk = 0; chunk < tiles; chunk += kBurstThreads * kBurstScanPerThread) {
        const uint32_t t0 = chunk + tid * kBurstScanPerThread;
        BurstAgg a[kBurstScanPerThread];
        uint64_t mine[2] = {0ull, 0ull};
#pragma unroll
        for (uint32_t j = 0; j < kBurstScanPerThread; ++j) {
            a[j] = BurstAgg{};
            if (t0 + j < tiles) a[j] = p.agg[t0 + j];
            mine[0] += a[j].samples;
            mine[1] += a[j].starts;
        }
        __syncthreads();
        uint64_t exc[2];
#pragma unroll
        for (uint32_t f = 0; f < 2u; ++f) {
            uint64_t sum;
            exc[f] = carry[f] + block_sum_exclusive(mine[f], ws[f], sum);
            carry[f] += sum;
        }
#pragma unroll
        for (uint32_t j = 0; j < kBurstScanPerThread; ++j) {
            if (t0 + j < tiles) {
                BurstCarry c;
                c.samples = exc[0];
                c.starts = exc[1];
                p.carry[t0 + j] = c;
                const uint32_t cap = a[j].capture & ~(kBurstFirst | kBurstLast);
                if (cap < list.num_captures) {
                    unsigned long long *r = p.result + (size_t)cap * kBurstWords;
                    if (a[j].capture & kBurstFirst) {
                        r[kBurstWordBegin] = exc[1];
                        r[kBurstWordBegin + 1u] = exc[0];
                    }
                    if (a[j].capture & kBurstLast) {            // (the sums behind the capture, until the second half)
                        r[kBurstWordCount] = exc[1] + a[j].starts;
                        r[kBurstWordTotal] = exc[0] + a[j].samples;
                    }
                }
            }
            exc[0] += a[j].samples;
            exc[1] += a[j].starts;
        }
    }
    __syncthreads();

    // the captures: their counts (a capture without an edge has no tile: its words are still zero)
    for (uint32_t c = tid; c < list.num_captures; c += kBurstThreads) {
        uint64_t lo, hi;
        edge_list_range(list, c, total, lo, hi);
        unsigned long long *r = p.result + (size_t)c * kBurstWords;
        r[kBurstWordCount] -= r[kBurstWordBegin];
        r[kBurstWordTotal] -= r[kBurstWordBegin + 1u];
        r[kBurstWordEdges] = hi - lo;
        r[kBurstWordLo] = lo;
    }
}

// ---- 3. every tile once more, with its carry-in: the table -----------------------------------------------------

__global__ __launch_bounds__(kBurstThreads) void burst_table_kernel(BurstParams p) {
    __shared__ uint64_t edge[kBurstEdgeSlots];
    __shared__ uint64_t ws[2][kBurstWaves];
    const uint32_t tid = threadIdx.x;
    const EdgeListView &list = p.list;
    if (list.num_captures == 0u) return;
    const uint64_t total = edge_list_total(list);
    TileCursor cur = cursor_begin(list, total);

    for (uint64_t t = blockIdx.x; t < p.num_tiles_cap; t += gridDim.x) {
        if (!cursor_seek(cur, list, total, t)) break;           // (uniform)
        const uint64_t base = (t - cur.tile0) * kBurstTile, E = cur.hi - cur.lo, R = (E + 1u) / 2u;
        __syncthreads();
        stage_edges(edge, list, cur, base);
        __syncthreads();

        const BurstCarry in = p.carry[t];
        const unsigned long long *res = p.result + (size_t)cur.c * kBurstWords;
        const LaneRuns r = lane_runs(edge, p, base, E);
        uint64_t mine = 0ull, all;
#pragma unroll
        for (uint32_t q = 0; q < kBurstRunsPerThread; ++q) mine += r.end[q] - r.begin[q];
        // in front of this lane's first run, within the capture
        uint64_t samples = in.samples - res[kBurstWordBegin + 1u] + block_sum_exclusive(mine, ws[0], all);
        uint64_t bursts = in.starts - res[kBurstWordBegin] + block_sum_exclusive((uint64_t)__popc(r.starts), ws[1], all);
        const uint64_t slot0 = burst_table_base(cur.lo, cur.c);
        const uint64_t run0 = base / 2u + (uint64_t)kBurstRunsPerThread * tid;
#pragma unroll
        for (uint32_t q = 0; q < kBurstRunsPerThread; ++q) {
            if ((r.starts >> q) & 1u) {
                if (bursts < R && slot0 + bursts < p.table_slots) {
                    BurstDev *b = p.table + slot0 + bursts;
                    b->first_sample = r.begin[q];
                    b->offset = samples;
                    b->first_run = run0 + q;
                }
                ++bursts;
            }
            samples += r.end[q] - r.begin[q];
            if ((r.lasts >> q) & 1u) {
                const uint64_t at = bursts - 1u;                // (run 0 begins a burst: there is one in front)
                if (at < R && slot0 + at < p.table_slots) {
                    BurstDev *b = p.table + slot0 + at;
                    b->end_offset = samples;
                    b->end_run = run0 + q + 1u;
                }
            }
        }
    }
}

hipError_t launch_burst_table(const BurstParams &p, uint64_t expect_edges, hipStream_t stream) {
    uint64_t groups = burst_tiles_of(expect_edges, p.list.num_captures);
    if (groups > p.num_tiles_cap) groups = p.num_tiles_cap;
    if (groups < 1u) groups = 1u;
    if (groups > kBurstMaxGroups) groups = kBurstMaxGroups;
    hipLaunchKernelGGL(burst_agg_kernel, dim3((uint32_t)groups), dim3(kBurstThreads), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(burst_scan_kernel, dim3(1), dim3(kBurstThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(burst_table_kernel, dim3((uint32_t)groups), dim3(kBurstThreads), 0, stream, p);
    return hipGetLastError();
}

// ---- the copy --------------------------------------------------------------------------------------------------

namespace {

// 16 bytes of a capture at an address that is only sample-aligned
struct __attribute__((packed, aligned(4))) Vec16a4 {
    uint32_t w[4];
};
struct __attribute__((packed, aligned(2))) Vec16a2 {
    uint32_t w[4];
};

// what the copy reads of an entry
struct BurstSpan {
    uint64_t first, offset, end_offset;
};
__device__ __forceinline__ BurstSpan burst_span(const BurstDev *table, uint64_t b) {
    BurstSpan s;
    s.first = table[b].first_sample;
    s.offset = table[b].offset;
    s.end_offset = table[b].end_offset;
    return s;
}

// the last burst in [lo, hi] whose offset is <= s (lo's is): bursts of no samples share their offset with the burst
// behind them, so this is the burst that holds sample s of the cut
__device__ __forceinline__ uint64_t burst_of(const BurstDev *table, uint64_t lo, uint64_t hi, uint64_t s) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1u) / 2u;
        if (table[mid].offset <= s) {
            lo = mid;
        } else {
            hi = mid - 1u;
        }
    }
    return lo;
}

}  // namespace

// kBytes: of a sample, 4 or 2
template <uint32_t kBytes>
__global__ __launch_bounds__(kBurstCopyThreads) void burst_copy_kernel(BurstCopyParams p) {
    using Sample = typename std::conditional<kBytes == 4u, uint32_t, uint16_t>::type;
    using SrcVec = typename std::conditional<kBytes == 4u, Vec16a4, Vec16a2>::type;
    constexpr uint64_t kPerVec = 16u / kBytes;
    const uint64_t vecs = (p.total + kPerVec - 1u) / kPerVec;
    const uint64_t v0 = (uint64_t)blockIdx.x * kBurstCopySpan;
    if (v0 >= vecs || p.num_bursts == 0u) return;               // (uniform)
    const Sample *src = static_cast<const Sample *>(p.src);
    Sample *dst = static_cast<Sample *>(p.dst);
    const bool vectors = (reinterpret_cast<uintptr_t>(p.dst) & 15u) == 0u;

    // the bursts of the span's first and last sample (uniform: every lane searches the same words)
    const uint64_t s_first = v0 * kPerVec;
    uint64_t s_last = (v0 + kBurstCopySpan) * kPerVec;
    s_last = (s_last < p.total ? s_last : p.total) - 1u;
    const uint64_t b_first = burst_of(p.table, 0u, p.num_bursts - 1u, s_first);
    const uint64_t b_last = burst_of(p.table, b_first, p.num_bursts - 1u, s_last);

    uint64_t b = b_first;
    BurstSpan cur = burst_span(p.table, b);
#pragma unroll 1
    for (uint32_t j = 0; j < kBurstCopyVecPerThread; ++j) {
        const uint64_t v = v0 + (uint64_t)j * kBurstCopyThreads + threadIdx.x;
        if (v >= vecs) break;
        const uint64_t s = v * kPerVec;
        if (s >= cur.end_offset && b < b_last) {                // (a lane's vectors ascend: the walk only goes forward)
            b = burst_of(p.table, b, b_last, s);
            cur = burst_span(p.table, b);
        }
        const uint64_t at = cur.first + (s - cur.offset);
        if (vectors && s >= cur.offset && s + kPerVec <= cur.end_offset && s + kPerVec <= p.total && at + kPerVec <= p.n &&
            at + kPerVec > at) {
            const SrcVec x = *reinterpret_cast<const SrcVec *>(src + at);
            *reinterpret_cast<uint4 *>(dst + s) = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]);
            continue;
        }
        // a vector that straddles bursts, holds whole bursts, or is the cut's partial last one: sample by sample
        uint64_t bb = b;
        BurstSpan c = cur;
        for (uint64_t i = 0; i < kPerVec; ++i) {
            const uint64_t si = s + i;
            if (si >= p.total) break;
            while (si >= c.end_offset && bb < b_last) {
                ++bb;
                c = burst_span(p.table, bb);
            }
            if (si >= c.offset && si < c.end_offset) {
                const uint64_t from = c.first + (si - c.offset);
                if (from < p.n) dst[si] = src[from];
            }
        }
    }
}

hipError_t launch_burst_copy(const BurstCopyParams &p, hipStream_t stream) {
    if (p.total == 0u || p.num_bursts == 0u) return hipSuccess;
    if (p.sample_bytes != 4u && p.sample_bytes != 2u) return hipErrorInvalidValue;
    const uint64_t per_vec = 16u / p.sample_bytes;
    const uint64_t vecs = (p.total + per_vec - 1u) / per_vec;
    const uint64_t groups = (vecs + kBurstCopySpan - 1u) / kBurstCopySpan;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    if (p.sample_bytes == 4u) {
        hipLaunchKernelGGL(burst_copy_kernel<4u>, dim3((uint32_t)groups), dim3(kBurstCopyThreads), 0, stream, p);
    } else {
        hipLaunchKernelGGL(burst_copy_kernel<2u>, dim3((uint32_t)groups), dim3(kBurstCopyThreads), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace ookd
