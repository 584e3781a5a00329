// clean.hip -- edge cleaning: the runs shorter than a minimum deleted from every capture's edge list, and the kept
// edges written to a second, compact list (the contract is in include/ookiedokie_amd.h, the design in DESIGN.md 4.19).
//
// d(i) = short(i) && !d(i-1) is a recurrence along a capture's runs: a segmented scan, shaped like symbols.hip's and
// done in three dependent launches on one stream -- aggregates per tile, one workgroup that scans the aggregates, and
// the tiles once more with their carry-in, which compact the kept edges.  No workgroup ever waits for another inside
// a kernel.  A tile is kCleanTile edges of ONE capture (every capture's last tile may be partial), so the carry starts
// at 0 at every capture's first tile; a tile's edges are staged in LDS with plain 8-byte loads (a capture's list may
// start at an odd index of the run's array, so nothing wider is aligned).
//
// The recurrence as a scan: a short run maps the d in front of it to its negation, any other run maps it to 0.  Maps
// of one bit compose associatively and there are four of them (const 0, const 1, id, not), two bits each
// (clean.hpp: map_then), so lanes, waves, tiles and captures all scan the same way.
//
// A debounced context queues the same three launches in every run's chain and a fourth behind them,
// clean_block_prefix_kernel: the cleaned list's prefix over the run's own blocks, which the state machine reads in the
// place of the run's blk_offset.
#include "clean.hpp"
#include "kernels.hpp"     // kBlockShift: the edge stage's block

namespace ookd {

namespace {

// a tile's edges in LDS: slot i holds edge base + i of the capture, i <= kCleanTile (one edge behind the tile's last
// closes its last run).  One spare word per eight keeps the lanes' 64-byte strides off the same banks.
constexpr uint32_t kCleanTileEdges = kCleanTile + 1u;
__device__ __forceinline__ uint32_t edge_slot(uint32_t i) { return i + (i >> 3); }
constexpr uint32_t kCleanEdgeSlots = kCleanTileEdges + (kCleanTileEdges >> 3) + 1u;
constexpr uint32_t kCleanWaves = kCleanThreads / 64u;
static_assert(kCleanPerThread % 2u == 0u, "a lane's first run is an on-run: the level is the parity of q");

// the capture that owns tile t of the run: (c, its range, its first tile, its tiles).  t only grows from call to call.
struct TileCursor {
    uint32_t c;
    uint64_t lo, hi;
    uint64_t tile0, tiles;
};
__device__ __forceinline__ uint64_t tiles_of(uint64_t lo, uint64_t hi) { return (hi - lo + kCleanTile - 1u) / kCleanTile; }

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

// the tile's edges into LDS (the caller synchronises before and after): edges base .. base + kCleanTile of the
// capture's E; every load lies inside the capture's own list
__device__ __forceinline__ void stage_edges(uint64_t *edge, const EdgeListView &v, const TileCursor &k, uint64_t base) {
    const uint64_t E = k.hi - k.lo;
    for (uint32_t i = threadIdx.x; i < kCleanTileEdges; i += kCleanThreads) {
        const uint64_t el = base + i;
        edge[edge_slot(i)] = el < E ? v.edges[k.lo + el] : 0ull;
    }
}

// bit q: this lane's run base + kCleanPerThread tid + q exists (is closed) and is short
__device__ __forceinline__ uint32_t lane_shorts(const uint64_t *edge, const CleanParams &p, uint64_t base, uint64_t E) {
    const uint32_t j0 = kCleanPerThread * threadIdx.x;
    uint32_t shorts = 0u;
    uint64_t e0 = edge[edge_slot(j0)];
#pragma unroll
    for (uint32_t q = 0; q < kCleanPerThread; ++q) {
        const uint64_t e1 = edge[edge_slot(j0 + q + 1u)];
        // base and j0 are even: run base + j0 + q is "on" when q is even
        if (base + j0 + q + 1u < E && e1 - e0 < p.min_len[(q & 1u) ^ 1u]) shorts |= 1u << q;
        e0 = e1;
    }
    return shorts;
}

__device__ __forceinline__ uint32_t map_of_shorts(uint32_t shorts) {
    uint32_t m = kMapId;
#pragma unroll
    for (uint32_t q = 0; q < kCleanPerThread; ++q) m = map_then(m, (shorts >> q) & 1u ? kMapNot : kMapConst0);
    return m;
}

// Workgroup-wide: every thread gives the map of its own stretch and leaves with the map of everything in front of it
// in the workgroup; `all` receives the map of the whole workgroup (uniform).  wm: LDS, one word per wave; the caller
// synchronises before it is used again.
__device__ __forceinline__ uint32_t block_map_exclusive(uint32_t m, uint32_t *wm, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t prev = (uint32_t)__shfl_up((int)m, s);
        if (lane >= s) m = map_then(prev, m);
    }
    if (lane == 63u) wm[wave] = m;
    uint32_t exc = (uint32_t)__shfl_up((int)m, 1);
    if (lane == 0u) exc = kMapId;
    __syncthreads();
    uint32_t pre = kMapId;
    all = kMapId;
    for (uint32_t w = 0; w < kCleanWaves; ++w) {
        const uint32_t mw = wm[w];
        if (w < wave) pre = map_then(pre, mw);
        all = map_then(all, mw);
    }
    return map_then(pre, exc);
}

// The same for a sum: leaves with the sum of the threads in front; `all` receives the workgroup's sum
__device__ __forceinline__ uint32_t block_sum_exclusive(uint32_t v, uint32_t *ws, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t prev = (uint32_t)__shfl_up((int)inc, s);
        if (lane >= s) inc += prev;
    }
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    uint32_t pre = 0u;
    all = 0u;
    for (uint32_t w = 0; w < kCleanWaves; ++w) {
        const uint32_t sw = ws[w];
        if (w < wave) pre += sw;
        all += sw;
    }
    return pre + inc - v;
}

}  // namespace

// ---- 1. every tile's aggregate ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kCleanThreads) void clean_agg_kernel(CleanParams p) {
    __shared__ uint64_t edge[kCleanEdgeSlots];
    __shared__ uint32_t wm[kCleanWaves];
    __shared__ uint32_t cnt[6];                 // kept[2], del[2][2] of the tile
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const EdgeListView &list = p.list;
    if (list.num_captures == 0u) return;
    const uint64_t total = edge_list_total(list);
    TileCursor cur = cursor_begin(list, total);

    for (uint64_t t = blockIdx.x; t < p.num_tiles_cap; t += gridDim.x) {
        if (!cursor_seek(cur, list, total, t)) break;           // (uniform)
        const uint64_t k = t - cur.tile0, base = k * kCleanTile, E = cur.hi - cur.lo;
        __syncthreads();
        stage_edges(edge, list, cur, base);
        if (tid < 6u) cnt[tid] = 0u;
        __syncthreads();

        const uint32_t shorts = lane_shorts(edge, p, base, E);
        uint32_t all;
        const uint32_t front = block_map_exclusive(map_of_shorts(shorts), wm, all);
        // this lane's runs once for each d in front of the tile; six counts of at most 8, ten bits each
        uint64_t packed = 0ull;
#pragma unroll
        for (uint32_t x = 0; x < 2u; ++x) {
            uint32_t d = (front >> x) & 1u, kept = 0u, del[2] = {0u, 0u};
#pragma unroll
            for (uint32_t q = 0; q < kCleanPerThread; ++q) {
                const uint32_t dn = ((shorts >> q) & 1u) & (d ^ 1u);
                const bool is_edge = base + kCleanPerThread * tid + q < E;
                kept += (is_edge && !(dn | d)) ? 1u : 0u;
                del[(q & 1u) ^ 1u] += dn;
                d = dn;
            }
            packed |= (uint64_t)kept << (30u * x) | (uint64_t)del[0] << (30u * x + 10u) | (uint64_t)del[1] << (30u * x + 20u);
        }
        packed = wave_sum_u64(packed);          // (64 lanes x 8 < 2^10: no field carries into the next)
        if (lane == 0u) {
#pragma unroll
            for (uint32_t f = 0; f < 6u; ++f) atomicAdd(&cnt[f], (uint32_t)(packed >> (10u * f)) & 1023u);
        }
        __syncthreads();
        if (tid == 0u) {
            CleanAgg a;
            a.kept[0] = cnt[0];
            a.del[0][0] = cnt[1];
            a.del[0][1] = cnt[2];
            a.kept[1] = cnt[3];
            a.del[1][0] = cnt[4];
            a.del[1][1] = cnt[5];
            a.map = all;
            a.capture = cur.c | (k == 0u ? kCleanFirst : 0u) | (k + 1u == cur.tiles ? kCleanLast : 0u);
            p.agg[t] = a;
        }
    }
}

// ---- 2. one workgroup: every tile's carry-in and offset, every capture's counts and cleaned prefix -------------

__global__ __launch_bounds__(kCleanThreads) void clean_scan_kernel(CleanParams p) {
    __shared__ uint32_t wm[kCleanWaves], ws[3][kCleanWaves];
    __shared__ unsigned long long t_tiles;
    const uint32_t tid = threadIdx.x;
    const EdgeListView &list = p.list;
    const uint64_t total = edge_list_total(list);
    if (tid == 0u) t_tiles = 0ull;
    __syncthreads();
    {
        unsigned long long mine = 0ull;
        for (uint32_t c = tid; c < list.num_captures; c += kCleanThreads) {
            uint64_t lo, hi;
            edge_list_range(list, c, total, lo, hi);
            mine += tiles_of(lo, hi);
        }
        if (mine) atomicAdd(&t_tiles, mine);
    }
    __syncthreads();
    const uint32_t tiles = (uint32_t)(t_tiles < p.num_tiles_cap ? t_tiles : p.num_tiles_cap);

    // the tiles: d in front of each, and the sums (kept edges, deleted runs per level) in front of each.  A lane takes
    // kCleanScanPerThread consecutive aggregates -- their loads are in flight together -- folds them, and the
    // workgroup scans the lanes' folds: one step covers 2048 tiles
    uint32_t carry_d = 0u, carry_sum[3] = {0u, 0u, 0u};         // (uniform)
    for (uint32_t chunk = 0; chunk < tiles; chunk += kCleanThreads * kCleanScanPerThread) {
        const uint32_t t0 = chunk + tid * kCleanScanPerThread;
        CleanAgg a[kCleanScanPerThread];
        uint32_t m[kCleanScanPerThread], fold = kMapId;
#pragma unroll
        for (uint32_t j = 0; j < kCleanScanPerThread; ++j) {
            a[j] = CleanAgg{};
            a[j].map = kMapId;
            if (t0 + j < tiles) a[j] = p.agg[t0 + j];
        }
#pragma unroll
        for (uint32_t j = 0; j < kCleanScanPerThread; ++j) {
            // a capture's first tile has 0 in front of it whatever came before: to what follows it says a constant
            m[j] = (a[j].capture & kCleanFirst) ? ((a[j].map & 1u) ? kMapConst1 : kMapConst0) : (a[j].map & 3u);
            fold = map_then(fold, m[j]);
        }
        __syncthreads();
        uint32_t all;
        const uint32_t front = block_map_exclusive(fold, wm, all);
        uint32_t d = (front >> carry_d) & 1u;                   // in front of this lane's first tile
        carry_d = (all >> carry_d) & 1u;
        uint32_t x[kCleanScanPerThread], v[kCleanScanPerThread][3], mine[3] = {0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < kCleanScanPerThread; ++j) {
            x[j] = (a[j].capture & kCleanFirst) ? 0u : d;
            d = (m[j] >> d) & 1u;
            const bool valid = t0 + j < tiles;
            v[j][0] = valid ? (x[j] ? a[j].kept[1] : a[j].kept[0]) : 0u;
            v[j][1] = valid ? (x[j] ? a[j].del[1][0] : a[j].del[0][0]) : 0u;
            v[j][2] = valid ? (x[j] ? a[j].del[1][1] : a[j].del[0][1]) : 0u;
#pragma unroll
            for (uint32_t f = 0; f < 3u; ++f) mine[f] += v[j][f];
        }
        uint32_t exc[3];
#pragma unroll
        for (uint32_t f = 0; f < 3u; ++f) {
            uint32_t sum;
            exc[f] = carry_sum[f] + block_sum_exclusive(mine[f], ws[f], sum);
            carry_sum[f] += sum;
        }
#pragma unroll
        for (uint32_t j = 0; j < kCleanScanPerThread; ++j) {
            if (t0 + j < tiles) {
                CleanCarry c;
                c.d = x[j];
                c.offset = exc[0];
                p.carry[t0 + j] = c;
                const uint32_t cap = a[j].capture & ~(kCleanFirst | kCleanLast);
                if (cap < list.num_captures) {
                    unsigned long long *r = p.result + (size_t)cap * kCleanWords;
                    if (a[j].capture & kCleanFirst) {
                        r[kCleanWordBegin] = exc[0];
                        r[kCleanWordBegin + 1u] = exc[1];
                        r[kCleanWordBegin + 2u] = exc[2];
                    }
                    if (a[j].capture & kCleanLast) {            // (the sums behind the capture, until the second half)
                        r[kCleanWordOut] = exc[0] + v[j][0];
                        r[kCleanWordDel] = exc[1] + v[j][1];
                        r[kCleanWordDel + 1u] = exc[2] + v[j][2];
                    }
                }
            }
#pragma unroll
            for (uint32_t f = 0; f < 3u; ++f) exc[f] += v[j][f];
        }
    }
    __syncthreads();

    // the captures: their counts, and the exclusive prefix of their cleaned edges (a capture without an edge has no
    // tile: its words are still zero)
    uint32_t carry_out = 0u;
    for (uint32_t chunk = 0; chunk < list.num_captures; chunk += kCleanThreads) {
        const uint32_t c = chunk + tid;
        uint32_t out = 0u;
        if (c < list.num_captures) {
            uint64_t lo, hi;
            edge_list_range(list, c, total, lo, hi);
            unsigned long long *r = p.result + (size_t)c * kCleanWords;
            out = (uint32_t)(r[kCleanWordOut] - r[kCleanWordBegin]);
            r[kCleanWordDel] -= r[kCleanWordBegin + 1u];
            r[kCleanWordDel + 1u] -= r[kCleanWordBegin + 2u];
            r[kCleanWordOut] = out;
            r[kCleanWordIn] = hi - lo;
        }
        __syncthreads();
        uint32_t sum;
        const uint32_t exc = carry_out + block_sum_exclusive(out, ws[0], sum);
        if (c < list.num_captures) p.out_prefix[c] = exc;
        carry_out += sum;
    }
    if (tid == 0u) p.out_prefix[list.num_captures] = carry_out;
}

// ---- 3. every tile once more, with its carry-in: the kept edges, compacted -------------------------------------

__global__ __launch_bounds__(kCleanThreads) void clean_compact_kernel(CleanParams p) {
    __shared__ uint64_t edge[kCleanEdgeSlots];
    __shared__ uint64_t kept_edge[kCleanTile];
    __shared__ uint32_t wm[kCleanWaves], ws[kCleanWaves];
    const uint32_t tid = threadIdx.x;
    const EdgeListView &list = p.list;
    if (list.num_captures == 0u) return;
    const uint64_t total = edge_list_total(list);
    TileCursor cur = cursor_begin(list, total);

    for (uint64_t t = blockIdx.x; t < p.num_tiles_cap; t += gridDim.x) {
        if (!cursor_seek(cur, list, total, t)) break;           // (uniform)
        const uint64_t base = (t - cur.tile0) * kCleanTile, E = cur.hi - cur.lo;
        __syncthreads();
        stage_edges(edge, list, cur, base);
        __syncthreads();

        const CleanCarry in = p.carry[t];
        const uint32_t shorts = lane_shorts(edge, p, base, E);
        uint32_t all;
        const uint32_t front = block_map_exclusive(map_of_shorts(shorts), wm, all);
        // edge i goes with run i (d now) or with run i - 1 (d before)
        uint32_t d = (front >> (in.d & 1u)) & 1u, keep = 0u;
#pragma unroll
        for (uint32_t q = 0; q < kCleanPerThread; ++q) {
            const uint32_t dn = ((shorts >> q) & 1u) & (d ^ 1u);
            if (base + kCleanPerThread * tid + q < E && !(dn | d)) keep |= 1u << q;
            d = dn;
        }
        uint32_t kept_tile;
        uint32_t at = block_sum_exclusive((uint32_t)__popc(keep), ws, kept_tile);
#pragma unroll
        for (uint32_t q = 0; q < kCleanPerThread; ++q) {
            if ((keep >> q) & 1u) kept_edge[at++] = edge[edge_slot(kCleanPerThread * tid + q)];
        }
        __syncthreads();
        for (uint32_t j = tid; j < kept_tile; j += kCleanThreads) {
            const uint64_t o = (uint64_t)in.offset + j;
            if (o < p.out_capacity) p.out[o] = kept_edge[j];
        }
    }
}

// ---- 4. (the debounced decode only) the cleaned list's prefix over the run's own blocks ------------------------
//
// One lane per block: a lower bound for b * 4096 inside the capture's cleaned range.  The cleaned edges in front of a
// block are among the run's own in front of it, so the run's own prefix brackets the search from above.  Whatever the
// lists hold, every load stays below out_capacity and every store below blk_prefix_capacity.
__global__ __launch_bounds__(kCleanThreads) void clean_block_prefix_kernel(CleanParams p) {
    const EdgeListView &list = p.list;
    const uint64_t bpc = list.blocks_per_cap;
    if (list.num_captures == 0u || bpc == 0u) return;
    const uint64_t entries = (uint64_t)list.num_captures * bpc;     // and one more word: the total
    const uint64_t raw_total = edge_list_total(list);
    for (uint64_t i = (uint64_t)blockIdx.x * kCleanThreads + threadIdx.x; i <= entries; i += (uint64_t)gridDim.x * kCleanThreads) {
        if (i >= p.blk_prefix_capacity) break;
        const uint32_t c = (uint32_t)(i / bpc);
        const uint64_t b = i - (uint64_t)c * bpc;
        uint64_t lo = p.out_prefix[c];
        if (lo > p.out_capacity) lo = p.out_capacity;
        if (i == entries) {
            p.blk_prefix[i] = (uint32_t)lo;
            break;
        }
        uint64_t hi = p.out_prefix[c + 1u];
        if (hi > p.out_capacity) hi = p.out_capacity;
        if (hi < lo) hi = lo;
        uint64_t raw_lo, raw_hi;
        edge_list_range(list, c, raw_total, raw_lo, raw_hi);
        uint64_t raw_b = list.blk_offset[i];
        if (raw_b > raw_hi) raw_b = raw_hi;
        if (raw_b < raw_lo) raw_b = raw_lo;
        // first cleaned edge of the capture at or beyond the block's first output, among its first `n`
        uint64_t j0 = 0u, n = hi - lo < raw_b - raw_lo ? hi - lo : raw_b - raw_lo;
        const uint64_t at = b << kBlockShift;
        while (n != 0u) {
            const uint64_t half = n >> 1;
            if (p.out[lo + j0 + half] < at) {
                j0 += half + 1u;
                n -= half + 1u;
            } else {
                n = half;
            }
        }
        p.blk_prefix[i] = (uint32_t)(lo + j0);
    }
}

hipError_t launch_clean_edges(const CleanParams &p, uint64_t expect_edges, hipStream_t stream) {
    uint64_t groups = clean_tiles_of(expect_edges, p.list.num_captures);
    if (groups > p.num_tiles_cap) groups = p.num_tiles_cap;
    if (groups < 1u) groups = 1u;
    if (groups > kCleanMaxGroups) groups = kCleanMaxGroups;
    hipLaunchKernelGGL(clean_agg_kernel, dim3((uint32_t)groups), dim3(kCleanThreads), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(clean_scan_kernel, dim3(1), dim3(kCleanThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(clean_compact_kernel, dim3((uint32_t)groups), dim3(kCleanThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess || !p.blk_prefix) return e;
    uint64_t lanes = (uint64_t)p.list.num_captures * p.list.blocks_per_cap + 1u;
    if (lanes > p.blk_prefix_capacity) lanes = p.blk_prefix_capacity;
    groups = (lanes + kCleanThreads - 1u) / kCleanThreads;
    if (groups < 1u) groups = 1u;
    if (groups > kCleanMaxGroups) groups = kCleanMaxGroups;
    hipLaunchKernelGGL(clean_block_prefix_kernel, dim3((uint32_t)groups), dim3(kCleanThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ookd
