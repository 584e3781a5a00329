// symbols.hip -- symbol survey: pulse/gap symbols of ONE capture's edge list counted by kind, and the distances
// between its sync symbols (the contract is in include/ookiedokie_amd.h, the design in DESIGN.md 4.16).
//
// Symbol j of the capture is the edges e[2j], e[2j + 1], e[2j + 2].  A workgroup takes a tile of kSymTile symbols
// per step: it stages the tile's edges in LDS with plain 8-byte loads (a capture's list may start at an odd index of
// the run's array, so nothing wider is aligned), and every lane classifies kSymPerThread consecutive symbols.
//
// The frame members need, at every sync, the position of the sync before it and the symbols of role OTHER since:
// a segmented scan over the whole list, done in three dependent launches on one stream -- aggregates per tile
// (with the kind counts), one workgroup that scans the aggregates, and the tiles once more with their carry-in.  No
// workgroup ever waits for another inside a kernel.
#include "symbols.hpp"

namespace ookd {

namespace {

constexpr uint32_t kRoleAbsent = 4;     // a symbol at or beyond S (in LDS only)

// a tile's edges in LDS: slot i holds edge 2 base - 2 + i of the capture, i < kSymTileEdges -- two edges in front of
// the tile's first symbol (the symbol before it, for the frames kernel) and one behind its last.  One spare word
// per eight keeps the lanes' 64-byte strides off the same banks.
constexpr uint32_t kSymTileEdges = 2u * kSymTile + 3u;
__device__ __forceinline__ uint32_t edge_slot(uint32_t i) { return i + (i >> 3); }
constexpr uint32_t kSymEdgeSlots = kSymTileEdges + (kSymTileEdges >> 3) + 1u;

struct CapRange {
    uint64_t lo;        // the capture's first edge in the run's list
    uint64_t S;         // its symbols
    uint32_t tiles;
};

// the capture's range, inside the list (edge_list_dev.hpp), and what it holds in symbols and tiles
__device__ __forceinline__ CapRange cap_range(const SymParams &p) {
    uint64_t lo, hi;
    edge_list_range(p.list, p.capture, edge_list_total(p.list), lo, hi);
    const uint64_t E = hi - lo;
    CapRange r;
    r.lo = lo;
    r.S = E < 3u ? 0ull : (E - 1u) / 2u;
    uint64_t tiles = (r.S + kSymTile - 1u) / kSymTile;
    if (tiles > p.num_tiles_cap) tiles = p.num_tiles_cap;
    r.tiles = (uint32_t)tiles;
    return r;
}

struct SymLds {
    uint64_t edge[kSymEdgeSlots];
    uint64_t lower[2][kSymClasses], upper[2][kSymClasses];
    uint8_t role_of_key[kSymKinds + 7u];
};

__device__ __forceinline__ void load_tables(SymLds &s, const SymParams &p) {
    for (uint32_t i = threadIdx.x; i < 2u * kSymClasses; i += kSymThreads) {
        s.lower[i / kSymClasses][i % kSymClasses] = p.lower[i / kSymClasses][i % kSymClasses];
        s.upper[i / kSymClasses][i % kSymClasses] = p.upper[i / kSymClasses][i % kSymClasses];
    }
    for (uint32_t i = threadIdx.x; i < kSymKinds; i += kSymThreads) s.role_of_key[i] = p.role[i];
}

// the tile's edges into LDS (the caller synchronises before and after).  Edge index 2 S is the last any symbol
// needs, and 2 S <= E - 1: every load lies inside the capture's own list.
__device__ __forceinline__ void stage_edges(SymLds &s, const SymParams &p, const CapRange &r, uint64_t base) {
    const uint64_t end_sym = base + kSymTile < r.S ? base + kSymTile : r.S;
    const int64_t last_edge = (int64_t)(2u * end_sym);
    for (uint32_t i = threadIdx.x; i < kSymTileEdges; i += kSymThreads) {
        const int64_t el = (int64_t)(2u * base) + (int64_t)i - 2;
        uint64_t v = 0ull;
        if (el >= 0 && el <= last_edge) v = p.list.edges[r.lo + (uint64_t)el];
        s.edge[edge_slot(i)] = v;
    }
}

__device__ __forceinline__ uint32_t class_of(const uint64_t *lower, const uint64_t *upper, uint32_t n, uint64_t d) {
    uint32_t c = kSymClasses;
    for (uint32_t k = 0; k < n; ++k)            // (n is uniform; the ranges are disjoint)
        if (d >= lower[k] && d <= upper[k]) c = k;
    return c;
}

// the kind of the tile's symbol with local index sl (-1 .. kSymTile - 1): on class * 17 + off class
__device__ __forceinline__ uint32_t kind_of(const SymLds &s, const SymParams &p, int sl) {
    const uint32_t i = (uint32_t)(2 * sl + 2);
    const uint64_t e0 = s.edge[edge_slot(i)], e1 = s.edge[edge_slot(i + 1u)], e2 = s.edge[edge_slot(i + 2u)];
    const uint32_t on = class_of(s.lower[1], s.upper[1], p.num_classes[1], e1 - e0);
    const uint32_t off = class_of(s.lower[0], s.upper[0], p.num_classes[0], e2 - e1);
    return on * kSymSide + off;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}

// (a then b): what the two stretches together say to what follows them
__device__ __forceinline__ void combine(uint32_t &last, uint32_t &others, uint32_t b_last, uint32_t b_others) {
    if (b_last != kSymNoSync) {
        last = b_last;
        others = b_others;
    } else {
        others += b_others;
    }
}

// inclusive scan of (last, others) over the wave's lanes
__device__ __forceinline__ void wave_scan(uint32_t &last, uint32_t &others) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t pl = (uint32_t)__shfl_up((int)last, s), po = (uint32_t)__shfl_up((int)others, s);
        if (lane >= s && last == kSymNoSync) {
            last = pl;
            others += po;
        }
    }
}

// Workgroup-wide: every thread gives its own stretch (last, others) and leaves with what lies in front of it --
// `carry`, then the threads before it.  tot_* receive carry + all threads (uniform).  wl / wo: LDS, one word per
// wave; the caller synchronises before they are used again.
__device__ __forceinline__ void block_exclusive(uint32_t &last, uint32_t &others, uint32_t carry_last, uint32_t carry_others,
                                                uint32_t *wl, uint32_t *wo, uint32_t &tot_last, uint32_t &tot_others) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    wave_scan(last, others);
    if (lane == 63u) {
        wl[wave] = last;
        wo[wave] = others;
    }
    uint32_t el = (uint32_t)__shfl_up((int)last, 1), eo = (uint32_t)__shfl_up((int)others, 1);
    if (lane == 0u) {
        el = kSymNoSync;
        eo = 0u;
    }
    __syncthreads();
    uint32_t pl = carry_last, po = carry_others;
    tot_last = carry_last;
    tot_others = carry_others;
    for (uint32_t w = 0; w < kSymThreads / 64u; ++w) {
        const uint32_t l = wl[w], o = wo[w];
        if (w < wave) combine(pl, po, l, o);
        combine(tot_last, tot_others, l, o);
    }
    combine(pl, po, el, eo);
    last = pl;
    others = po;
}

}  // namespace

// ---- 1. kind counts, and every tile's aggregate ----------------------------------------------------------------

template <bool kRoles>
__global__ __launch_bounds__(kSymThreads) void symbol_kinds_kernel(SymParams p) {
    __shared__ SymLds s;
    __shared__ unsigned long long hist[kSymKinds];
    __shared__ uint32_t t_first, t_last1, t_syncs, t_others;    // the tile's aggregate (t_last1: last + 1, 0 = no sync)
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const CapRange r = cap_range(p);
    load_tables(s, p);
    for (uint32_t i = tid; i < kSymKinds; i += kSymThreads) hist[i] = 0ull;
    if (blockIdx.x == 0 && tid == 0) p.result[kSymWordS] = r.S;

    for (uint32_t tile = blockIdx.x; tile < r.tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kSymTile;
        __syncthreads();
        stage_edges(s, p, r, base);
        if (kRoles && tid == 0) {
            t_first = kSymNoSync;
            t_last1 = 0u;
            t_syncs = 0u;
            t_others = 0u;
        }
        __syncthreads();

        uint32_t role[kSymPerThread];
        uint32_t syncs = 0u, first = kSymNoSync, last1 = 0u;
#pragma unroll
        for (uint32_t q = 0; q < kSymPerThread; ++q) {
            const uint32_t sl = kSymPerThread * tid + q;
            const uint64_t j = base + sl;
            const bool valid = j < r.S;
            const uint32_t key = valid ? kind_of(s, p, (int)sl) : 0u;
            wave_peel_add<false>(hist, valid, key, 0ull);
            if (kRoles) {
                role[q] = valid ? (uint32_t)s.role_of_key[key] : kRoleAbsent;
                if (role[q] == kRoleSync) {
                    if (first == kSymNoSync) first = (uint32_t)j;
                    last1 = (uint32_t)j + 1u;
                    ++syncs;
                }
            }
        }
        if (kRoles) {
            if (syncs) {
                atomicMin(&t_first, first);
                atomicMax(&t_last1, last1);
                atomicAdd(&t_syncs, syncs);
            }
            __syncthreads();
            // the OTHERs behind the tile's last sync (all of them, without one)
            const uint32_t from = t_last1;
            uint32_t others = 0u;
#pragma unroll
            for (uint32_t q = 0; q < kSymPerThread; ++q)
                others += (role[q] == kRoleOther && (uint32_t)(base + kSymPerThread * tid + q) >= from) ? 1u : 0u;
            others = wave_sum_u32(others);
            if (lane == 0u && others) atomicAdd(&t_others, others);
            __syncthreads();
            if (tid == 0) {
                SymAgg a;
                a.last = t_last1 ? t_last1 - 1u : kSymNoSync;
                a.others = t_others;
                a.first = t_first;
                a.syncs = t_syncs;
                p.agg[tile] = a;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < kSymKinds; i += kSymThreads) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&p.result[kSymWordKinds + i], v);
    }
}

// ---- 2. one workgroup: every tile's carry-in, and the totals ---------------------------------------------------

__global__ __launch_bounds__(kSymScanThreads) void symbol_scan_kernel(SymParams p) {
    __shared__ uint32_t wl[kSymScanThreads / 64u], wo[kSymScanThreads / 64u];
    __shared__ uint32_t t_first;
    __shared__ unsigned long long t_syncs;
    static_assert(kSymScanThreads == kSymThreads, "block_exclusive is written for kSymThreads");
    const uint32_t tid = threadIdx.x;
    const CapRange r = cap_range(p);
    if (tid == 0) {
        t_first = kSymNoSync;
        t_syncs = 0ull;
    }
    uint32_t carry_last = kSymNoSync, carry_others = 0u;        // (uniform)
    uint32_t first = kSymNoSync;
    unsigned long long syncs = 0ull;
    for (uint32_t chunk = 0; chunk < r.tiles; chunk += kSymScanThreads) {
        const uint32_t i = chunk + tid;
        uint32_t last = kSymNoSync, others = 0u;
        if (i < r.tiles) {
            const SymAgg a = p.agg[i];
            last = a.last;
            others = a.others;
            if (a.first < first) first = a.first;
            syncs += a.syncs;
        }
        uint32_t tot_last, tot_others;
        __syncthreads();
        block_exclusive(last, others, carry_last, carry_others, wl, wo, tot_last, tot_others);
        if (i < r.tiles) {
            SymCarry c;
            c.last = last;
            c.others = others;
            p.carry[i] = c;
        }
        carry_last = tot_last;
        carry_others = tot_others;
    }
    __syncthreads();
    if (first != kSymNoSync) atomicMin(&t_first, first);
    if (syncs) atomicAdd(&t_syncs, syncs);
    __syncthreads();
    if (tid == 0) {
        p.result[kSymWordSyncs] = t_syncs;
        p.result[kSymWordSyncs + 1u] = t_first != kSymNoSync ? (unsigned long long)t_first : (unsigned long long)r.S;
        p.result[kSymWordSyncs + 2u] = carry_last != kSymNoSync ? (unsigned long long)(r.S - carry_last) : 0ull;
    }
}

// ---- 3. every tile once more, with its carry-in: the frames ----------------------------------------------------

__global__ __launch_bounds__(kSymThreads) void symbol_frames_kernel(SymParams p) {
    __shared__ SymLds s;
    __shared__ unsigned long long frames[2u * kFrameBins];
    __shared__ uint8_t role_of[kSymTile + 8u];                  // role_of[sl + 1], sl = -1 .. kSymTile - 1
    __shared__ uint32_t wl[kSymThreads / 64u], wo[kSymThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const CapRange r = cap_range(p);
    load_tables(s, p);
    for (uint32_t i = tid; i < 2u * kFrameBins; i += kSymThreads) frames[i] = 0ull;

    for (uint32_t tile = blockIdx.x; tile < r.tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kSymTile;
        __syncthreads();
        stage_edges(s, p, r, base);
        __syncthreads();

        uint32_t role[kSymPerThread];
        uint32_t last = kSymNoSync, others = 0u;
#pragma unroll
        for (uint32_t q = 0; q < kSymPerThread; ++q) {
            const uint32_t sl = kSymPerThread * tid + q;
            const uint64_t j = base + sl;
            role[q] = j < r.S ? (uint32_t)s.role_of_key[kind_of(s, p, (int)sl)] : kRoleAbsent;
            role_of[sl + 1u] = (uint8_t)role[q];
            if (role[q] == kRoleSync) {
                last = (uint32_t)j;
                others = 0u;
            } else if (role[q] == kRoleOther) {
                ++others;
            }
        }
        if (tid == 0) role_of[0] = (uint8_t)(base ? (uint32_t)s.role_of_key[kind_of(s, p, -1)] : kRoleAbsent);
        const SymCarry c = p.carry[tile];
        uint32_t tot_last, tot_others;
        block_exclusive(last, others, c.last, c.others, wl, wo, tot_last, tot_others);      // (synchronises: role_of is whole)

        // this lane's symbols again, from what lies in front of them
#pragma unroll
        for (uint32_t q = 0; q < kSymPerThread; ++q) {
            const uint32_t sl = kSymPerThread * tid + q;
            if (role[q] == kRoleSync) {
                const uint32_t j = (uint32_t)(base + sl);
                if (last != kSymNoSync) {
                    const uint32_t d = j - last;
                    // the symbol just before this sync is free (a sync there is no OTHER: nothing to take off)
                    const uint32_t inside = others - (role_of[sl] == kRoleOther ? 1u : 0u);
                    const uint32_t bin = d < kFrameBins - 1u ? d : kFrameBins - 1u;
                    atomicAdd(&frames[(inside == 0u ? kFrameBins : 0u) + bin], 1ull);
                }
                last = j;
                others = 0u;
            } else if (role[q] == kRoleOther) {
                ++others;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 2u * kFrameBins; i += kSymThreads) {
        const unsigned long long v = frames[i];
        if (v) atomicAdd(&p.result[kSymWordFrames + i], v);
    }
}

hipError_t launch_symbol_survey(const SymParams &p, bool with_roles, uint64_t expect_edges, hipStream_t stream) {
    uint32_t groups = sym_tiles_of(expect_edges);
    if (groups > p.num_tiles_cap) groups = p.num_tiles_cap;
    if (groups < 1u) groups = 1u;
    if (groups > kSymMaxGroups) groups = kSymMaxGroups;
    if (!with_roles) {
        hipLaunchKernelGGL(symbol_kinds_kernel<false>, dim3(groups), dim3(kSymThreads), 0, stream, p);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(symbol_kinds_kernel<true>, dim3(groups), dim3(kSymThreads), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(symbol_scan_kernel, dim3(1), dim3(kSymScanThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(symbol_frames_kernel, dim3(groups), dim3(kSymThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ookd
