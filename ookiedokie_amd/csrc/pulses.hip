// pulses.hip -- pulse survey: run-length histograms of every capture's edge list in one pass (the contract is in
// include/ookiedokie_amd.h, the design in DESIGN.md 4.15).
//
// The run's edge lists lie end to end in one array; capture c owns [off[c B], off[(c + 1) B]) of it, B = blocks per
// capture, off = the edge stage's exclusive prefix (what ookd_rx_get_edges copies two words of).  The grid walks the
// array as one list: a lane loads two neighbouring edges with one 16-byte load, takes the edge to their right from
// the next lane, and knows from the capture's bounds which of its two differences are runs of that capture.
#include "pulses.hpp"

namespace ookd {

namespace {

constexpr int kPulsePeelRounds = 6;     // distinct (level, bin) keys a wave looks at before its lanes add for themselves
constexpr uint32_t kPulsePeelMin = 8;   // a key held by fewer lanes is not worth the reduction: its lanes add for themselves

// sum over the wave (every lane calls it; lanes outside the group pass 0)
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, s);
    return v;
}

// Every lane of the wave calls this together.  An OOK capture puts nearly all runs of a level into a handful of
// bins, so most lanes of a wave hold the same key: the wave finds the lanes that share the first pending lane's
// key, sums their lengths across lanes, and that lane alone adds (count, sum) to the workgroup's histogram -- one
// LDS add per distinct key instead of up to 64 on one address.  A key held by few lanes (a rare timing; a capture
// whose runs spread over many bins) gains nothing from the reduction: its lanes step aside to add for themselves
// and the rounds go on with the next pending key, so a rare key in the first lane does not end them.
__device__ __forceinline__ void wave_add_runs(unsigned long long *hist, bool valid, uint32_t key, uint64_t len) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(valid), self = 0ull;
#pragma unroll 1
    for (int r = 0; r < kPulsePeelRounds && todo; ++r) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader);
        const bool mine = valid && key == lk;
        const uint64_t same = __ballot(mine) & todo;
        const uint32_t n = (uint32_t)__popcll(same);
        todo &= ~same;
        if (n < kPulsePeelMin) {                // (wave-uniform)
            self |= same;
            continue;
        }
        const uint64_t total = wave_sum_u64(mine ? len : 0ull);
        if ((int)lane == leader) {
            atomicAdd(&hist[2u * lk], (unsigned long long)n);
            atomicAdd(&hist[2u * lk + 1u], (unsigned long long)total);
        }
    }
    self |= todo;
    if ((self >> lane) & 1ull) {
        atomicAdd(&hist[2u * key], 1ull);
        atomicAdd(&hist[2u * key + 1u], (unsigned long long)len);
    }
}

// the capture that owns global edge index g: moves (c, lo, hi) forward until lo <= g < hi.  g only grows from call to
// call, and g < off[num_captures * B], so the loop ends inside the table.
struct CapCursor {
    uint32_t c;
    uint64_t lo, hi;
};
__device__ __forceinline__ void cursor_seek(CapCursor &k, const PulseParams &p, uint64_t g) {
    while (g >= k.hi && k.c + 1u < p.num_captures) {
        ++k.c;
        k.lo = k.hi;
        k.hi = p.blk_offset[(size_t)(k.c + 1u) * p.blocks_per_cap];
    }
}

__device__ __forceinline__ void flush_hist(const unsigned long long *hist, unsigned long long *dst) {
    for (uint32_t i = threadIdx.x; i < 2u * kPulseKeys; i += kPulseThreads) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

}  // namespace

__global__ __launch_bounds__(kPulseThreads) void pulse_hist_kernel(PulseParams p) {
    __shared__ unsigned long long hist[2u * kPulseKeys];       // (count, sum) per (level, bin): 16 KiB
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < 2u * kPulseKeys; i += kPulseThreads) hist[i] = 0ull;

    // the list's end: the prefix's last word, and never beyond what the list can hold (the host refuses a run whose
    // list overflowed; this keeps the loads inside the allocation whatever it was given)
    uint64_t total = p.blk_offset[(size_t)p.num_captures * p.blocks_per_cap];
    if (total > p.edge_capacity) total = p.edge_capacity;

    // E, first and last edge of every capture: the open runs are the host's to derive
    if (blockIdx.x == 0) {
        for (uint32_t c = tid; c < p.num_captures; c += kPulseThreads) {
            uint64_t lo = p.blk_offset[(size_t)c * p.blocks_per_cap];
            uint64_t hi = p.blk_offset[(size_t)(c + 1u) * p.blocks_per_cap];
            if (hi > total) hi = total;
            if (lo > hi) lo = hi;
            unsigned long long *m = p.result + (size_t)c * kPulseWords + kPulseMetaWord;
            m[0] = hi - lo;
            m[1] = hi > lo ? p.edges[lo] : 0ull;
            m[2] = hi > lo ? p.edges[hi - 1u] : 0ull;
        }
    }
    __syncthreads();

    const uint64_t steps = (total + kPulseEdgesPerStep - 1u) / kPulseEdgesPerStep;
    CapCursor cur{0u, 0ull, 0ull};
    cur.lo = p.blk_offset[0];
    cur.hi = p.blk_offset[p.blocks_per_cap];
    uint32_t flushed_c = 0u;            // the capture whose runs the LDS histogram holds
    bool dirty = false;
    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const uint64_t base = step * kPulseEdgesPerStep;        // workgroup-uniform
        // The histogram in LDS belongs to one capture at a time: flush it before a step that collects for another
        // capture.  A step with a boundary inside adds straight to the results and leaves the LDS histogram alone.
        CapCursor first = cur;
        cursor_seek(first, p, base);
        const uint64_t last_g = (base + kPulseEdgesPerStep < total ? base + kPulseEdgesPerStep : total) - 1u;
        const bool one_capture = last_g < first.hi;     // uniform: every edge of the step lies in first.c
        if (dirty && one_capture && first.c != flushed_c) {
            __syncthreads();
            flush_hist(hist, p.result + (size_t)flushed_c * kPulseWords);
            __syncthreads();
            for (uint32_t i = tid; i < 2u * kPulseKeys; i += kPulseThreads) hist[i] = 0ull;
            __syncthreads();
            dirty = false;
        }
        cur = first;

        const uint64_t g = base + 2ull * tid;           // this lane's two edges: g, g + 1
        uint64_t e0 = 0ull, e1 = 0ull;
        if (g + 1u < total) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(p.edges + g);     // g is even: 16-byte aligned
            e0 = v.x;
            e1 = v.y;
        } else if (g < total) {
            e0 = p.edges[g];
        }
        // the edge to the right of the pair: the next lane's first; the wave's last lane fetches it
        uint64_t e2 = (uint64_t)__shfl_down((unsigned long long)e0, 1);
        if (lane == 63u) e2 = g + 2u < total ? p.edges[g + 2u] : 0ull;

        if (one_capture) {
            // run g -> g + 1 and run g + 1 -> g + 2, both inside first.c when their right edge is
            const bool va = g + 1u <= last_g, vb = g + 2u < first.hi;
            const uint32_t la = (uint32_t)((g - first.lo) & 1ull) ^ 1u;     // run i is "on" when i is even
            const uint64_t da = e1 - e0, db = e2 - e1;
            wave_add_runs(hist, va, la * kPulseBins + pulse_bin_of(va ? da : 0ull), da);
            wave_add_runs(hist, vb, (la ^ 1u) * kPulseBins + pulse_bin_of(vb ? db : 0ull), db);
            flushed_c = first.c;
            dirty = true;
        } else {
            // a boundary between captures inside the step: every lane finds the capture of each of its edges, and a
            // difference is a run only when both edges are that capture's
            CapCursor k = first;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint64_t gl = g + (uint64_t)h;
                if (gl < total) {
                    cursor_seek(k, p, gl);
                    if (gl >= k.lo && gl + 1u < k.hi && gl + 1u < total) {
                        const uint64_t d = h == 0 ? e1 - e0 : e2 - e1;
                        const uint32_t lv = (uint32_t)((gl - k.lo) & 1ull) ^ 1u;
                        unsigned long long *dst = p.result + (size_t)k.c * kPulseWords + 2u * (lv * kPulseBins + pulse_bin_of(d));
                        atomicAdd(&dst[0], 1ull);
                        atomicAdd(&dst[1], (unsigned long long)d);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (dirty) flush_hist(hist, p.result + (size_t)flushed_c * kPulseWords);
}

hipError_t launch_pulse_hist(const PulseParams &p, uint64_t expect_edges, hipStream_t stream) {
    const uint64_t per_group = (uint64_t)kPulseEdgesPerStep * kPulseStepsPerGroup;
    uint64_t groups = (expect_edges + per_group - 1u) / per_group;
    if (groups < 1u) groups = 1u;
    if (groups > kPulseMaxGroups) groups = kPulseMaxGroups;
    hipLaunchKernelGGL(pulse_hist_kernel, dim3((uint32_t)groups), dim3(kPulseThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ookd
