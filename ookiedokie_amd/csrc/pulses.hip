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

// the capture that owns global edge index g: moves (c, lo, hi) forward until lo <= g < hi.  g only grows from call to
// call, and g < off[num_captures * B], so the loop ends inside the table.
struct CapCursor {
    uint32_t c;
    uint64_t lo, hi;
};
__device__ __forceinline__ void cursor_seek(CapCursor &k, const EdgeListView &v, uint64_t g) {
    while (g >= k.hi && k.c + 1u < v.num_captures) {
        ++k.c;
        k.lo = k.hi;
        k.hi = v.blk_offset[(size_t)(k.c + 1u) * v.blocks_per_cap];
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

    const EdgeListView &list = p.list;
    const uint64_t total = edge_list_total(list);

    // E, first and last edge of every capture: the open runs are the host's to derive
    if (blockIdx.x == 0) {
        for (uint32_t c = tid; c < list.num_captures; c += kPulseThreads) {
            uint64_t lo, hi;
            edge_list_range(list, c, total, lo, hi);
            unsigned long long *m = p.result + (size_t)c * kPulseWords + kPulseMetaWord;
            m[0] = hi - lo;
            m[1] = hi > lo ? list.edges[lo] : 0ull;
            m[2] = hi > lo ? list.edges[hi - 1u] : 0ull;
        }
    }
    __syncthreads();

    const uint64_t steps = (total + kPulseEdgesPerStep - 1u) / kPulseEdgesPerStep;
    CapCursor cur{0u, 0ull, 0ull};
    cur.lo = list.blk_offset[0];
    cur.hi = list.blk_offset[list.blocks_per_cap];
    uint32_t flushed_c = 0u;            // the capture whose runs the LDS histogram holds
    bool dirty = false;
    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const uint64_t base = step * kPulseEdgesPerStep;        // workgroup-uniform
        // The histogram in LDS belongs to one capture at a time: flush it before a step that collects for another
        // capture.  A step with a boundary inside adds straight to the results and leaves the LDS histogram alone.
        CapCursor first = cur;
        cursor_seek(first, list, base);
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
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(list.edges + g);  // g is even: 16-byte aligned
            e0 = v.x;
            e1 = v.y;
        } else if (g < total) {
            e0 = list.edges[g];
        }
        // the edge to the right of the pair: the next lane's first; the wave's last lane fetches it
        uint64_t e2 = (uint64_t)__shfl_down((unsigned long long)e0, 1);
        if (lane == 63u) e2 = g + 2u < total ? list.edges[g + 2u] : 0ull;

        if (one_capture) {
            // run g -> g + 1 and run g + 1 -> g + 2, both inside first.c when their right edge is
            const bool va = g + 1u <= last_g, vb = g + 2u < first.hi;
            const uint32_t la = (uint32_t)((g - first.lo) & 1ull) ^ 1u;     // run i is "on" when i is even
            const uint64_t da = e1 - e0, db = e2 - e1;
            wave_peel_add<true>(hist, va, la * kPulseBins + pulse_bin_of(va ? da : 0ull), da);
            wave_peel_add<true>(hist, vb, (la ^ 1u) * kPulseBins + pulse_bin_of(vb ? db : 0ull), db);
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
                    cursor_seek(k, list, gl);
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
