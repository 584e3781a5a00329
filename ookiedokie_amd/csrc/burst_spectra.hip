// burst_spectra.hip -- burst spectra: the Welch spectrum of every burst of a burst table, 1024-sample Hann frames
// (gfx950, wave64).  The contract is in include/ookiedokie_amd.h ("Burst spectra"), the design in DESIGN.md 4.24.
//
//   frame f of burst b = capture samples [first_b + 1024 f, first_b + 1024 f + 1024), f < F_b = floor(num_b / 1024)
//   power_b[k] = sum_f |X_{b,f}[k]|^2, with the frame transform of spectrum.hip (spectrum_dev.hpp)
//
// The walk.  The cut's coordinate offset_b + 1024 f orders all frames of the capture.  Workgroup g owns the frames
// whose coordinate lies in [g S 1024, (g + 1) S 1024), S = span_frames: it finds the burst that holds its first
// sample by a search over `offset`, as burst_copy_kernel does, and walks on burst by burst.  Of each burst its four
// waves take the frames of the span in turn, one frame per wave at a time, the next frame's loads issued before
// the current one is transformed; a lane folds its fp32 sums into doubles every kSpecFold frames, and at the end of
// the burst (or of the span) the four waves' doubles are added in wave order, as spectrum_kernel does at its end.
//
// What becomes of that sum:
//   - the burst's frames all lie in this span: wave 0 reduces it to the summary (total, DC bins, peak with ties to
//     the lowest k) and stores 40 bytes -- or, with `only`, the workgroup stores the 1024 doubles;
//   - the burst began in an earlier span: row 2 g of `rows`;
//   - the burst begins here and runs on: row 2 g + 1.
// Only the first burst of a span can have begun earlier and only the last can run on, so two rows per span do.
// burst_spectra_rows_kernel, one workgroup per span, looks for the burst that begins in its span and runs on, adds
// that burst's rows in span order and makes the summary: one very long burst is a serial loop over its rows in one
// workgroup.  Every workgroup of the first kernel also keeps the sum of all it did in its row of keyed_rows (four
// bins per thread, added burst after burst by the same thread); burst_keyed_kernel adds the rows in span order.
//
// No atomics, no workgroup waits for another, every sum has a fixed order: a result is a fixed function of the
// capture, the table and S, bit for bit -- and with `only` the same kernels over one burst at the same S repeat the
// sums of that burst in the same order.
//
// Loads.  A burst's first sample is only sample-aligned, so a frame is read with load_frame's sample-by-sample
// form: exactly the frame's 1024 samples, nothing below the burst, beyond it or beyond the capture's n samples
// (burst_frames clips F_b to the samples that exist, whatever the table says).
#include "burst_spectra.hpp"
#include "common.hpp"
#include "spectrum_dev.hpp"

#pragma clang fp contract(off)

namespace ookd {

namespace {

// the last burst in [lo, hi] whose offset is <= s (lo's is): the burst that holds sample s of the cut (bursts.hip)
__device__ __forceinline__ uint64_t spec_burst_of(const BurstDev *table, uint64_t lo, uint64_t hi, uint64_t s) {
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

// F_b, clipped to the whole frames that exist below n
__device__ __forceinline__ uint64_t burst_frames(const BurstDev &e, uint64_t n) {
    if (e.end_offset <= e.offset || e.first_sample >= n) return 0u;
    const uint64_t F = (e.end_offset - e.offset) / (uint64_t)kSpecBins, room = (n - e.first_sample) / (uint64_t)kSpecBins;
    return F < room ? F : room;
}

// frames [fa, fb) of a burst of F frames at `offset` (< hi) have their coordinate in [lo, hi)
__device__ __forceinline__ void span_frames_of(uint64_t offset, uint64_t F, uint64_t lo, uint64_t hi, uint64_t &fa,
                                               uint64_t &fb) {
    fa = offset >= lo ? 0u : (lo - offset + (uint64_t)kSpecBins - 1u) / (uint64_t)kSpecBins;
    fb = (hi - offset + (uint64_t)kSpecBins - 1u) / (uint64_t)kSpecBins;
    if (fb > F) fb = F;
}

// Wave 0 (all 64 lanes): the summary of the 1024 doubles at sd.  Lane L adds bins L + 64 j in j order, then the
// lanes' sums meet in a butterfly; the peak is the largest of bins 2 .. 1022, the lowest k among equals.
__device__ __forceinline__ void summarise(const double *sd, uint32_t lane, uint64_t frames, BurstSpecSummary *out) {
    double sum = 0.0, best = -1.0;
    uint32_t bk = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t k = lane + 64u * j;
        const double v = sd[k];
        sum += v;
        if (k >= 2u && k <= (uint32_t)kSpecBins - 2u && v > best) {
            best = v;
            bk = k;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(sum, m), ob = __shfl_xor(best, m);
        const uint32_t ok = (uint32_t)__shfl_xor((int)bk, m);
        sum = sum + os;
        if (ob > best || (ob == best && ok < bk)) {
            best = ob;
            bk = ok;
        }
    }
    if (lane == 0u) {
        BurstSpecSummary s;
        s.frames = frames;
        s.total = sum;
        s.dc = (sd[kSpecBins - 1] + sd[0]) + sd[1];
        s.peak = best;
        s.peak_bin = bk;
        s.reserved = 0u;
        *out = s;
    }
}

template <int FMT>
__global__ __launch_bounds__(kSpecThreads, kSpecGroupsPerCu) void burst_spectra_kernel(const BurstSpectraParams p,
                                                                                      const uint64_t g0) {
    __shared__ __attribute__((aligned(16))) float2 s_tw[kSpecBins];
    __shared__ __attribute__((aligned(16))) float s_win[kSpecBins];
    __shared__ __attribute__((aligned(16))) float2 s_x[kSpecWaves * kSpecXchg];

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (a scalar: so are the wave's frame numbers)
    const uint64_t g = g0 + blockIdx.x;
    if (g >= p.spans || p.num_bursts == 0u) return;             // (uniform)
    const uint64_t width = (uint64_t)p.span_frames * kSpecBins;
    const uint64_t lo = g * width;
    if (lo >= p.total) return;
    const uint64_t hi = p.total - lo < width ? p.total : lo + width;
    const bool all = p.only == kBurstSpecAll;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.src);

    load_spectrum_tables(s_tw, s_win, p.twiddle, p.window, tid);
    __syncthreads();

    float2 *xw = s_x + wave * kSpecXchg;
    double *sd = reinterpret_cast<double *>(s_x);
    // all this workgroup summed, bins tid + 256 i: kept in its row of keyed_rows between bursts, not in registers
    double *grow = all ? p.keyed_rows + g * (uint64_t)kSpecBins : nullptr;
    bool gfirst = true;

    uint64_t b = all ? spec_burst_of(p.table, 0u, p.num_bursts - 1u, lo) : p.only;
#pragma unroll 1
    for (; b < p.num_bursts; ++b) {
        const BurstDev e = p.table[b];
        if (e.offset >= hi) break;
        const uint64_t F = burst_frames(e, p.n);
        uint64_t fa, fb;
        span_frames_of(e.offset, F, lo, hi, fa, fb);
        if (fa < fb) {
            float pw[16];
            double acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                pw[k] = 0.0f;
                acc[k] = 0.0;
            }
            uint32_t held = 0;
            const unsigned char *bsrc = src + e.first_sample * (uint64_t)sample_bytes((uint32_t)FMT);
            uint64_t f = fa + wave;
            RawFrame<FMT> raw, next;
#pragma unroll
            for (int k = 0; k < RawFrame<FMT>::kWords; ++k) raw.w[k] = next.w[k] = 0u;
            if (f < fb) load_frame<FMT, false>(raw, bsrc, f, lane);
#pragma unroll 1
            for (; f < fb; f += (uint64_t)kSpecWaves) {
                if (f + (uint64_t)kSpecWaves < fb) load_frame<FMT, false>(next, bsrc, f + (uint64_t)kSpecWaves, lane);
                float2 v[16];
                frame_transform<FMT>(raw, v, xw, s_tw, s_win, lane);
                add_frame_power(pw, v);
                if (++held == (uint32_t)kSpecFold) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        acc[k] += (double)pw[k];
                        pw[k] = 0.0f;
                    }
                    held = 0;
                }
                raw = next;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += (double)pw[k];

            // the burst's sum in this span, wave after wave
            __syncthreads();
            for (uint32_t w = 0; w < (uint32_t)kSpecWaves; ++w) {
                if (wave == w) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const uint32_t bin = lane + 64u * (uint32_t)k;
                        sd[bin] = w == 0 ? acc[k] : sd[bin] + acc[k];
                    }
                }
                __syncthreads();
            }
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = sd[tid + 256u * (uint32_t)i];
                if (all) grow[tid + 256u * (uint32_t)i] = gfirst ? x[i] : grow[tid + 256u * (uint32_t)i] + x[i];
            }
            gfirst = false;
            if (fa == 0u && fb == F) {                          // finished here
                if (all) {
                    if (wave == 0u) summarise(sd, lane, F, p.summary + b);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) p.one[tid + 256u * (uint32_t)i] = x[i];
                }
            } else {
                double *row = p.rows + (2u * g + (fa == 0u ? 1u : 0u)) * (uint64_t)kSpecBins;
#pragma unroll
                for (int i = 0; i < 4; ++i) row[tid + 256u * (uint32_t)i] = x[i];
            }
            __syncthreads();                                    // sd is the next burst's exchange region
        }
        if (!all) break;
    }
    if (all && gfirst) {                                        // (bursts of no frames only)
#pragma unroll
        for (int i = 0; i < 4; ++i) grow[tid + 256u * (uint32_t)i] = 0.0;
    }
}

// Workgroup g: the burst that begins in span g and runs on beyond it, if there is one -- its rows in span order,
// then its summary (or, with `only`, its 1024 doubles).
__global__ __launch_bounds__(kSpecThreads) void burst_spectra_rows_kernel(const BurstSpectraParams p, const uint64_t g0) {
    __shared__ double sd[kSpecBins];
    const uint32_t tid = threadIdx.x;
    const uint64_t g = g0 + blockIdx.x;
    if (g >= p.spans || p.num_bursts == 0u) return;             // (uniform, as every return below)
    const uint64_t width = (uint64_t)p.span_frames * kSpecBins;
    const uint64_t lo = g * width;
    if (lo >= p.total) return;
    const uint64_t hi = p.total - lo < width ? p.total : lo + width;
    const bool all = p.only == kBurstSpecAll;
    const uint64_t b = all ? spec_burst_of(p.table, 0u, p.num_bursts - 1u, hi - 1u) : p.only;
    if (b >= p.num_bursts) return;
    const BurstDev e = p.table[b];
    const uint64_t F = burst_frames(e, p.n);
    if (F == 0u || e.offset < lo || e.offset >= hi) return;     // does not begin here
    uint64_t fa, fb;
    span_frames_of(e.offset, F, lo, hi, fa, fb);
    if (fb >= F) return;                                        // finished by the first kernel
    uint64_t g_last = (e.offset + (F - 1u) * (uint64_t)kSpecBins) / width;
    if (g_last >= p.spans) g_last = p.spans - 1u;

    double x[4];
    const double *row = p.rows + (2u * g + 1u) * (uint64_t)kSpecBins;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = row[tid + 256u * (uint32_t)i];
#pragma unroll 4
    for (uint64_t gg = g + 1u; gg <= g_last; ++gg) {
        row = p.rows + 2u * gg * (uint64_t)kSpecBins;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] += row[tid + 256u * (uint32_t)i];
    }
    if (all) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sd[tid + 256u * (uint32_t)i] = x[i];
        __syncthreads();
        if (tid < 64u) summarise(sd, tid, F, p.summary + b);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p.one[tid + 256u * (uint32_t)i] = x[i];
    }
}

// keyed[k] = keyed_rows[0][k] + keyed_rows[1][k] + ... in that order
__global__ __launch_bounds__(kSpecThreads) void burst_keyed_kernel(const double *keyed_rows, double *keyed, uint64_t spans) {
    const uint32_t k = blockIdx.x * kSpecThreads + threadIdx.x;
    const double *col = keyed_rows + k;
    double sum = 0.0;
#pragma unroll 8
    for (uint64_t g = 0; g < spans; ++g) sum += col[g * (uint64_t)kSpecBins];
    keyed[k] = sum;
}

}  // namespace

namespace {

bool params_ok(const BurstSpectraParams &p) {
    return p.span_frames >= kBurstSpecMinSpan && (p.span_frames & (p.span_frames - 1u)) == 0u &&
           p.spans == burst_spec_spans(p.total, p.span_frames) && 2u * p.spans <= kBurstSpecMaxRows;
}

hipError_t launch_first(const BurstSpectraParams &p, uint64_t base, uint32_t count, hipStream_t stream) {
    const dim3 grid(count), block(kSpecThreads);
    switch (p.sample_fmt) {
    case kFmtSc16:
        hipLaunchKernelGGL(burst_spectra_kernel<(int)kFmtSc16>, grid, block, 0, stream, p, base);
        break;
    case kFmtCs8:
        hipLaunchKernelGGL(burst_spectra_kernel<(int)kFmtCs8>, grid, block, 0, stream, p, base);
        break;
    case kFmtCu8:
        hipLaunchKernelGGL(burst_spectra_kernel<(int)kFmtCu8>, grid, block, 0, stream, p, base);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_burst_spectra(const BurstSpectraParams &p, hipEvent_t mid, hipStream_t stream) {
    if (p.spans == 0u || p.num_bursts == 0u || p.total == 0u) return hipSuccess;
    if (!params_ok(p) || p.only != kBurstSpecAll) return hipErrorInvalidValue;
    hipError_t e = launch_first(p, 0u, (uint32_t)p.spans, stream);
    if (e != hipSuccess) return e;
    if (mid && (e = hipEventRecord(mid, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(burst_spectra_rows_kernel, dim3((uint32_t)p.spans), dim3(kSpecThreads), 0, stream, p, (uint64_t)0u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(burst_keyed_kernel, dim3(kSpecBins / kSpecThreads), dim3(kSpecThreads), 0, stream, p.keyed_rows,
                       p.keyed, p.spans);
    return hipGetLastError();
}

hipError_t launch_burst_spectrum_one(const BurstSpectraParams &p, uint64_t first_span, uint64_t num_spans, hipStream_t stream) {
    if (num_spans == 0u) return hipSuccess;
    if (!params_ok(p) || p.only >= p.num_bursts || !p.one || first_span >= p.spans || num_spans > p.spans - first_span) {
        return hipErrorInvalidValue;
    }
    const hipError_t e = launch_first(p, first_span, (uint32_t)num_spans, stream);
    if (e != hipSuccess || num_spans == 1u) return e;
    hipLaunchKernelGGL(burst_spectra_rows_kernel, dim3(1), dim3(kSpecThreads), 0, stream, p, first_span);
    return hipGetLastError();
}

}  // namespace ookd
