// spectrum.hip -- carrier survey: Welch power spectrum of whole captures, 1024-sample Hann frames (gfx950, wave64).
//
//   unpack (complexf.h:68-77, v / 2048) -> periodic Hann -> X_f[k] = sum_n w[n] x[1024 f + n] e^{-j 2 pi k n / 1024}
//   -> power[k] = sum_f |X_f[k]|^2     (the contract is in include/ookiedokie_amd.h at ookd_spectrum_*)
//
// One wave takes one frame; a workgroup of four waves strides over the frames of its capture.  The frame is read
// with one 16-byte load per lane and quarter (8 bytes for the 8-bit formats; single samples when the capture is
// not 16-byte aligned), so lane L holds samples n = 256 j + 4 L + i, j, i = 0..3.  The next frame's loads are
// issued before the current frame is transformed.  The transform itself -- window, the three steps of the
// 4 x 16 x 16 decimation in frequency, the two LDS exchanges and the table layout -- is spectrum_dev.hpp, shared
// with burst_spectra.hip; lane l ends with bins l + 64 ks.  A counter run over 2^26 samples shows no LDS bank
// conflict cycle.
//
// Sums.  |X|^2 is added to an fp32 sum per lane and bin; after kSpecFold = 32 frames (the header's budget for
// that sum) a lane folds its sums into doubles.  At its end a workgroup adds its four waves' doubles in wave
// order and writes 1024 partials to its row of partial[capture][group][1024] with plain stores;
// spectrum_reduce_kernel adds the rows in group order.  No atomics: a run is a fixed function of the capture
// and the grid, bit for bit.
#include "kernels.hpp"
#include "common.hpp"
#include "spectrum_dev.hpp"

#pragma clang fp contract(off)

namespace ookd {

namespace {

template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(kSpecThreads, kSpecGroupsPerCu) void spectrum_kernel(const SpectrumParams p) {
    __shared__ __attribute__((aligned(16))) float2 s_tw[kSpecBins];
    __shared__ __attribute__((aligned(16))) float s_win[kSpecBins];
    __shared__ __attribute__((aligned(16))) float2 s_x[kSpecWaves * kSpecXchg];

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    const uint32_t cap = blockIdx.y;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);

    load_spectrum_tables(s_tw, s_win, p.twiddle, p.window, tid);
    __syncthreads();

    float2 *xw = s_x + wave * kSpecXchg;

    float pw[16];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        pw[k] = 0.0f;
        acc[k] = 0.0;
    }
    uint32_t held = 0;

    const uint64_t step = (uint64_t)gridDim.x * kSpecWaves;
    uint64_t f = (uint64_t)blockIdx.x * kSpecWaves + wave;
    RawFrame<FMT> raw, next;
#pragma unroll
    for (int k = 0; k < RawFrame<FMT>::kWords; ++k) raw.w[k] = next.w[k] = 0u;
    if (f < p.frames) load_frame<FMT, ALIGNED>(raw, src, f, lane);

#pragma unroll 1
    for (; f < p.frames; f += step) {
        if (f + step < p.frames) load_frame<FMT, ALIGNED>(next, src, f + step, lane);

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

    // the workgroup's sum, wave after wave, then its row of the partials
    __syncthreads();
    double *sd = reinterpret_cast<double *>(s_x);
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
    double *row = p.partial + ((uint64_t)cap * gridDim.x + blockIdx.x) * kSpecBins;
    for (uint32_t i = tid; i < (uint32_t)kSpecBins; i += kSpecThreads) row[i] = sd[i];
}

// power[capture][k] = partial[capture][0][k] + partial[capture][1][k] + ... in that order
__global__ __launch_bounds__(kSpecThreads) void spectrum_reduce_kernel(const double *partial, double *power,
                                                                       uint32_t groups) {
    const uint32_t k = blockIdx.x * kSpecThreads + threadIdx.x;
    const double *col = partial + (uint64_t)blockIdx.y * groups * kSpecBins + k;
    double sum = 0.0;
    for (uint32_t g = 0; g < groups; ++g) sum += col[(uint64_t)g * kSpecBins];
    power[(uint64_t)blockIdx.y * kSpecBins + k] = sum;
}

template <int FMT>
void launch_fmt(const SpectrumParams &p, dim3 grid, hipStream_t stream) {
    if (p.aligned) hipLaunchKernelGGL((spectrum_kernel<FMT, true>), grid, dim3(kSpecThreads), 0, stream, p);
    else hipLaunchKernelGGL((spectrum_kernel<FMT, false>), grid, dim3(kSpecThreads), 0, stream, p);
}

}  // namespace

uint32_t spectrum_groups(uint64_t frames, uint32_t num_captures, int cus) {
    if (frames == 0 || num_captures == 0) return 0;
    // as many workgroups as the device holds at once (three per CU: 46 KiB of LDS each), shared among the captures
    uint64_t gx = ((uint64_t)(cus > 0 ? cus : 1) * kSpecGroupsPerCu + num_captures - 1) / num_captures;
    const uint64_t most = (frames + kSpecWaves - 1) / kSpecWaves;
    if (gx > most) gx = most;
    if (gx < 1) gx = 1;
    return (uint32_t)gx;
}

hipError_t launch_spectrum(const SpectrumParams &p, uint32_t num_captures, uint32_t groups, hipStream_t stream) {
    if (p.frames == 0 || num_captures == 0 || groups == 0) return hipSuccess;
    if (num_captures > 65535u) return hipErrorInvalidValue;
    const dim3 grid(groups, num_captures);
    switch (p.sample_fmt) {
    case kFmtSc16:
        launch_fmt<(int)kFmtSc16>(p, grid, stream);
        break;
    case kFmtCs8:
        launch_fmt<(int)kFmtCs8>(p, grid, stream);
        break;
    case kFmtCu8:
        launch_fmt<(int)kFmtCu8>(p, grid, stream);
        break;
    default:
        return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spectrum_reduce_kernel, dim3(kSpecBins / kSpecThreads, num_captures), dim3(kSpecThreads), 0,
                       stream, p.partial, p.power, groups);
    return hipGetLastError();
}

}  // namespace ookd
