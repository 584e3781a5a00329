// survey_tuned.hip -- tuned envelope survey, register-blocked form: histogram of the post-filter power of whole
// captures, the filter being the tuned contract's (include/ookiedokie_amd.h at ookd_filter_tuned_taps): complex taps
// c[k] = (re, im) on the raw samples, per tap tuned_step's four statements (front_dev.hpp), then
// p = ar*ar + ai*ai -> bin -> count, exactly as survey.hip counts the untuned filter's output.  A histogram is an
// exact integer function of the capture: an output one ulp off lands in the neighbouring bin, so there is no fused
// multiply-add, no guard band and no matrix core in this file.
//
//   survey_tuned_fir1_kernel<FMT, R> : 1 stage, decimation 1, <= 256 taps (OOKD_SURVEY_TUNED_FIR1): the window,
//                                      tap-chunk load and chunk body fir1_tuned_kernel (fir_tuned.hip) uses, all
//                                      from front_dev.hpp, with the exact packed multiply and add
//                                      (tuned_chunk<true, R>) and the survey's epilogue (survey_dev.hpp)
// Every other shape (OOKD_SURVEY_TUNED_GENERIC) runs survey_kernel<FMT, true>, survey.hip.
//
// Compiled with -ffp-contract=off like every kernel of the library.
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"
#include "survey_dev.hpp"

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr uint64_t kFir1MaxOutputsPerWave = 1ull << 31;         // a wave's 32-bit LDS counters cannot wrap

// bytes of one wave: its window (slot<R> layout) and its 256 counters
template <int R>
__host__ __device__ __forceinline__ uint32_t sv_wave_window_bytes(uint32_t Tp) {
    return fir1_wave_slots<R>(Tp) * (uint32_t)sizeof(float2);
}

// One wavefront = one tile of 64 R outputs at a time, working alone (no workgroup barrier inside the walk): raw
// 16-byte loads (4 SC16Q11 or 8 8-bit samples) -> unpack once into the wave's LDS window -> lane t accumulates
// its R consecutive outputs with the taps in SGPR pairs, 16 complex taps per chunk -> bin per output, one
// wave_count per output slot -> the wave's 256 counters in LDS.  The workgroup is persistent: its waves walk
// the capture's tiles and the counters are flushed once, at the end, as one 64-bit vector atomic per non-zero bin.
// Window slot j <-> input index t0 - Tp + j; an index in front of the capture is the zero history, an index at or
// beyond n is never read (those outputs are not counted).  A capture whose base is not 16-byte aligned takes the
// sample-by-sample loads for every tile, as the first and the last tile of any capture do.
template <int FMT, int R>
__global__ __launch_bounds__(256) void survey_tuned_fir1_kernel(const SurveyParams p, const float *ctaps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    constexpr uint32_t kTile = 64u * R;
    constexpr uint32_t kSpv = FMT == (int)kFmtSc16 ? 4u : 8u;          // samples per 16-byte vector
    constexpr int kRounds = (int)(((kTile + 256u) / kSpv + 63u) / 64u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t waves = blockDim.x >> 6;
    const uint32_t cap = blockIdx.y;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t win_bytes = sv_wave_window_bytes<R>(Tp);
    float2 *lds = reinterpret_cast<float2 *>(smem_raw + wave * win_bytes);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem_raw + waves * win_bytes);
    uint32_t *wave_hist = hist + wave * kLevelBins;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);
    const uint64_t n = p.n_out;                 // decimation 1: outputs = samples
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const uint32_t nvec = (kTile + Tp) / kSpv;  // Tp is a multiple of 16

    for (uint32_t i = lane; i < (uint32_t)kLevelBins; i += 64u) wave_hist[i] = 0u;

    for (uint64_t wt = (uint64_t)blockIdx.x * waves + wave; wt < p.num_tiles; wt += (uint64_t)gridDim.x * waves) {
        const uint64_t t0 = wt * kTile;
        // the window and the counters are private to this wavefront and the LDS executes one wave's accesses in
        // order: only keep the compiler from moving the writes above the reads of the tile before
        wave_lds_fence();
        if (aligned16 && t0 >= Tp && t0 + kTile <= n) {
            const uint4 *src4 = reinterpret_cast<const uint4 *>(src + (t0 - Tp) * sample_bytes((uint32_t)FMT));
            uint4 q[kRounds];
#pragma unroll
            for (int i = 0; i < kRounds; ++i) {
                const uint32_t v = lane + 64u * i;
                if (v < nvec) q[i] = ld_nt4(src4 + v);
            }
#pragma unroll
            for (int i = 0; i < kRounds; ++i) {
                const uint32_t v = lane + 64u * i;
                if (v < nvec) {
                    store_unpacked<FMT, R>(lds, v, q[i]);
                }
            }
        } else {
            for (uint32_t v = lane; v < (kTile + Tp) / 4u; v += 64u) {
                const int64_t g = (int64_t)t0 - (int64_t)Tp + 4 * (int64_t)v;
                float2 *dst = lds + slot<R>(4u * v);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dst[i] = (g + i < 0 || (uint64_t)(g + i) >= n) ? make_float2(0.0f, 0.0f)
                                                                  : survey_sample<FMT>(src, g + i);
            }
        }
        wave_lds_fence();

        // ---- accumulate ------------------------------------------------------
        v2f acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = (v2f){0.0f, 0.0f};
        const uint32_t nchunks = Tp / kTunedChunk;
        for (uint32_t c = 0; c < nchunks; ++c) {
            // 16 complex taps of this chunk -> 16 SGPR pairs (re, im)
            const float *tp = ctaps + 2u * c * kTunedChunk;
            v2f tpair[16];
            load_tap_chunk32(tp, tpair);
            // output r of this lane sits at window index Tp + R*lane + r; tap kc+kk reads
            // Tp + R*lane + r - kc - kk = R*lane + 16*m + (w + 16),  w = r - kk, m = (Tp - kc - 16)/16;
            // R*lane and 16*m are multiples of R (8 or 16), so their pad slots add up separately
            const uint32_t m = nchunks - 1 - c;
            const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(R + 1) * lane + (16u + 16u / R) * m);
            tuned_chunk<true, R>(acc, tpair, base, std::make_integer_sequence<int, R + kTunedChunk - 1>{});
        }

        // ---- bin and count: one wave_count per output slot, all 64 lanes together ----------
        const uint64_t o0 = t0 + (uint64_t)lane * R;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool valid = o0 + r < n;
            wave_count(wave_hist, valid, valid ? survey_bin(acc[r].x, acc[r].y) : 0u);
        }
    }

    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (uint32_t)kLevelBins; b += blockDim.x) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < waves; ++w) sum += hist[w * kLevelBins + b];
        if (sum) atomicAdd(p.hist + (uint64_t)cap * kLevelBins + b, sum);
    }
}

template <int FMT>
const void *fir1_kernel_of(uint32_t R) {
    return R == 16 ? reinterpret_cast<const void *>(&survey_tuned_fir1_kernel<FMT, 16>)
                   : reinterpret_cast<const void *>(&survey_tuned_fir1_kernel<FMT, 8>);
}

}  // namespace

bool survey_tuned_fir1_shape(uint32_t R, uint32_t waves) {
    return (R == 8 || R == 16) && (waves == 1 || waves == 2 || waves == 4);
}

hipError_t launch_survey_tuned_fir1(const SurveyParams &p, const float *ctaps, uint32_t num_captures, uint32_t R,
                                    uint32_t waves, hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    if (!ctaps || !survey_tuned_fir1_shape(R, waves) || p.num_stages != 1 || p.stage[0].decim != 1 || Tp == 0 ||
        Tp > 256u || Tp % kTunedChunk || p.stage[0].ntaps > Tp || p.tile != 64u * R || num_captures > 65535u)
        return hipErrorInvalidValue;
    const void *fn = p.sample_fmt == kFmtSc16 ? fir1_kernel_of<(int)kFmtSc16>(R)
                     : p.sample_fmt == kFmtCs8 ? fir1_kernel_of<(int)kFmtCs8>(R)
                     : p.sample_fmt == kFmtCu8 ? fir1_kernel_of<(int)kFmtCu8>(R) : nullptr;
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)waves * ((R == 16 ? sv_wave_window_bytes<16>(Tp) : sv_wave_window_bytes<8>(Tp)) +
                                        kLevelBins * sizeof(uint32_t));
    hipError_t e = ensure_dynamic_lds(fn, lds);
    if (e != hipSuccess) return e;
    int cus = 0, per_cu = 0;
    e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, (int)(64u * waves), lds);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    // persistent workgroups: what the device holds at once, each wave walking tiles wave-index + k * (all waves)
    const uint64_t groups_of_tiles = (p.num_tiles + waves - 1) / waves;
    uint64_t gx = ((uint64_t)cus * (uint64_t)per_cu + num_captures - 1) / num_captures;
    // a wave walks at most ceil(num_tiles / (gx * waves)) tiles: keep that within what its counters hold
    const uint64_t per_group = kFir1MaxOutputsPerWave / p.tile * waves;
    const uint64_t least = (p.num_tiles + per_group - 1) / per_group;
    if (gx < least) gx = least;
    if (gx > groups_of_tiles) gx = groups_of_tiles;
    if (gx > 0x7fffffffull) return hipErrorInvalidValue;
    SurveyParams pp = p;
    const float *ct = ctaps;
    void *args[] = {&pp, &ct};
    e = hipLaunchKernel(fn, dim3((uint32_t)gx, num_captures), dim3(64u * waves), args, lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace ookd
