// survey_carriers.hip -- tuned envelope survey of several carriers in one pass over a capture, counting every S-th
// output (OOKD_SURVEY_TUNED_MULTI; the contract is in include/ookiedokie_amd.h at ookd_survey_create_carriers):
// carrier k's histogram is survey_tuned_fir1_kernel's (survey_tuned.hip) for nu_k, restricted to the outputs with
// index i = 0 (mod S).  The same rule as in survey_tuned.hip holds here: a histogram is an exact integer function of
// the capture, so there is no guard band, no fused multiply-add and no matrix core in this file.
//
//   survey_tuned_multi_kernel<FMT, R, NOUT> : 1 stage, decimation 1, <= 256 taps.  The window of a tile is read
//                                             and unpacked ONCE (survey_tuned_fir1_kernel's loads, slot<R> layout),
//                                             then the chunk loop runs once per carrier, on the counted outputs
//                                             alone (tuned_chunk_strided, survey_dev.hpp).  R = output positions per
//                                             lane (8, 16; 32 and 64 for S >= R), NOUT = max(1, R / S) = the counted ones.
//
// Compiled with -ffp-contract=off like every kernel of the library.
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"
#include "survey_dev.hpp"

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr uint32_t kWaves = (uint32_t)kSurveyMultiWaves;
// The K x 256 counters are shared by the workgroup's waves (LDS atomics commute).  A workgroup counts at most this
// many outputs per carrier, so that no 32-bit LDS counter can wrap (the launch sizes the grid by it).
constexpr uint64_t kMultiMaxCountedPerGroup = 1ull << 31;

template <int R>
__host__ __device__ __forceinline__ uint32_t svm_wave_window_bytes(uint32_t Tp) {
    return fir1_wave_slots<R>(Tp) * (uint32_t)sizeof(float2);
}

// One wavefront = one tile of 64 R output positions at a time, working alone on a private window (no workgroup
// barrier inside the walk).  Lane t owns positions R t .. R t + R - 1 of the tile; of those it accumulates the NOUT
// counted ones, R t + j * (R / NOUT): NOUT = R / S for S <= R.  For S > R NOUT is 1 and only the lanes with
// R t = 0 (mod S) count theirs.  The tile start is a multiple of 512 and so of S: which positions are counted does
// not depend on the tile.  Window slot j <-> input index t0 - Tp + j; an index in front of the capture is the zero
// history, an index at or beyond n is never read.  A capture whose base is not 16-byte aligned takes the
// sample-by-sample loads for every tile, as the first and the last tile of any capture do.
// LDS: [kWaves windows][K][256 counters]; ctaps: carrier k's Tp pairs at ctaps + 2 Tp k; hist: [capture][K][256].
template <int FMT, int kR, int NOUT>
__global__ __launch_bounds__(64 * kSurveyMultiWaves) void survey_tuned_multi_kernel(const SurveyParams p,
                                                                                    const float *ctaps,
                                                                                    const uint32_t K,
                                                                                    const uint32_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    constexpr uint32_t kTile = 64u * kR;                                // a multiple of every legal stride
    constexpr int kStep = kR / NOUT;
    constexpr uint32_t kSpv = FMT == (int)kFmtSc16 ? 4u : 8u;          // samples per 16-byte vector
    constexpr int kRounds = (int)(((kTile + 256u) / kSpv + 63u) / 64u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t cap = blockIdx.y;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t win_bytes = svm_wave_window_bytes<kR>(Tp);
    float2 *lds = reinterpret_cast<float2 *>(smem_raw + wave * win_bytes);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem_raw + kWaves * win_bytes);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);
    const uint64_t n = p.n_out;                 // decimation 1: outputs = samples
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const uint32_t nvec = (kTile + Tp) / kSpv;  // Tp is a multiple of 16
    const uint32_t nchunks = Tp / kTunedChunk;
    // S > R: this lane's one position is a counted one
    const bool lane_counts = ((kR * lane) & (stride - 1u)) == 0u;

    for (uint32_t i = threadIdx.x; i < K * (uint32_t)kLevelBins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    for (uint64_t wt = (uint64_t)blockIdx.x * kWaves + wave; wt < p.num_tiles; wt += (uint64_t)gridDim.x * kWaves) {
        const uint64_t t0 = wt * kTile;
        // the window is private to this wavefront and the LDS executes one wave's accesses in order: only keep the
        // compiler from moving the writes above the reads of the tile before
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
                    store_unpacked<FMT, kR>(lds, v, q[i]);
                }
            }
        } else {
            for (uint32_t v = lane; v < (kTile + Tp) / 4u; v += 64u) {
                const int64_t g = (int64_t)t0 - (int64_t)Tp + 4 * (int64_t)v;
                float2 *dst = lds + slot<kR>(4u * v);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dst[i] = (g + i < 0 || (uint64_t)(g + i) >= n) ? make_float2(0.0f, 0.0f)
                                                                  : survey_sample<FMT>(src, g + i);
            }
        }
        wave_lds_fence();

        const uint64_t o0 = t0 + (uint64_t)lane * kR;
#pragma nounroll
        for (uint32_t k = 0; k < K; ++k) {
            // ---- accumulate the counted outputs of carrier k ----------------------
            const float *ct = ctaps + (size_t)2u * Tp * k;
            v2f acc[NOUT];
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j] = (v2f){0.0f, 0.0f};
            for (uint32_t c = 0; c < nchunks; ++c) {
                v2f tpair[16];
                load_tap_chunk32(ct + 2u * c * kTunedChunk, tpair);
                // as in survey_tuned_fir1_kernel: position r of this lane sits at window index Tp + R lane + r
                const uint32_t m = nchunks - 1 - c;
                if constexpr (kR >= 32) {
                    static_assert(kR < 32 || NOUT == 1, "the large windows hold one counted output per lane");
                    tuned_chunk_single<kR>(acc[0], tpair, reinterpret_cast<const v2f *>(lds + (uint32_t)(kR + 1) * lane), m);
                } else {
                    const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(kR + 1) * lane + (16u + 16u / kR) * m);
                    tuned_chunk_strided<kR, kStep>(acc, tpair, base, std::make_integer_sequence<int, kR + kTunedChunk - 1>{});
                }
            }
            // ---- bin and count into the workgroup's counters of carrier k ----------
            uint32_t *khist = hist + k * (uint32_t)kLevelBins;
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                const bool valid = o0 + (uint32_t)(j * kStep) < n && (NOUT > 1 || lane_counts);
                wave_count(khist, valid, valid ? survey_bin(acc[j].x, acc[j].y) : 0u);
            }
        }
    }

    __syncthreads();
    for (uint32_t i = threadIdx.x; i < K * (uint32_t)kLevelBins; i += blockDim.x) {
        const unsigned long long sum = hist[i];
        if (sum) atomicAdd(p.hist + (uint64_t)cap * K * kLevelBins + i, sum);
    }
}

// NOUT = max(1, R / S): the counted ones among a lane's R positions
template <int FMT, int R>
const void *multi_kernel_of(uint32_t stride) {
    switch (stride) {
    case 1: return reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, R, R>);
    case 2: return reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, R, R / 2>);
    case 4: return reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, R, R / 4>);
    case 8: return reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, R, R / 8>);
    default: return reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, R, 1>);
    }
}

// R = 32 and 64 exist for S >= R only: one counted output per lane
template <int FMT>
const void *multi_kernel_of(uint32_t R, uint32_t stride) {
    switch (R) {
    case 8: return multi_kernel_of<FMT, 8>(stride);
    case 16: return multi_kernel_of<FMT, 16>(stride);
    case 32: return stride >= 32 ? reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, 32, 1>) : nullptr;
    case 64: return stride >= 64 ? reinterpret_cast<const void *>(&survey_tuned_multi_kernel<FMT, 64, 1>) : nullptr;
    default: return nullptr;
    }
}

template <int... Rs>
size_t svm_window_bytes_of(uint32_t R, uint32_t Tp, std::integer_sequence<int, Rs...>) {
    size_t b = 0;
    ((void)((uint32_t)Rs == R ? (b = svm_wave_window_bytes<Rs>(Tp), 0) : 0), ...);
    return b;
}

}  // namespace

bool survey_multi_shape(uint32_t R, uint32_t stride) {
    return R == 8 || R == 16 || ((R == 32 || R == 64) && stride >= R);
}

hipError_t launch_survey_tuned_multi(const SurveyParams &p, const float *ctaps, uint32_t num_captures, uint32_t K,
                                     uint32_t stride, hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    if (!ctaps || K == 0 || K > (uint32_t)kSurveyMaxCarriers || stride == 0 || stride > (uint32_t)kSurveyMaxStride ||
        (stride & (stride - 1u)) || p.num_stages != 1 || p.stage[0].decim != 1 || Tp == 0 || Tp > 256u ||
        Tp % kTunedChunk || p.stage[0].ntaps > Tp || !survey_multi_shape(p.tile / 64u, stride) || p.tile % 64u || num_captures > 65535u)
        return hipErrorInvalidValue;
    const uint32_t R = p.tile / 64u, kTile = p.tile;
    const void *fn = p.sample_fmt == kFmtSc16 ? multi_kernel_of<(int)kFmtSc16>(R, stride)
                     : p.sample_fmt == kFmtCs8 ? multi_kernel_of<(int)kFmtCs8>(R, stride)
                     : p.sample_fmt == kFmtCu8 ? multi_kernel_of<(int)kFmtCu8>(R, stride) : nullptr;
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)kWaves * svm_window_bytes_of(R, Tp, std::integer_sequence<int, 8, 16, 32, 64>{}) +
                       (size_t)K * kLevelBins * sizeof(uint32_t);
    hipError_t e = ensure_dynamic_lds(fn, lds);
    if (e != hipSuccess) return e;
    int cus = 0, per_cu = 0;
    e = survey_device_cus(&cus);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, (int)(64u * kWaves), lds);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    // persistent workgroups: what the device holds at once, each wave walking tiles wave-index + k * (all waves)
    const uint64_t groups_of_tiles = (p.num_tiles + kWaves - 1) / kWaves;
    uint64_t gx = ((uint64_t)cus * (uint64_t)per_cu + num_captures - 1) / num_captures;
    // a wave walks at most ceil(num_tiles / (gx * waves)) tiles and a tile has at most ceil(tile / S) counted
    // outputs: keep waves * tiles * that within what the workgroup's shared counters hold
    const uint64_t counted_per_tile = (kTile + stride - 1) / stride;
    const uint64_t tiles_per_wave = kMultiMaxCountedPerGroup / (counted_per_tile * kWaves);
    const uint64_t least = (p.num_tiles + tiles_per_wave * kWaves - 1) / (tiles_per_wave * kWaves);
    if (gx < least) gx = least;
    if (gx > groups_of_tiles) gx = groups_of_tiles;
    if (gx > 0x7fffffffull) return hipErrorInvalidValue;
    SurveyParams pp = p;
    const float *ct = ctaps;
    uint32_t kk = K, ss = stride;
    void *args[] = {&pp, &ct, &kk, &ss};
    e = hipLaunchKernel(fn, dim3((uint32_t)gx, num_captures), dim3(64u * kWaves), args, lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace ookd
