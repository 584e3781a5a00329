// survey_tuned.hip -- tuned envelope survey: histogram of the post-filter power of whole captures, the filter being
// the tuned contract's (include/ookiedokie_amd.h at ookd_filter_tuned_taps): complex taps c[k] = (re, im) on the raw
// samples, per tap and in this order, float32, unfused, tap 0 on the newest sample, accumulators from +0:
//     ar = ar + re[k]*xr;   ar = ar - im[k]*xi;
//     ai = ai + re[k]*xi;   ai = ai + im[k]*xr;
// then p = ar*ar + ai*ai -> bin -> count, exactly as survey.hip counts the untuned filter's output.  A histogram
// is an exact integer function of the capture: an output one ulp off lands in the neighbouring bin, so there is
// no fused multiply-add, no guard band and no matrix core anywhere in this file.
//
//   survey_tuned_generic_kernel<FMT> : survey_kernel (survey.hip) with the four statements and (re, im) tap pairs
//                                      in LDS: any shape (OOKD_SURVEY_TUNED_GENERIC)
//   survey_tuned_fir1_kernel<FMT, R> : 1 stage, decimation 1, <= 256 taps (OOKD_SURVEY_TUNED_FIR1): the shape of
//                                      fir1_tuned_kernel (fir_tuned.hip) with the exact packed multiply and add of
//                                      fir1_bits_kernel<true, .> (kernels.hip) and the survey's epilogue
//
// Compiled with -ffp-contract=off like every kernel of the library.
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"
#include "survey_dev.hpp"

#include <utility>

#pragma clang fp contract(off)

namespace ookd {

namespace {

constexpr int kGenThreads = 256;
constexpr int kGenWaves = kGenThreads / 64;
constexpr uint64_t kGenMaxTilesPerGroup = 1ull << 20;   // x 1024 outputs: a 32-bit LDS counter cannot wrap
constexpr uint64_t kFir1MaxOutputsPerWave = 1ull << 31;         // each wave has counters of its own: the same

// One tap of the contract, four statements in order.
__device__ __forceinline__ void tuned_step_exact(float &ar, float &ai, float cr, float ci, float2 x) {
    ar = ar + cr * x.x;
    ar = ar - ci * x.y;
    ai = ai + cr * x.y;
    ai = ai + ci * x.x;
}

// ---------------------------------------------------------------------------------------------------------
// any shape: survey_kernel's structure
// ---------------------------------------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(kGenThreads) void survey_tuned_generic_kernel(const SurveyParams p, const float *ctaps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem_raw + p.lds_hist_off);
    float2 *ltaps = reinterpret_cast<float2 *>(smem_raw + p.lds_taps_off);

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)p.num_stages;            // >= 1: a tuned survey has a filter
    uint32_t *wave_hist = hist + (tid >> 6) * kLevelBins;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);

    for (uint32_t i = tid; i < (uint32_t)(kGenWaves * kLevelBins); i += kGenThreads) hist[i] = 0u;
    for (uint32_t i = tid; i < p.num_taps; i += kGenThreads) ltaps[i] = make_float2(ctaps[2 * i], ctaps[2 * i + 1]);
    __syncthreads();

    for (uint64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t j0 = (int64_t)(tile * p.tile);
        const uint64_t left = p.n_out - (uint64_t)j0;
        const uint32_t len = left < p.tile ? (uint32_t)left : p.tile;
        int64_t a[kMaxStages + 1];
        uint32_t n[kMaxStages + 1];
        survey_levels(p, j0, len, a, n);
        // level 0: index a[0] + n[0] - 1 = D (j0 + len) - 1 < D n_out <= samples in the capture
        for (uint32_t i = tid; i < n[0]; i += kGenThreads) {
            const int64_t g = a[0] + (int64_t)i;
            lds[i] = g < 0 ? make_float2(0.0f, 0.0f) : survey_sample<FMT>(src, g);
        }
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const float2 *in = lds + ((s & 1) ? p.lds_b_off : 0u);
            float2 *out = lds + ((s & 1) ? 0u : p.lds_b_off);
            const float2 *taps = ltaps + p.stage[s].tap_off;
            const int64_t D = p.stage[s].decim;
            const uint32_t T = p.stage[s].ntaps;
            const bool last = (s == S - 1);
            const uint32_t cnt = n[s + 1];
            for (uint32_t base = 0; base < cnt; base += kGenThreads) {
                const uint32_t i = base + tid;
                const bool valid = i < cnt;
                float ar = 0.0f, ai = 0.0f;
                if (valid) {
                    // output a[s+1] + i reads level-s inputs D i + T - 1 - k of the slice (survey_kernel)
                    const float2 *x0 = in + ((uint32_t)D * i + T - 1u);
#pragma unroll 4
                    for (uint32_t k = 0; k < T; ++k) {
                        const float2 c = taps[k];
                        tuned_step_exact(ar, ai, c.x, c.y, x0[-(int)k]);
                    }
                }
                if (!last) {
                    // outputs in front of the capture do not exist: the next stage's history is zero there
                    if (valid) out[i] = (a[s + 1] + (int64_t)i) < 0 ? make_float2(0.0f, 0.0f) : make_float2(ar, ai);
                } else {
                    wave_count(wave_hist, valid, valid ? survey_bin(ar, ai) : 0u);
                }
            }
            __syncthreads();
        }
    }

    __syncthreads();
    {
        uint32_t sum = 0;
        for (int w = 0; w < kGenWaves; ++w) sum += hist[w * kLevelBins + tid];
        if (sum) atomicAdd(p.hist + (uint64_t)cap * kLevelBins + tid, (unsigned long long)sum);
    }
}

// ---------------------------------------------------------------------------------------------------------
// 1 stage, decimation 1, <= 256 taps: register-blocked, exact order
// ---------------------------------------------------------------------------------------------------------

// acc(re, im) += c * x for one complex tap c = tp (re, im) held in an SGPR pair, every product and every sum
// rounded on its own -- the four statements, two components at a time:
//   (ar, ai) = (ar, ai) + (re, re) * (xr, xi)          op_sel_hi:[0,1]: both halves read tp.lo
//   (ar, ai) = (ar, ai) + (-im, im) * (xi, xr)         both halves read tp.hi, x's halves swapped, the low
//                                                      product negated: x + (-y) is x - y bit for bit
// so ar receives re*xr first and im*xi second, ai re*xi first and im*xr second.
__device__ __forceinline__ void cmac_tuned_exact(v2f &acc, v2f tp, v2f x) {
    v2f p1, p2;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(p1) : "s"(tp), "v"(x));
    asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(p1));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[1,0]" : "=v"(p2) : "s"(tp), "v"(x));
    asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(p2));
}

// Compile-time unrolled body of one 16-tap chunk (tuned_wstep / tuned_chunk of fir_tuned.hip): window position W
// (newest first) feeds output r with tap kk = r - W when 0 <= kk < 16, so every output receives its taps in
// ascending order.
template <int R, int W, int... Rs>
__device__ __forceinline__ void sv_wstep(v2f *acc, const v2f *tpair, const v2f *base, std::integer_sequence<int, Rs...>) {
    constexpr int cp = W + kSurveyTunedChunk;           // 1 .. R + 15
    const v2f x = base[cp + cp / R];
    ((void)((Rs - W >= 0 && Rs - W < kSurveyTunedChunk) ? (cmac_tuned_exact(acc[Rs], tpair[(Rs - W) & 15], x), 0) : 0),
     ...);
}

template <int R, int... Ws>
__device__ __forceinline__ void sv_chunk(v2f *acc, const v2f *tpair, const v2f *base, std::integer_sequence<int, Ws...>) {
    (sv_wstep<R, R - 1 - Ws>(acc, tpair, base, std::make_integer_sequence<int, R>{}), ...);
}

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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
                    float2 *dst = lds + slot<R>(kSpv * v);     // 4 or 8 slots, never straddle a pad (R is 8 or 16)
                    if (FMT == (int)kFmtSc16) {
                        dst[0] = unpack_iq(q[i].x);
                        dst[1] = unpack_iq(q[i].y);
                        dst[2] = unpack_iq(q[i].z);
                        dst[3] = unpack_iq(q[i].w);
                    } else {
                        dst[0] = unpack_iq(widen8<FMT>(q[i].x & 0xffffu));
                        dst[1] = unpack_iq(widen8<FMT>(q[i].x >> 16));
                        dst[2] = unpack_iq(widen8<FMT>(q[i].y & 0xffffu));
                        dst[3] = unpack_iq(widen8<FMT>(q[i].y >> 16));
                        dst[4] = unpack_iq(widen8<FMT>(q[i].z & 0xffffu));
                        dst[5] = unpack_iq(widen8<FMT>(q[i].z >> 16));
                        dst[6] = unpack_iq(widen8<FMT>(q[i].w & 0xffffu));
                        dst[7] = unpack_iq(widen8<FMT>(q[i].w >> 16));
                    }
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- accumulate ------------------------------------------------------
        v2f acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = (v2f){0.0f, 0.0f};
        const uint32_t nchunks = Tp / kSurveyTunedChunk;
        for (uint32_t c = 0; c < nchunks; ++c) {
            // 16 complex taps of this chunk -> 16 SGPR pairs (re, im)
            const float *tp = ctaps + 2u * c * kSurveyTunedChunk;
            v8f ta, tb, tc, td;
            asm volatile("s_load_dwordx8 %0, %4, 0x0\n\t"
                         "s_load_dwordx8 %1, %4, 0x20\n\t"
                         "s_load_dwordx8 %2, %4, 0x40\n\t"
                         "s_load_dwordx8 %3, %4, 0x60\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&s"(ta), "=&s"(tb), "=&s"(tc), "=&s"(td)
                         : "s"(tp)
                         : "memory");
            const v2f tpair[16] = {
                __builtin_shufflevector(ta, ta, 0, 1), __builtin_shufflevector(ta, ta, 2, 3),
                __builtin_shufflevector(ta, ta, 4, 5), __builtin_shufflevector(ta, ta, 6, 7),
                __builtin_shufflevector(tb, tb, 0, 1), __builtin_shufflevector(tb, tb, 2, 3),
                __builtin_shufflevector(tb, tb, 4, 5), __builtin_shufflevector(tb, tb, 6, 7),
                __builtin_shufflevector(tc, tc, 0, 1), __builtin_shufflevector(tc, tc, 2, 3),
                __builtin_shufflevector(tc, tc, 4, 5), __builtin_shufflevector(tc, tc, 6, 7),
                __builtin_shufflevector(td, td, 0, 1), __builtin_shufflevector(td, td, 2, 3),
                __builtin_shufflevector(td, td, 4, 5), __builtin_shufflevector(td, td, 6, 7)};
            // output r of this lane sits at window index Tp + R*lane + r; tap kc+kk reads
            // Tp + R*lane + r - kc - kk = R*lane + 16*m + (w + 16),  w = r - kk, m = (Tp - kc - 16)/16;
            // R*lane and 16*m are multiples of R (8 or 16), so their pad slots add up separately
            const uint32_t m = nchunks - 1 - c;
            const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(R + 1) * lane + (16u + 16u / R) * m);
            sv_chunk<R>(acc, tpair, base, std::make_integer_sequence<int, R + kSurveyTunedChunk - 1>{});
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

hipError_t device_cus(int *cus) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    return hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
}

}  // namespace

bool survey_tuned_fir1_shape(uint32_t R, uint32_t waves) {
    return (R == 8 || R == 16) && (waves == 1 || waves == 2 || waves == 4);
}

hipError_t launch_survey_tuned_generic(const SurveyParams &p, const float *ctaps, uint32_t num_captures,
                                       size_t lds_bytes, hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    if (!ctaps || p.num_stages == 0) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = device_cus(&cus);
    if (e != hipSuccess) return e;
    // as launch_survey: as many workgroups as fit the device at once, each walking its share and flushing once
    uint64_t per_cu = (160 * 1024) / lds_bytes;
    if (per_cu > 2048 / kGenThreads) per_cu = 2048 / kGenThreads;
    if (per_cu < 1) per_cu = 1;
    uint64_t gx = ((uint64_t)cus * per_cu + num_captures - 1) / num_captures;
    const uint64_t least = (p.num_tiles + kGenMaxTilesPerGroup - 1) / kGenMaxTilesPerGroup;
    if (gx < least) gx = least;
    if (gx > p.num_tiles) gx = p.num_tiles;
    if (gx > 0x7fffffffull || num_captures > 65535u) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)gx, num_captures);
    switch (p.sample_fmt) {
    case kFmtSc16:
        hipLaunchKernelGGL(survey_tuned_generic_kernel<(int)kFmtSc16>, grid, dim3(kGenThreads), lds_bytes, stream, p, ctaps);
        break;
    case kFmtCs8:
        hipLaunchKernelGGL(survey_tuned_generic_kernel<(int)kFmtCs8>, grid, dim3(kGenThreads), lds_bytes, stream, p, ctaps);
        break;
    case kFmtCu8:
        hipLaunchKernelGGL(survey_tuned_generic_kernel<(int)kFmtCu8>, grid, dim3(kGenThreads), lds_bytes, stream, p, ctaps);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_survey_tuned_fir1(const SurveyParams &p, const float *ctaps, uint32_t num_captures, uint32_t R,
                                    uint32_t waves, hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    if (!ctaps || !survey_tuned_fir1_shape(R, waves) || p.num_stages != 1 || p.stage[0].decim != 1 || Tp == 0 ||
        Tp > 256u || Tp % kSurveyTunedChunk || p.stage[0].ntaps > Tp || p.tile != 64u * R || num_captures > 65535u)
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
    e = device_cus(&cus);
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
