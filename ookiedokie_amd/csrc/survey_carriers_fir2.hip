// survey_carriers_fir2.hip -- tuned envelope survey of several carriers in one pass over a capture through TWO
// decimate-by-2 stages (<= 16 and <= 32 taps: the backend default fs128_fs16_dec4), counting every S-th output
// (OOKD_SURVEY_TUNED_MULTI_FIR2; the contract is in include/ookiedokie_amd.h at ookd_survey_create_carriers):
// carrier k's histogram is the tuned contract's for nu_k chained over both stages, restricted to the outputs with
// index i = 0 (mod S).  The rule of survey_carriers.hip holds here: a histogram is an exact integer function of the
// capture, so there is no guard band, no fused multiply-add and no matrix core in this file.
//
//   survey_tuned_multi_fir2_kernel<FMT, NOUT, THIN> : the window of a tile of F = 256 final outputs (4 F + 74 samples
//                                               of the capture at 16 / 32 taps) is read and unpacked ONCE, then per
//                                               carrier stage 0 runs into a per-wave row of stage-0 outputs and
//                                               stage 1 runs on the counted outputs alone.  NOUT = max(1, 4 / S) =
//                                               the counted ones among a lane's four final outputs.  THIN = 32, 64
//                                               (= S): stage 0 computes only the 32 row entries under every
//                                               counted output, 128 / S per lane; THIN = 0: all of them.
//
// Compiled with -ffp-contract=off like every kernel of the library.
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"
#include "survey_dev.hpp"

#pragma clang fp contract(off)

namespace ookd {

namespace {

typedef Fir2Dec4 G;             // fir2_tuned_kernel's tile (fir_tuned.hip): F = 256, R1 = 9, R2 = 4, L0 = 1166 samples
constexpr uint32_t kWaves = (uint32_t)kSurveyMultiWaves;
// as in survey_carriers.hip: what a workgroup may count per carrier, so that no 32-bit LDS counter can wrap
constexpr uint64_t kFir2MaxCountedPerGroup = 1ull << 31;
// Both levels of a wave's window hold float2 here (level 0 is unpacked once for all carriers): sample i of level 0
// at slot i + i / P1, stage-0 output j at slot j + j / P2 of the row -- lane strides P1 + 1 = 19 and P2 + 1 = 9
// float2, conflict free for ds_read_b64.
// The thinned stage 0 (THIN = S = 32, 64) gives a lane 128 / S outputs, so its level 0 pads every P0 = 256 / S samples.
// Its last counted output is F - S, so its window ends with that one's: 4 (F - S) + 78 samples.
constexpr int level0_pad(int thin) { return thin ? 2 * (128 / thin) : G::P1; }
constexpr int level0_len(int thin) { return thin ? 4 * (G::F - thin) + 78 : G::L0; }
constexpr uint32_t slots0(int thin) { return (uint32_t)((level0_len(thin) + level0_len(thin) / level0_pad(thin) + 2 + 1) & ~1); }
constexpr uint32_t kSlots1 = (uint32_t)((G::L1 + G::L1 / G::P2 + 2 + 1) & ~1);
constexpr uint32_t wave_bytes(int thin) { return (slots0(thin) + kSlots1) * (uint32_t)sizeof(float2); }
// complex taps of one carrier: stage 0 padded to T1 pairs, then stage 1 padded to T2 pairs (zero pairs)
constexpr uint32_t kCarrierTapFloats = (uint32_t)kSurveyFir2TapFloats;
static_assert(kSurveyFir2TapFloats == 2 * (G::T1 + G::T2) && G::T1 == kTunedChunk && G::T2 == 2 * kTunedChunk &&
              G::D1 == 2 && G::D2 == 2 && G::F == (int)kSurveyFir2Tile, "the shape survey.cpp lays the taps out for");
// global index of local input sample 0 of the tile that starts at final output 0 (fir2_tuned_kernel's kA0)
constexpr int kA0 = G::D1 * ((G::D2 - 1) - (G::T2 - 1)) + (G::D1 - 1) - (G::T1 - 1);
static_assert(kA0 == -74, "a tile of F outputs reads 4 F + 74 samples at 16 / 32 taps");

// One chunk of 16 complex taps of a decimate-by-D stage for a lane that accumulates every STEP-th of its R output
// positions: acc[j] is position j * STEP.  Window position W (newest first) is the sample at index
// OFF + D (R - 1) - W of the lane's block (OFF = padded taps - 1 - 16 chunk) and feeds position r with tap
// kk = D r - D (R - 1) + W of the chunk when 0 <= kk < 16, so every output receives its taps in ascending order, each
// as the contract's four statements (cmac_tuned<true>).  A window position no counted output reads is not loaded.
template <int D, int R, int STEP, int P, int OFF, int W, int... Js>
__device__ __forceinline__ void fir2s_wstep(v2f *acc, const v2f *tpair, const v2f *base,
                                            std::integer_sequence<int, Js...>) {
    constexpr int c = OFF + D * (R - 1) - W;
    static_assert(c >= 0, "window underflow");
    constexpr bool used = ((D * Js * STEP - D * (R - 1) + W >= 0 && D * Js * STEP - D * (R - 1) + W < kTunedChunk) || ...);
    if constexpr (used) {
        const v2f x = base[c + c / P];
        ((void)((D * Js * STEP - D * (R - 1) + W >= 0 && D * Js * STEP - D * (R - 1) + W < kTunedChunk)
                    ? (cmac_tuned<true>(acc[Js], tpair[(D * Js * STEP - D * (R - 1) + W) & 15], x), 0)
                    : 0),
         ...);
    }
}

template <int D, int R, int STEP, int P, int OFF, int... Ws>
__device__ __forceinline__ void fir2s_chunk(v2f *acc, const float *ct, const v2f *base,
                                            std::integer_sequence<int, Ws...>) {
    v2f tpair[16];
    load_tap_chunk32(ct, tpair);
    (fir2s_wstep<D, R, STEP, P, OFF, Ws>(acc, tpair, base, std::make_integer_sequence<int, R / STEP>{}), ...);
}

// Taps k0 .. k1 - 1 of stage 1 one at a time (a last chunk that is not full): the pairs behind the true tap count are
// padding, and a zero tap on a stage-0 output that is inf or NaN would make a NaN the contract does not have.
// Position r of the lane reads row index (T2 - 1) + D2 r - k of its block.
template <int STEP>
__device__ __forceinline__ void fir2s_stage1_taps(v2f *acc, const float *ct2, const v2f *base, uint32_t k0, uint32_t k1) {
#pragma nounroll
    for (uint32_t k = k0; k < k1; ++k) {
        const v2f tp = {ct2[2u * k], ct2[2u * k + 1u]};
#pragma unroll
        for (int j = 0; j < G::R2 / STEP; ++j) {
            const uint32_t c = (uint32_t)(G::T2 - 1 + G::D2 * j * STEP) - k;
            cmac_tuned<true>(acc[j], tp, base[c + c / (uint32_t)G::P2]);
        }
    }
}

template <int FMT>
__device__ __forceinline__ float2 unpack_lane16(uint32_t w, int e) {
    // sample e of a dword: the SC16Q11 sample itself, or one of its two 8-bit ones
    if (FMT == (int)kFmtSc16) return unpack_iq(w);
    return unpack_iq(widen8<FMT>(e ? (w >> 16) : (w & 0xffffu)));
}

// One wavefront = one tile of F = 256 final outputs at a time, working alone on a private window (no workgroup
// barrier inside the walk).  Final output J0 + j reads stage-0 outputs (local) 2 j + 31 - k2, stage-0 output j1
// (local; global 2 J0 - 30 + j1) reads inputs (local) 2 j1 + 15 - k1; local input 0 is global 4 J0 - 74.  An input
// in front of the capture is the zero history and so is a stage-0 output with a negative global index; an input at or
// beyond n is never read.  Lane t computes stage-0 outputs 9 t .. 9 t + 8 and owns final outputs 4 t .. 4 t + 3, of
// which it accumulates the NOUT = max(1, 4 / S) counted ones; for S > 4 only the lanes with 4 t = 0 (mod S) count
// theirs.  J0 is a multiple of 256 and so of S.  THIN = S = 32, 64: counted output S m reads row entries
// 2 S m .. 2 S m + 31 and nothing else is read by a lane that counts, so the 64 S / 256 lanes t of block
// m = t / (64 S / 256) compute those alone, 128 / S each; the rest of the row is stale and feeds only results that
// are thrown away.  A capture whose base is not 16-byte aligned takes the sample-by-sample loads for every tile, as
// the first and the last tiles of any capture do.
// LDS: [kWaves x (window, row)][K][256 counters]; ctaps: carrier k's pairs at ctaps + 96 k (stage 0: 16 pairs,
// stage 1: 32 pairs); hist: [capture][K][256].  n = samples per capture, ntaps2 = true taps of stage 1.
template <int FMT, int NOUT, int THIN>
__global__ __launch_bounds__(64 * kSurveyMultiWaves) void survey_tuned_multi_fir2_kernel(const SurveyParams p,
                                                                                         const float *ctaps,
                                                                                         const uint32_t K,
                                                                                         const uint32_t stride,
                                                                                         const uint64_t n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    static_assert(THIN == 0 || ((THIN == 32 || THIN == 64) && NOUT == 1), "the thinned stage 0 is for S = 32 and 64");
    constexpr int kStep = G::R2 / NOUT;
    constexpr int kL0 = level0_len(THIN);                               // samples of the window
    constexpr int kP0 = level0_pad(THIN);                               // samples of level 0 between two pad slots
    constexpr int kR1 = THIN ? 128 / THIN : G::R1;                      // stage-0 outputs per lane
    constexpr uint32_t kWaveBytes = wave_bytes(THIN);
    constexpr int kSpd = FMT == (int)kFmtSc16 ? 1 : 2;                  // samples per dword
    constexpr int kSpv = 4 * kSpd;                                      // samples per 16-byte vector
    // the window starts kShift samples into a 16-byte vector in every tile (4 J0 is a multiple of 1024)
    constexpr int kShift = ((kA0 % kSpv) + kSpv) % kSpv;
    constexpr int kVecs = (kL0 + kShift + kSpv - 1) / kSpv;
    constexpr int kRounds = (kVecs + 63) / 64;
    static_assert((FMT == (int)kFmtSc16 ? kShift == 2 : kShift == 6), "where the window starts inside its first vector");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t cap = blockIdx.y;
    float2 *lds0 = reinterpret_cast<float2 *>(smem_raw + wave * kWaveBytes);
    float2 *lds1 = lds0 + slots0(THIN);
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem_raw + kWaves * kWaveBytes);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(p.iq) +
                               (uint64_t)cap * p.cap_stride * sample_bytes((uint32_t)FMT);
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const uint32_t ntaps2 = p.stage[1].ntaps;
    // S > 4: this lane's one position is a counted one
    const bool lane_counts = ((G::R2 * lane) & (stride - 1u)) == 0u;

    for (uint32_t i = threadIdx.x; i < K * (uint32_t)kLevelBins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    for (uint64_t wt = (uint64_t)blockIdx.x * kWaves + wave; wt < p.num_tiles; wt += (uint64_t)gridDim.x * kWaves) {
        const uint64_t J0 = wt * (uint64_t)G::F;
        const int64_t a0 = (int64_t)(G::D1 * G::D2) * (int64_t)J0 + kA0;
        // the window is private to this wavefront and the LDS executes one wave's accesses in order: only keep the
        // compiler from moving the writes above the reads of the tile before
        wave_lds_fence();
        if (aligned16 && a0 >= kShift && (uint64_t)(a0 - kShift) + (uint64_t)(kVecs * kSpv) <= n) {
            const uint4 *src4 = reinterpret_cast<const uint4 *>(src + (uint64_t)(a0 - kShift) * sample_bytes((uint32_t)FMT));
            uint4 q[kRounds];
#pragma unroll
            for (int i = 0; i < kRounds; ++i) {
                const uint32_t v = lane + 64u * i;
                if (64 * (i + 1) <= kVecs || v < (uint32_t)kVecs) q[i] = ld_nt4(src4 + v);
            }
#pragma unroll
            for (int i = 0; i < kRounds; ++i) {
                const uint32_t v = lane + 64u * i;
                if (64 * (i + 1) <= kVecs || v < (uint32_t)kVecs) {
                    const int i0 = kSpv * (int)v - kShift;          // local index of the vector's first sample
                    const uint32_t w4[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
                    for (int e = 0; e < kSpv; ++e) {
                        const int li = i0 + e;
                        if (li >= 0 && li < kL0) lds0[li + li / kP0] = unpack_lane16<FMT>(w4[e / kSpd], e % kSpd);
                    }
                }
            }
        } else {
            for (int li = (int)lane; li < kL0; li += 64) {
                const int64_t g = a0 + li;
                lds0[li + li / kP0] = (g < 0 || (uint64_t)g >= n) ? make_float2(0.0f, 0.0f) : survey_sample<FMT>(src, g);
            }
        }
        wave_lds_fence();

        const uint64_t o0 = J0 + (uint64_t)lane * G::R2;
        // this lane's first stage-0 output: its row index, and its global index
        const uint32_t j1 = THIN ? 2u * THIN * (lane / (THIN / 4u)) + (uint32_t)kR1 * (lane % (THIN / 4u)) : (uint32_t)kR1 * lane;
        const int64_t g1 = (int64_t)G::D2 * (int64_t)J0 + (G::D2 - 1) - (G::T2 - 1) + (int64_t)j1;
#pragma nounroll
        for (uint32_t k = 0; k < K; ++k) {
            const float *ct1 = ctaps + (size_t)kCarrierTapFloats * k, *ct2 = ct1 + 2 * G::T1;
            // ---- stage 0 of carrier k: this lane -> row entries j1 .. j1 + kR1 - 1 (2 j1 is a multiple of kP0) ----
            {
                v2f a1[kR1];
#pragma unroll
                for (int r = 0; r < kR1; ++r) a1[r] = (v2f){0.0f, 0.0f};
                fir2s_chunk<G::D1, kR1, 1, kP0, G::T1 - 1>(a1, ct1, reinterpret_cast<const v2f *>(lds0 + 2u * j1 + 2u * j1 / (uint32_t)kP0),
                                                           std::make_integer_sequence<int, G::D1 * (kR1 - 1) + kTunedChunk>{});
                // the row is read by the stage 1 of the carrier before: wave-private, in order
                wave_lds_fence();
#pragma unroll
                for (int r = 0; r < kR1; ++r) {
                    const uint32_t j = j1 + (uint32_t)r;
                    lds1[j + j / (uint32_t)G::P2] = g1 + r < 0 ? make_float2(0.0f, 0.0f) : make_float2(a1[r].x, a1[r].y);
                }
            }
            wave_lds_fence();
            // ---- stage 1 on the counted outputs: whole chunks unrolled, the rest tap by tap --------
            v2f acc[NOUT];
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j] = (v2f){0.0f, 0.0f};
            const v2f *row = reinterpret_cast<const v2f *>(lds1 + (G::P2 + 1) * lane);
            if (ntaps2 >= (uint32_t)kTunedChunk)
                fir2s_chunk<G::D2, G::R2, kStep, G::P2, G::T2 - 1>(acc, ct2, row,
                                                                   std::make_integer_sequence<int, G::D2 * (G::R2 - 1) + kTunedChunk>{});
            else
                fir2s_stage1_taps<kStep>(acc, ct2, row, 0u, ntaps2);
            if (ntaps2 >= 2u * (uint32_t)kTunedChunk)
                fir2s_chunk<G::D2, G::R2, kStep, G::P2, G::T2 - 1 - kTunedChunk>(acc, ct2 + 2 * kTunedChunk, row,
                                                                                 std::make_integer_sequence<int, G::D2 * (G::R2 - 1) + kTunedChunk>{});
            else if (ntaps2 > (uint32_t)kTunedChunk)
                fir2s_stage1_taps<kStep>(acc, ct2, row, (uint32_t)kTunedChunk, ntaps2);
            // ---- bin and count into the workgroup's counters of carrier k ----------
            uint32_t *khist = hist + k * (uint32_t)kLevelBins;
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                const bool valid = o0 + (uint32_t)(j * kStep) < p.n_out && (NOUT > 1 || lane_counts);
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

// NOUT = max(1, 4 / S): the counted ones among a lane's four final outputs; thin: stage 0 thinned for S = 32, 64
template <int FMT>
const void *fir2_kernel_of(uint32_t stride, bool thin) {
    switch (stride) {
    case 1: return reinterpret_cast<const void *>(&survey_tuned_multi_fir2_kernel<FMT, 4, 0>);
    case 2: return reinterpret_cast<const void *>(&survey_tuned_multi_fir2_kernel<FMT, 2, 0>);
    case 32: if (thin) return reinterpret_cast<const void *>(&survey_tuned_multi_fir2_kernel<FMT, 1, 32>); break;
    case 64: if (thin) return reinterpret_cast<const void *>(&survey_tuned_multi_fir2_kernel<FMT, 1, 64>); break;
    default: break;
    }
    return reinterpret_cast<const void *>(&survey_tuned_multi_fir2_kernel<FMT, 1, 0>);
}

}  // namespace

hipError_t launch_survey_tuned_multi_fir2(const SurveyParams &p, const float *ctaps, uint32_t num_captures, uint32_t K,
                                          uint32_t stride, uint64_t n, bool thin, hipStream_t stream) {
    if (p.num_tiles == 0 || num_captures == 0) return hipSuccess;
    if (!ctaps || K == 0 || K > (uint32_t)kSurveyMaxCarriers || stride == 0 || stride > (uint32_t)kSurveyMaxStride ||
        (stride & (stride - 1u)) || p.num_stages != 2 || p.stage[0].decim != 2 || p.stage[1].decim != 2 ||
        p.stage[0].ntaps == 0 || p.stage[0].ntaps > (uint32_t)G::T1 || p.stage[1].ntaps == 0 ||
        p.stage[1].ntaps > (uint32_t)G::T2 || p.tile != kSurveyFir2Tile || p.n_out != n / 4u ||
        p.num_tiles != (p.n_out + kSurveyFir2Tile - 1) / kSurveyFir2Tile || num_captures > 65535u)
        return hipErrorInvalidValue;
    thin = thin && stride >= 32u;
    const void *fn = p.sample_fmt == kFmtSc16 ? fir2_kernel_of<(int)kFmtSc16>(stride, thin)
                     : p.sample_fmt == kFmtCs8 ? fir2_kernel_of<(int)kFmtCs8>(stride, thin)
                     : p.sample_fmt == kFmtCu8 ? fir2_kernel_of<(int)kFmtCu8>(stride, thin) : nullptr;
    if (!fn) return hipErrorInvalidValue;
    const uint32_t wbytes = !thin ? wave_bytes(0) : stride == 32u ? wave_bytes(32) : wave_bytes(64);
    const size_t lds = (size_t)kWaves * wbytes + (size_t)K * kLevelBins * sizeof(uint32_t);
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
    const uint64_t counted_per_tile = (kSurveyFir2Tile + stride - 1) / stride;
    const uint64_t tiles_per_wave = kFir2MaxCountedPerGroup / (counted_per_tile * kWaves);
    const uint64_t least = (p.num_tiles + tiles_per_wave * kWaves - 1) / (tiles_per_wave * kWaves);
    if (gx < least) gx = least;
    if (gx > groups_of_tiles) gx = groups_of_tiles;
    if (gx > 0x7fffffffull) return hipErrorInvalidValue;
    SurveyParams pp = p;
    const float *ct = ctaps;
    uint32_t kk = K, ss = stride;
    uint64_t nn = n;
    void *args[] = {&pp, &ct, &kk, &ss, &nn};
    e = hipLaunchKernel(fn, dim3((uint32_t)gx, num_captures), dim3(64u * kWaves), args, lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace ookd
