// survey_dev.hpp -- device code shared by the envelope survey's kernel files (survey.hip, survey_tuned.hip): the
// slice of every level a tile needs, one sample of any format as float2 (unpack_iq, front_dev.hpp), the bin of an
// output, and the wave's aggregated count.  Compiled with -ffp-contract=off: the power keeps its three roundings.
#pragma once

#include "kernels.hpp"
#include "front_dev.hpp"

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ookd {

constexpr int kPeelRounds = 4;
constexpr size_t kSurveyLdsBudget = 40 * 1024;      // level buffers + histograms: four workgroups per CU

// first index and length of the slice of every level that outputs [j0, j0 + len) of the last level need
// (gen_levels of front_dev.hpp for origin 0)
__host__ __device__ inline void survey_levels(const SurveyParams &p, int64_t j0, uint32_t len, int64_t *a,
                                              uint32_t *n) {
    const int S = (int)p.num_stages;
    a[S] = j0;
    n[S] = len;
    for (int s = S - 1; s >= 0; --s) {
        const int64_t D = p.stage[s].decim;
        const int64_t T = p.stage[s].ntaps;
        a[s] = D * a[s + 1] + (D - 1) - (T - 1);
        n[s] = (uint32_t)(D * ((int64_t)n[s + 1] - 1) + T);
    }
}

#ifdef __HIPCC__
template <int FMT>
__device__ __forceinline__ float2 survey_sample(const void *src, int64_t i) {
    if (FMT == (int)kFmtSc16) return unpack_iq(reinterpret_cast<const uint32_t *>(src)[i]);
    return unpack_iq(widen8<FMT>(reinterpret_cast<const uint16_t *>(src)[i]));
}

__device__ __forceinline__ uint32_t survey_bin(float re, float im) {
    const float rr = re * re;
    const float ii = im * im;
    return level_bin_of_bits(__float_as_uint(rr + ii));
}

// every lane of the wave calls this together
__device__ __forceinline__ void wave_count(uint32_t *wave_hist, bool valid, uint32_t bin) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < kPeelRounds && todo; ++r) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
        const uint64_t same = __ballot(valid && bin == lb) & todo;
        if ((int)lane == leader) atomicAdd(&wave_hist[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&wave_hist[bin], 1u);
}

// tuned_chunk<true, R> (front_dev.hpp) for a lane that accumulates only every STEP-th of its R output positions:
// acc[j] is position j * STEP.  Window position W (newest first) feeds it with tap kk = j * STEP - W when
// 0 <= kk < 16, so every counted output still receives its taps in ascending order, each as the exact packed
// multiply and add; a window position no counted output reads is not loaded.  STEP = 1 is tuned_chunk<true, R>.
template <int R, int STEP, int W, int... Js>
__device__ __forceinline__ void tuned_wstep_strided(v2f *acc, const v2f *tpair, const v2f *base,
                                                    std::integer_sequence<int, Js...>) {
    constexpr int cp = W + kTunedChunk;                 // 1 .. R + 15
    constexpr bool used = ((Js * STEP - W >= 0 && Js * STEP - W < kTunedChunk) || ...);
    if constexpr (used) {
        const v2f x = base[cp + cp / R];
        ((void)((Js * STEP - W >= 0 && Js * STEP - W < kTunedChunk)
                    ? (cmac_tuned<true>(acc[Js], tpair[(Js * STEP - W) & 15], x), 0)
                    : 0),
         ...);
    }
}

// The same for a lane with ONE counted output, position 0 of its R >= 32: tap kk of chunk-from-the-end m reads
// window index R * lane + u, u = 16 (m + 1) - kk, at slot (R + 1) * lane + u + u / R -- 16 m is no multiple of R here,
// so the pad slots in front of u are counted at run time (u is wave-uniform).  lanebase = window + (R + 1) * lane.
template <int R>
__device__ __forceinline__ void tuned_chunk_single(v2f &acc, const v2f *tpair, const v2f *lanebase, uint32_t m) {
#pragma unroll
    for (int kk = 0; kk < kTunedChunk; ++kk) {
        const uint32_t u = (uint32_t)kTunedChunk * (m + 1u) - (uint32_t)kk;
        cmac_tuned<true>(acc, tpair[kk], lanebase[u + u / (uint32_t)R]);
    }
}

template <int R, int STEP, int... Ws>
__device__ __forceinline__ void tuned_chunk_strided(v2f *acc, const v2f *tpair, const v2f *base,
                                                    std::integer_sequence<int, Ws...>) {
    (tuned_wstep_strided<R, STEP, R - 1 - Ws>(acc, tpair, base, std::make_integer_sequence<int, R / STEP>{}), ...);
}
#endif

}  // namespace ookd
