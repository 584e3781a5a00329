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
#endif

}  // namespace ookd
