// fir_tuned.hip -- frequency-tuned front end: one FIR with COMPLEX taps on the raw samples.
//
// The slicer only looks at |y|, and
//     | sum_k h[k] x[n-k] e^{-j 2 pi nu (n-k)} |  =  | sum_k (h[k] e^{+j 2 pi nu k}) x[n-k] |,
// so "mix the carrier at nu cycles per sample down, then low-pass with h" has the envelope of one FIR with
// taps c[k] = h[k] e^{j 2 pi nu k}: no oscillator, no phase state -- a capture, a chunk or a shard may start
// anywhere.  The taps come from the host (ookd_filter_tuned_taps, the contract in include/ookiedokie_amd.h) as
// (re, im) pairs; stage s of a decimating chain is tuned to nu times the decimation before it.
//
// The contract's arithmetic of one stage output (float32, unfused, tap 0 on the newest sample, from +0) is
// tuned_step's four statements (front_dev.hpp).  With im == 0 every extra term is +-0: nu = 0 is the reference's
// result.
//
//   fir1_tuned_kernel        : 1 stage, decimation 1, <= 256 taps (OOKD_FRONT_TUNED_FIR1): fused packed FMAs
//                              (tuned_chunk<false, R>, front_dev.hpp), guard band and epilogue of fir1_tile_finish,
//                              recompute in the contract's order
//   fir1_tuned_multi_kernel  : the same shape for K carriers in one pass over the capture (OOKD_FRONT_TUNED_MULTI):
//                              loads, quiet statistics and unpack once per tile, accumulation and epilogue per carrier
//   fir2_tuned_kernel        : 2 stages of decimation 2, <= 16 and <= 32 taps, on request (OOKD_FRONT_TUNED_FIR2):
//                              fir2_bits_kernel's tile (kernels.hip) with complex taps -- level 0 raw in LDS, level 1
//                              float2, fused packed FMAs in both stages, quiet test, guard band, recompute in the
//                              contract's order from the raw window
//   fir_tuned_generic_kernel : the contract for every shape (OOKD_FRONT_TUNED_GENERIC)
//
// Compiled with -ffp-contract=off (see kernels.hip).
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"

#include <hip/hip_ext.h>

#pragma clang fp contract(off)

namespace ookd {

// The contract's value of one output (guard-band path): sequential, unfused.
template <int R>
__device__ __noinline__ float2 fir1_tuned_exact_output(const float2 *lds, uint32_t j_out, const float *ctaps,
                                                       uint32_t ntaps) {
    float ar = 0.0f, ai = 0.0f;
    for (uint32_t k = 0; k < ntaps; ++k) tuned_step(ar, ai, ctaps[2 * k], ctaps[2 * k + 1], lds[slot<R>(j_out - k)]);
    return make_float2(ar, ai);
}

// One wavefront = one tile of 64 R outputs, working alone, as in fir1_bits_kernel: raw loads -> quiet test ->
// unpack ONCE into the wave's LDS window (slot<R>: lane stride R + 1 float2, conflict free for ds_read_b64) ->
// register-blocked packed FMAs with the taps in SGPRs -> threshold, guard band, bit words, tile info.
// A chunk of 16 complex taps costs a lane R + 15 LDS reads for 32 R packed FMAs -- per FMA no more than the
// real-tap kernel's R + 31 reads for 32 R.
template <int R>
__global__ __launch_bounds__(64) void fir1_tuned_kernel(const FrontParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    constexpr uint32_t kTile = 64u * R;                 // outputs per wavefront
    constexpr int kRounds = (kTile + 256 + 255) / 256;  // 16 B loads per lane (taps <= 256)
    static_assert(kTile / 4 >= 64, "the first load round is a full one");
    const uint32_t tid = threadIdx.x & 63u;
    const uint32_t cap = blockIdx.y;
    const uint64_t t0 = ((uint64_t)blockIdx.x + p.tile_base) * kTile;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);
    uint64_t *words = p.bits + (uint64_t)cap * p.words_per_cap;

    // ---- load the wave's window: slot j <-> input index t0 - Tp + j ------------
    const uint32_t nvec = (kTile + Tp) >> 2;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const bool interior = aligned16 && t0 >= Tp && t0 + kTile <= p.n_valid;
    if (interior) {
        const uint4 *src4 = reinterpret_cast<const uint4 *>(src + (t0 - Tp));
        uint4 q[kRounds];
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            // (a lane without a vector in this round repeats its first one: the quiet test takes minima too)
            q[i] = (64u * (i + 1) <= kTile / 4 || v < nvec) ? ld_nt4(src4 + v) : q[0];
        }
        // ---- quiet test ----------------------------------------------------------
        // A carrier beside 0 Hz comes with a DC term at 0 Hz, so "every sample is small" never holds.  For any
        // constant d:  y = sum_k c[k] (x[n-k] - d) + d sum_k c[k],  hence
        //     |y| <= max|x - d| sum|c[k]| + |d| |sum c[k]|
        // -- the window's spread against all the taps, its offset against the filter's response at 0 Hz only
        // (the stop band of a tuned filter).  d = the midpoint of the window's component ranges:
        // max|x - d| <= sqrt(2) a / 2, |d| <= sqrt(2) b / 2 with a = the larger range, b = the larger
        // |min + max|.  The host folds the taps' sums, the threshold and the float chain's own rounding into
        // quiet_a / quiet_b (rx.cpp: setup_tuned_quiet); interior windows hold capture samples only.
        if (!p.fir_out && p.quiet_lsb > 0) {
            v2s mx = (v2s){-32768, -32768}, mn = (v2s){32767, 32767};
#pragma unroll
            for (int i = 0; i < kRounds; ++i) {
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].x), as_v2s(q[i].y)));
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].z), as_v2s(q[i].w)));
                mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].x), as_v2s(q[i].y)));
                mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].z), as_v2s(q[i].w)));
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                mx = __builtin_elementwise_max(mx, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mx), d)));
                mn = __builtin_elementwise_min(mn, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mn), d)));
            }
            const int ri = (int)mx.x - (int)mn.x, rq = (int)mx.y - (int)mn.y;
            const int si = abs((int)mx.x + (int)mn.x), sq = abs((int)mx.y + (int)mn.y);
            const float a = (float)max(ri, rq), b = (float)max(si, sq);
            if (a * p.quiet_a + b * p.quiet_b < 1.0f) {
                // (sparse output: nothing is stored -- see fir1_bits_kernel)
                if (!p.sparse) {
                    if (tid < kTile / 64) words[(t0 >> 6) + tid] = 0;
                    if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + t0 / kTile] = 0;
                }
                if (p.quiet_count && tid == 0) atomicAdd(p.quiet_count + (blockIdx.x % kQuietCounters), 1u);
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            if (64u * (i + 1) <= kTile / 4 || v < nvec) {
                store_unpacked<(int)kFmtSc16, R>(lds, v, q[i]);
            }
        }
    } else {
        // first / last tiles of a capture, halo, unaligned host pointers
        for (uint32_t v = tid; v < nvec; v += 64) {
            const int64_t n = (int64_t)t0 - (int64_t)Tp + 4 * (int64_t)v;
            float2 *dst = lds + slot<R>(4 * v);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i] = fetch_sample(p, src, nullptr, n + i);
        }
    }
    // the window is private to this wavefront and the LDS executes one wave's accesses in order
    wave_lds_fence();

    // ---- accumulate ----------------------------------------------------------
    v2f acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = (v2f){0.0f, 0.0f};
    const uint32_t nchunks = Tp / kTunedChunk;
    for (uint32_t c = 0; c < nchunks; ++c) {
        // 16 complex taps of this chunk -> 16 SGPR pairs (re, im)
        const float *tp = p.ctaps + 2u * c * kTunedChunk;
        v2f tpair[16];
        load_tap_chunk32(tp, tpair);
        // output r of this lane sits at window index Tp + R*tid + r; tap kc+kk reads
        // Tp + R*tid + r - kc - kk = R*tid + 16*m + (w + 16),  w = r - kk, m = (Tp - kc - 16)/16;
        // R*tid and 16*m are multiples of R (8 or 16), so their pad slots add up separately
        const uint32_t m = nchunks - 1 - c;
        const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(R + 1) * tid + (16u + 16u / R) * m);
        tuned_chunk<false, R>(acc, tpair, base, std::make_integer_sequence<int, R + kTunedChunk - 1>{});
    }

    const uint32_t info = fir1_tile_finish<false, R>(p, acc, t0, tid, cap, words, [&](uint32_t r) {
        return fir1_tuned_exact_output<R>(lds, Tp + R * tid + r, p.ctaps, p.stage[0].ntaps);
    });
    if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + t0 / kTile] = info;
}

// ---------------------------------------------------------------------------
// K carriers in one pass: fir1_tuned_kernel's tile with everything that does not depend on nu done once
// ---------------------------------------------------------------------------
// The three nu-independent steps of an interior window, as fir1_tuned_kernel spells them inline.  (That kernel keeps
// its own text: with only its load and unpack rounds routed through these functions both of its listings came out
// different -- same length, other instruction order and registers -- and its instruction stream is what
// profiles/tuned_rate.json measured.  The statistics here also end in SGPRs, which its listing does not have.)
template <int R, int ROUNDS>
__device__ __forceinline__ void tuned_window_load(const uint4 *src4, uint32_t tid, uint32_t nvec, uint4 (&q)[ROUNDS]) {
    constexpr uint32_t kTile = 64u * R;
#pragma unroll
    for (int i = 0; i < ROUNDS; ++i) {
        const uint32_t v = tid + 64u * i;
        // (a lane without a vector in this round repeats its first one: the quiet statistics take minima too)
        q[i] = (64u * (i + 1) <= kTile / 4 || v < nvec) ? ld_nt4(src4 + v) : q[0];
    }
}

// a = the larger component range, b = the larger |min + max| of the window (raw LSB), the same in every lane
template <int ROUNDS>
__device__ __forceinline__ void tuned_window_stats(const uint4 (&q)[ROUNDS], float &a, float &b) {
    v2s mx = (v2s){-32768, -32768}, mn = (v2s){32767, 32767};
#pragma unroll
    for (int i = 0; i < ROUNDS; ++i) {
        mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].x), as_v2s(q[i].y)));
        mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].z), as_v2s(q[i].w)));
        mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].x), as_v2s(q[i].y)));
        mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].z), as_v2s(q[i].w)));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        mx = __builtin_elementwise_max(mx, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mx), d)));
        mn = __builtin_elementwise_min(mn, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mn), d)));
    }
    const int ri = (int)mx.x - (int)mn.x, rq = (int)mx.y - (int)mn.y;
    const int si = abs((int)mx.x + (int)mn.x), sq = abs((int)mx.y + (int)mn.y);
    // (every lane holds the same two numbers: one copy in SGPRs keeps the per-carrier tests off the vector unit's
    //  divergence handling)
    a = (float)__builtin_amdgcn_readfirstlane(max(ri, rq));
    b = (float)__builtin_amdgcn_readfirstlane(max(si, sq));
}

template <int R, int ROUNDS>
__device__ __forceinline__ void tuned_window_unpack(float2 *lds, uint32_t tid, uint32_t nvec, const uint4 (&q)[ROUNDS]) {
    constexpr uint32_t kTile = 64u * R;
#pragma unroll
    for (int i = 0; i < ROUNDS; ++i) {
        const uint32_t v = tid + 64u * i;
        if (64u * (i + 1) <= kTile / 4 || v < nvec) store_unpacked<(int)kFmtSc16, R>(lds, v, q[i]);
    }
}

// carrier k's table entry (wave-uniform, 32 bytes) -> SGPRs, as load_tap_chunk32 fetches the taps
__device__ __forceinline__ TunedCarrierDev load_carrier(const TunedCarrierDev *tab, uint32_t k) {
    static_assert(sizeof(TunedCarrierDev) == 32, "one s_load_dwordx8");
    v8f e;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(e)
                 : "s"(tab + k)
                 : "memory");
    TunedCarrierDev c;
    c.tap_off = __builtin_bit_cast(uint32_t, e[0]);
    c.p_star = e[1];
    c.p_lo = e[2];
    c.p_hi = e[3];
    c.quiet_a = e[4];
    c.quiet_b = e[5];
    c.pad[0] = c.pad[1] = 0;
    return c;
}

// One wavefront = one tile of 64 R outputs of EVERY carrier: the capture is read, tested and unpacked once, then the
// chunk loop and the epilogue of fir1_tuned_kernel run once per carrier that is not quiet in this tile, on the same
// LDS window and in the same accumulators.  Carrier k's bit words, tile infos and floats live where capture k's
// would (the edge / state machine chain runs a batch of K); the grid is (tiles, 1).
template <int R>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(R == kFir1RShort ? 8 : 5)))
void fir1_tuned_multi_kernel(const FrontParams p, const TunedCarrierDev *tab,
                                                              const uint32_t K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    constexpr uint32_t kTile = 64u * R;                 // outputs per wavefront
    constexpr int kRounds = (kTile + 256 + 255) / 256;  // 16 B loads per lane (taps <= 256)
    static_assert(kTile / 4 >= 64, "the first load round is a full one");
    const uint32_t tid = threadIdx.x & 63u;
    const uint64_t tile = (uint64_t)blockIdx.x + p.tile_base;
    const uint64_t t0 = tile * kTile;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq);
    float2 *lds = reinterpret_cast<float2 *>(smem_raw);

    // ---- load the wave's window: slot j <-> input index t0 - Tp + j ------------
    const uint32_t nvec = (kTile + Tp) >> 2;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const bool interior = aligned16 && t0 >= Tp && t0 + kTile <= p.n_valid;
    uint32_t quiet = 0;                                 // bit k: carrier k cannot reach its threshold in this tile
    if (interior) {
        uint4 q[kRounds];
        tuned_window_load<R>(reinterpret_cast<const uint4 *>(src + (t0 - Tp)), tid, nvec, q);
        // ---- quiet test: fir1_tuned_kernel's bound, the window's statistics once, the weights per carrier ----
        if (!p.fir_out && p.quiet_lsb > 0) {
            float a, b;
            tuned_window_stats(q, a, b);
#pragma nounroll
            for (uint32_t k = 0; k < K; ++k) {
                const TunedCarrierDev c = load_carrier(tab, k);
                if (a * c.quiet_a + b * c.quiet_b < 1.0f) {
                    quiet |= 1u << k;
                    // (sparse output: nothing is stored -- see fir1_bits_kernel)
                    if (!p.sparse) {
                        if (tid < kTile / 64) p.bits[(uint64_t)k * p.words_per_cap + (t0 >> 6) + tid] = 0;
                        if (tid == 0) p.tile_info[(uint64_t)k * p.tiles_per_cap + tile] = 0;
                    }
                }
            }
            // (window, carrier) pairs that skipped the filter
            if (quiet && p.quiet_count && tid == 0) atomicAdd(p.quiet_count + (blockIdx.x % kQuietCounters), (uint32_t)__popc(quiet));
            if (quiet == (1u << K) - 1u) return;        // K <= 16
        }
        tuned_window_unpack<R>(lds, tid, nvec, q);
    } else {
        // first / last tiles of a capture, unaligned host pointers
        for (uint32_t v = tid; v < nvec; v += 64) {
            const int64_t n = (int64_t)t0 - (int64_t)Tp + 4 * (int64_t)v;
            float2 *dst = lds + slot<R>(4 * v);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i] = fetch_sample(p, src, nullptr, n + i);
        }
    }
    // the window is private to this wavefront and the LDS executes one wave's accesses in order; from here on it
    // is only read
    wave_lds_fence();

    const uint32_t nchunks = Tp / kTunedChunk;
#pragma nounroll
    for (uint32_t k = 0; k < K; ++k) {
        if ((quiet >> k) & 1u) continue;
        const TunedCarrierDev c = load_carrier(tab, k);
        const float *ctaps = p.ctaps + c.tap_off;
        // ---- accumulate: fir1_tuned_kernel's chunk loop on this carrier's taps ----
        v2f acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = (v2f){0.0f, 0.0f};
        for (uint32_t ch = 0; ch < nchunks; ++ch) {
            v2f tpair[16];
            load_tap_chunk32(ctaps + 2u * ch * kTunedChunk, tpair);
            const uint32_t m = nchunks - 1 - ch;
            const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(R + 1) * tid + (16u + 16u / R) * m);
            tuned_chunk<false, R>(acc, tpair, base, std::make_integer_sequence<int, R + kTunedChunk - 1>{});
        }
        // ---- its own band, bit words, float plane and tile info ----
        FrontParams pk = p;
        pk.p_star = c.p_star;
        pk.p_lo = c.p_lo;
        pk.p_hi = c.p_hi;
        uint64_t *words = p.bits + (uint64_t)k * p.words_per_cap;
        const uint32_t info = fir1_tile_finish<false, R>(pk, acc, t0, tid, k, words, [&](uint32_t r) {
            return fir1_tuned_exact_output<R>(lds, Tp + R * tid + r, ctaps, p.stage[0].ntaps);
        });
        if (tid == 0) p.tile_info[(uint64_t)k * p.tiles_per_cap + tile] = info;
    }
}

// ---------------------------------------------------------------------------
// two decimate-by-2 stages (the backend default fs128_fs16_dec4), fused: fir2_bits_kernel's tile with complex taps
// ---------------------------------------------------------------------------
// One wavefront = one tile of G::F final outputs, working alone, in Fir2Geom's LDS layout (front_dev.hpp): level 0
// stays raw (4 B per sample, lane stride P1 + 1), stage 1 leaves the L1 level-1 outputs stage 2 needs as float2
// (lane stride P2 + 1).  Stage output J reads inputs D (J + 1) - 1 - k; tap k of a chunk of 16 complex taps sits in
// one SGPR pair, every output receives its taps in ascending order (the contract's), fused: two v_pk_fma_f32 per
// sample-tap (cmac_tuned<false>).  tuned_guard_error over both stages bounds what that differs from the contract by.
__device__ __forceinline__ v2f tuned2_sample(const v2f *base, int i) { return base[i]; }
__device__ __forceinline__ v2f tuned2_sample(const uint32_t *base, int i) {        // the raw SC16Q11 level
    const float2 v = unpack_iq(base[i]);
    return (v2f){v.x, v.y};
}

// Window position W (newest first) feeds output r with tap kk = D r - D (R - 1) + W of the chunk when 0 <= kk < 16.
template <int D, int R, int P, int CHUNK_OFF, int W, typename In, int... Rs>
__device__ __forceinline__ void tuned2_wstep(v2f *acc, const v2f *tpair, const In *base,
                                             std::integer_sequence<int, Rs...>) {
    // sample index inside the lane's window: c = Tpad - 1 + D (R - 1) - 16 chunk - W
    constexpr int c = CHUNK_OFF + D * (R - 1) - W;
    static_assert(c >= 0, "window underflow");
    const v2f x = tuned2_sample(base, c + c / P);
    ((void)((D * Rs - D * (R - 1) + W >= 0 && D * Rs - D * (R - 1) + W < kTunedChunk)
                ? (cmac_tuned<false>(acc[Rs], tpair[(D * Rs - D * (R - 1) + W) & 15], x), 0)
                : 0),
     ...);
}

// chunk CH of a stage's taps (16 pairs at ct + 32 CH): tap k = 16 CH + kk of output r reads window sample
// (TPAD - 1) + D r - k
template <int D, int R, int P, int TPAD, int CH, typename In, int... Ws>
__device__ __forceinline__ void tuned2_chunk(v2f *acc, const float *ct, const In *base, std::integer_sequence<int, Ws...>) {
    v2f tpair[16];
    load_tap_chunk32(ct + 2 * kTunedChunk * CH, tpair);
    (tuned2_wstep<D, R, P, TPAD - 1 - kTunedChunk * CH, Ws>(acc, tpair, base, std::make_integer_sequence<int, R>{}), ...);
}

template <int D, int R, int P, int TPAD, typename In, int... CHs>
__device__ __forceinline__ void tuned2_stage(v2f *acc, const float *ct, const In *base, std::integer_sequence<int, CHs...>) {
    (tuned2_chunk<D, R, P, TPAD, CHs>(acc, ct, base, std::make_integer_sequence<int, D * (R - 1) + kTunedChunk>{}), ...);
}

// The contract's value of one final output (guard-band path): the ntaps2 level-1 values it reads, each from the raw
// level-0 window, then stage 2 -- tuned_step's four statements per tap per stage.  `j` = final output inside the tile.
template <typename G>
__device__ __noinline__ float2 fir2_tuned_exact_output(const uint32_t *lds0, const float *ct1, uint32_t ntaps1,
                                                       const float *ct2, uint32_t ntaps2, uint32_t j) {
    float ar2 = 0.0f, ai2 = 0.0f;
    for (uint32_t k2 = 0; k2 < ntaps2; ++k2) {
        const uint32_t j1 = G::D2 * j + (G::T2 - 1) - k2;               // local level-1 index
        float ar1 = 0.0f, ai1 = 0.0f;
        for (uint32_t k1 = 0; k1 < ntaps1; ++k1) {
            const uint32_t i = G::D1 * j1 + (G::T1 - 1) - k1;           // local input index
            tuned_step(ar1, ai1, ct1[2 * k1], ct1[2 * k1 + 1], unpack_iq(lds0[i + i / G::P1]));
        }
        tuned_step(ar2, ai2, ct2[2 * k2], ct2[2 * k2 + 1], make_float2(ar1, ai1));
    }
    return make_float2(ar2, ai2);
}

template <typename G>
__global__ __launch_bounds__(64) void fir2_tuned_kernel(const FrontParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    static_assert(G::T1 == kTunedChunk && G::T2 % kTunedChunk == 0, "whole chunks of complex taps");
    const uint32_t tid = threadIdx.x & 63u;
    const uint32_t cap = blockIdx.y;
    const uint64_t J0 = ((uint64_t)blockIdx.x + p.tile_base) * G::F;       // first final output
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    uint32_t *lds0 = reinterpret_cast<uint32_t *>(smem_raw);               // raw I,Q pairs
    float2 *lds1 = reinterpret_cast<float2 *>(lds0 + G::slots0);
    uint64_t *words = p.bits + (uint64_t)cap * p.words_per_cap;
    const float *ct1 = p.ctaps + 2u * p.stage[0].tap_off, *ct2 = p.ctaps + 2u * p.stage[1].tap_off;

    // global index of local input sample 0: D1 j1_0 + D1 - 1 - (T1 - 1) with j1_0 = D2 J0 + D2 - 1 - (T2 - 1).  J0 is
    // a multiple of F, so the window starts the same kShift samples into a 16-byte vector in every tile and the
    // vectors end with the window
    constexpr int kA0 = G::D1 * ((G::D2 - 1) - (G::T2 - 1)) + (G::D1 - 1) - (G::T1 - 1);
    constexpr int kShift = ((kA0 % 4) + 4) % 4;
    constexpr int kVecs = (G::L0 + kShift) / 4;
    constexpr int kRounds = (kVecs + 63) / 64;
    static_assert((G::D1 * G::D2 * G::F) % 4 == 0 && (G::L0 + kShift) % 4 == 0 && kShift == 2 && kVecs >= 64,
                  "the window is whole vectors but for its first two samples; the first load round is a full one");
    const int64_t a0 = (int64_t)(G::D1 * G::D2) * (int64_t)J0 + kA0;

    // ---- load + quiet test + store raw (as in fir2_bits_kernel, the test as in fir1_tuned_kernel) ----------
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const bool interior = aligned16 && a0 >= kShift && (uint64_t)(a0 + G::L0) <= p.n_valid;
    if (interior) {
        const uint4 *src4 = reinterpret_cast<const uint4 *>(src + (a0 - kShift));
        uint4 q[kRounds];
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            // (a lane without a vector in this round repeats its first one: the quiet test takes minima too)
            q[i] = (64 * (i + 1) <= kVecs || v < (uint32_t)kVecs) ? ld_nt4(src4 + v) : q[0];
        }
        // ---- quiet test: fir1_tuned_kernel's bound over both stages --------------------------------------------
        // For any constant d:  y1 = sum c1 (x - d) + d C1,  y2 = sum c2 (y1 - d C1) + d C1 C2,  hence
        //     |y2| <= A1 A2 max|x - d| + |C1| |C2| |d|
        // with A_s = sum |c_s[k]| and C_s = sum c_s[k]: the window's spread against all the taps, its offset against
        // the chain's response at 0 Hz only.  The host folds the sums, the threshold and the float chains' rounding
        // into quiet_a / quiet_b (front_plan.cpp: tuned_quiet_weights2); a, b as in fir1_tuned_kernel, over the L0
        // samples of the window (the first vector's first two samples lie in front of it).
        if (!p.fir_out && p.quiet_lsb > 0) {
            uint4 f = q[0];
            if (tid == 0) f.x = f.y = f.z;
            v2s mx = __builtin_elementwise_max(__builtin_elementwise_max(as_v2s(f.x), as_v2s(f.y)),
                                               __builtin_elementwise_max(as_v2s(f.z), as_v2s(f.w)));
            v2s mn = __builtin_elementwise_min(__builtin_elementwise_min(as_v2s(f.x), as_v2s(f.y)),
                                               __builtin_elementwise_min(as_v2s(f.z), as_v2s(f.w)));
#pragma unroll
            for (int i = 1; i < kRounds; ++i) {
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].x), as_v2s(q[i].y)));
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].z), as_v2s(q[i].w)));
                mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].x), as_v2s(q[i].y)));
                mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].z), as_v2s(q[i].w)));
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                mx = __builtin_elementwise_max(mx, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mx), d)));
                mn = __builtin_elementwise_min(mn, as_v2s(__shfl_xor(__builtin_bit_cast(uint32_t, mn), d)));
            }
            const int ri = (int)mx.x - (int)mn.x, rq = (int)mx.y - (int)mn.y;
            const int si = abs((int)mx.x + (int)mn.x), sq = abs((int)mx.y + (int)mn.y);
            const float a = (float)max(ri, rq), b = (float)max(si, sq);
            if (a * p.quiet_a + b * p.quiet_b < 1.0f) {
                // (sparse output: nothing is stored -- see fir2_bits_kernel)
                if (!p.sparse) {
                    if (tid < G::F / 64) words[(J0 >> 6) + tid] = 0;
                    if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + J0 / G::F] = 0;
                }
                if (p.quiet_count && tid == 0) atomicAdd(p.quiet_count + (blockIdx.x % kQuietCounters), 1u);
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            if (64 * (i + 1) <= kVecs || v < (uint32_t)kVecs) {
                const int i0 = 4 * (int)v - kShift;                 // local index of q[i].x
                const uint32_t w4[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int li = i0 + e;
                    if (li >= 0) lds0[li + li / G::P1] = w4[e];
                }
            }
        }
    } else {
        // first / last tiles, halo, unaligned pointers: values outside the capture are zeros or the previous shard's
        // samples -- all of them int16, so the level stays raw
        for (int li = (int)tid; li < G::L0; li += 64) lds0[li + li / G::P1] = fetch_raw(p, src, a0 + li);
    }
    // both windows are private to this wavefront and the LDS executes one wave's accesses in order
    wave_lds_fence();

    // ---- stage 1: lane t -> local level-1 outputs R1 t .. R1 t + R1 - 1 ------------------------------------------
    {
        v2f acc[G::R1];
#pragma unroll
        for (int r = 0; r < G::R1; ++r) acc[r] = (v2f){0.0f, 0.0f};
        tuned2_stage<G::D1, G::R1, G::P1, G::T1>(acc, ct1, lds0 + (G::P1 + 1) * tid, std::make_integer_sequence<int, G::N1>{});
#pragma unroll
        for (int r = 0; r < G::R1; ++r) {
            const int j = G::R1 * (int)tid + r;
            lds1[j + j / G::P2] = make_float2(acc[r].x, acc[r].y);
        }
    }
    wave_lds_fence();

    // ---- stage 2: lane t -> final outputs J0 + R2 t .. + R2 - 1 --------------------------------------------------
    v2f acc[G::R2];
#pragma unroll
    for (int r = 0; r < G::R2; ++r) acc[r] = (v2f){0.0f, 0.0f};
    tuned2_stage<G::D2, G::R2, G::P2, G::T2>(acc, ct2, reinterpret_cast<const v2f *>(lds1 + (G::P2 + 1) * tid),
                                             std::make_integer_sequence<int, G::N2>{});

    // ---- threshold, guard band, pack: R2 bits per lane, 64 / R2 lanes per word (fir2_bits_kernel's epilogue) ------
    static_assert(G::R2 == 4, "bit packing below assumes 4 outputs per lane");
    const uint64_t o0 = J0 + (uint64_t)tid * G::R2;
    uint32_t nib = 0;
    float2 *fout = p.fir_out ? reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out : nullptr;
#pragma unroll
    for (int r = 0; r < G::R2; ++r) {
        const bool valid = o0 + r < p.n_out;
        const float pw = power_ref(acc[r].x, acc[r].y);
        bool bit = pw >= p.p_hi;
        if (valid && !bit && pw >= p.p_lo) {
            // inside the guard band: redo this output in the contract's order
            const float2 y = fir2_tuned_exact_output<G>(lds0, ct1, p.stage[0].ntaps, ct2, p.stage[1].ntaps, G::R2 * tid + r);
            bit = power_ref(y.x, y.y) >= p.p_star;
            if (p.recompute_count) atomicAdd(p.recompute_count, 1ull);
        }
        nib |= ((valid && bit) ? 1u : 0u) << r;
        if (fout && valid) fout[o0 + r] = make_float2(acc[r].x, acc[r].y);
    }
    {
        // level changes inside the tile, as in the 1-stage kernels
        const uint32_t keep = o0 >= p.n_out ? 0u : (o0 + G::R2 <= p.n_out ? (uint32_t)G::R2 : (uint32_t)(p.n_out - o0));
        const uint32_t prev_top = __shfl_up(nib >> (G::R2 - 1), 1);
        uint32_t ch = (nib ^ (nib << 1)) & ((1u << G::R2) - 2u);
        if (tid != 0) ch |= (nib ^ prev_top) & 1u;
        ch &= (1u << keep) - 1u;
        uint32_t cnt = __popc(ch);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(nib & 1u));
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)((nib >> (G::R2 - 1)) & 1u), 63);
        const uint64_t chl = __ballot(ch != 0);         // (the word that holds the first change: R2 bits per lane)
        const uint32_t widx = chl ? ((uint32_t)__builtin_ctzll(chl) * (uint32_t)G::R2) >> 6 : 0u;
        if (tid == 0) {
            p.tile_info[(uint64_t)cap * p.tiles_per_cap + J0 / G::F] =
                cnt | (widx << kTileWordShift) | (first << 30) | (last << 31) | p.stamp_bits;
        }
    }
    uint32_t half = nib << (4u * (tid & 7u));
    half |= __shfl_xor(half, 1);
    half |= __shfl_xor(half, 2);
    half |= __shfl_xor(half, 4);                // lanes 8g..8g+7 hold outputs 32g..32g+31
    const uint32_t hi = __shfl_down(half, 8);
    if ((tid & 15u) == 0) words[(J0 >> 6) + (tid >> 4)] = (uint64_t)half | ((uint64_t)hi << 32);
}

// ---------------------------------------------------------------------------
// any shape, the contract's order throughout: fir_generic_kernel (kernels.hip) with complex taps
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fir_tuned_generic_kernel(const FrontParams p, uint32_t lds_b_off, uint32_t tile) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *buf[2] = {reinterpret_cast<float2 *>(smem_raw), reinterpret_cast<float2 *>(smem_raw) + lds_b_off};

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)p.num_stages;
    const int64_t j0 = (int64_t)blockIdx.x * tile;
    GenLevel lv[kMaxStages + 1];
    int64_t off[kMaxStages];
    gen_levels(p, j0, tile, lv, off);

    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    for (uint32_t i = tid; i < lv[0].len; i += 256) buf[0][i] = fetch_sample(p, src, nullptr, lv[0].a + (int64_t)i);
    __syncthreads();

    uint64_t *words = p.bits ? p.bits + (uint64_t)cap * p.words_per_cap : nullptr;
    float2 *fout = p.fir_out ? reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out : nullptr;

    for (int s = 0; s < S; ++s) {
        const float2 *in = buf[s & 1];
        float2 *out = buf[(s + 1) & 1];
        const float *ct = p.ctaps + 2u * p.stage[s].tap_off;
        const int64_t D = p.stage[s].decim;
        const uint32_t T = p.stage[s].ntaps;
        const bool last = (s == S - 1);
        const uint32_t n = lv[s + 1].len;
        for (uint32_t base = 0; base < n; base += 256) {
            const uint32_t i = base + tid;
            float ar = 0.0f, ai = 0.0f;
            if (i < n) {
                const int64_t jl = lv[s + 1].a + (int64_t)i;
                const int64_t newest = D * jl + off[s] - lv[s].a;   // index into `in`
                for (uint32_t k = 0; k < T; ++k) tuned_step(ar, ai, ct[2 * k], ct[2 * k + 1], in[newest - (int64_t)k]);
            }
            if (!last) {
                if (i < n) out[i] = make_float2(ar, ai);
            } else {
                const int64_t o = j0 + (int64_t)i;
                const bool valid = (i < n) && o >= 0 && (uint64_t)o < p.n_out;
                const bool bit = valid && (power_ref(ar, ai) >= p.p_star);
                const uint64_t ball = __ballot(bit);
                // (a tile below 256 outputs is one round: the waves past it own no word)
                if (words && lane_id() == 0 && base + (tid & ~63u) < tile) words[((uint64_t)j0 + base + (tid & ~63u)) >> 6] = ball;
                if (fout && valid) fout[o] = make_float2(ar, ai);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// outputs per lane: as the real-tap kernel -- small tiles only pay through the quiet shortcut
static int tuned_R(const FrontParams &p) { return p.quiet_lsb > 0 ? kFir1RShort : kFir1RLong; }

static size_t tuned_lds_bytes(const FrontParams &p) {
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t slots = tuned_R(p) == kFir1RShort ? fir1_wave_slots<kFir1RShort>(Tp) : fir1_wave_slots<kFir1RLong>(Tp);
    return (size_t)slots * sizeof(float2);
}

bool front_uses_tuned_fir1(const FrontParams &p) {
    // (the load rounds cover a tap history of up to 256 samples, as in fir1_bits_kernel)
    return p.tune == 1 && p.ctaps && p.num_stages == 1 && p.stage[0].decim == 1 && p.origin == 0 && !p.iq_f32 &&
           !p.halo_f32 && p.stage[0].ntaps_pad <= 256u;
}

uint32_t tuned_fir1_tile_bits(const FrontParams &p) { return 64u * (uint32_t)tuned_R(p); }

hipError_t launch_front_tuned_fir1(const FrontParams &p, uint32_t num_captures, hipStream_t stream, hipEvent_t t0,
                                   hipEvent_t t1, uint64_t tile_begin, uint64_t tile_count) {
    if (!front_uses_tuned_fir1(p) || p.sample_fmt != kFmtSc16) return hipErrorInvalidValue;
    const int R = tuned_R(p);
    // whole 4096-output blocks, so every bit word of the capture is written
    const uint64_t all = (p.n_out + kFirTile - 1) / kFirTile * (kFirTile / (64 * R));
    const uint64_t b = tile_begin < all ? tile_begin : all;
    const uint64_t grid = tile_count < all - b ? tile_count : all - b;
    if (grid == 0) return hipSuccess;
    FrontParams pp = p;
    pp.tile_base = (uint32_t)b;
    void *args[] = {&pp};
    const void *fn = R == kFir1RShort ? reinterpret_cast<const void *>(&fir1_tuned_kernel<kFir1RShort>)
                                      : reinterpret_cast<const void *>(&fir1_tuned_kernel<kFir1RLong>);
    const size_t lds = tuned_lds_bytes(p);
    hipError_t e = ensure_dynamic_lds(fn, lds);
    if (e != hipSuccess) return e;
    e = hipExtLaunchKernel(fn, dim3((uint32_t)grid, num_captures), dim3(64), args, lds, stream, t0, t1, 0);
    return e != hipSuccess ? e : hipGetLastError();
}

bool front_uses_tuned_fir2(const FrontParams &p) {
    // use_fir2's shape (kernels.hip: every level's phase is D - 1 when the origin is a multiple of the total
    // decimation), tuned, asked for, and not forced to the contract's order (tune == 2)
    static_assert(Fir2Dec4::T1 == 16 && Fir2Dec4::T2 == 32, "tuned_fir2_shape's tap counts");
    return p.tune == 1 && p.tuned_fir2 && p.ctaps && !p.iq_f32 && !p.halo_f32 &&
           tuned_fir2_shape(p.stage, p.num_stages) && p.origin % 4 == 0;
}

hipError_t launch_front_tuned_fir2(const FrontParams &p, uint32_t num_captures, hipStream_t stream, hipEvent_t t0,
                                   hipEvent_t t1, uint64_t tile_begin, uint64_t tile_count) {
    static_assert(kTunedFir2Tile == (uint32_t)Fir2Dec4::F, "the tile front_tile_bits reports");
    if (!front_uses_tuned_fir2(p) || p.sample_fmt != kFmtSc16) return hipErrorInvalidValue;
    const uint64_t all = (p.n_out + Fir2Dec4::F - 1) / Fir2Dec4::F;
    const uint64_t b = tile_begin < all ? tile_begin : all;
    const uint64_t grid = tile_count < all - b ? tile_count : all - b;
    if (grid == 0) return hipSuccess;
    FrontParams pp = p;
    pp.tile_base = (uint32_t)b;
    void *args[] = {&pp};
    const void *fn = reinterpret_cast<const void *>(&fir2_tuned_kernel<Fir2Dec4>);
    const hipError_t e = hipExtLaunchKernel(fn, dim3((uint32_t)grid, num_captures), dim3(64), args, Fir2Dec4::wave_bytes,
                                            stream, t0, t1, 0);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_front_tuned_multi(const FrontParams &p, const TunedCarrierDev *carriers, uint32_t num_carriers,
                                    hipStream_t stream, hipEvent_t t0, hipEvent_t t1, uint64_t tile_begin,
                                    uint64_t tile_count) {
    if (!front_uses_tuned_fir1(p) || p.sample_fmt != kFmtSc16 || p.halo || !carriers || num_carriers == 0 ||
        num_carriers > kMaxCarriers) {
        return hipErrorInvalidValue;
    }
    const int R = tuned_R(p);
    // whole 4096-output blocks, so every bit word of every carrier is written
    const uint64_t all = (p.n_out + kFirTile - 1) / kFirTile * (kFirTile / (64 * R));
    const uint64_t b = tile_begin < all ? tile_begin : all;
    const uint64_t grid = tile_count < all - b ? tile_count : all - b;
    if (grid == 0) return hipSuccess;
    FrontParams pp = p;
    pp.tile_base = (uint32_t)b;
    void *args[] = {&pp, &carriers, &num_carriers};
    const void *fn = R == kFir1RShort ? reinterpret_cast<const void *>(&fir1_tuned_multi_kernel<kFir1RShort>)
                                      : reinterpret_cast<const void *>(&fir1_tuned_multi_kernel<kFir1RLong>);
    const size_t lds = tuned_lds_bytes(p);
    hipError_t e = ensure_dynamic_lds(fn, lds);
    if (e != hipSuccess) return e;
    e = hipExtLaunchKernel(fn, dim3((uint32_t)grid, 1), dim3(64), args, lds, stream, t0, t1, 0);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_front_tuned_generic(const FrontParams &p, uint32_t num_captures, hipStream_t stream) {
    if (!p.tune || !p.ctaps || p.iq_f32 || p.halo_f32 || p.sample_fmt != kFmtSc16) return hipErrorInvalidValue;
    // the tile and its level buffers, as launch_front_generic (the levels hold float2 samples whatever the taps are)
    const GenTile g = generic_tile(p.stage, p.num_stages);
    if (!g.tile) return hipErrorInvalidValue;       // (plan_front refuses such a filter)
    const size_t lds = (size_t)g.lds_bytes;
    // cover every bit word of the capture so the tail words are written (as zeros)
    uint64_t tiles = (p.n_out + g.tile - 1) / g.tile;
    if (p.bits && p.words_per_cap * 64 / g.tile > tiles) tiles = p.words_per_cap * 64 / g.tile;
    if (tiles == 0) return hipSuccess;
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(&fir_tuned_generic_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fir_tuned_generic_kernel, dim3((uint32_t)tiles, num_captures), dim3(256), lds, stream, p, g.lds_b_off,
                       g.tile);
    return hipGetLastError();
}

}  // namespace ookd
