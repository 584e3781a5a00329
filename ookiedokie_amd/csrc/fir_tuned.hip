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
// any shape, the contract's order throughout: fir_generic_kernel (kernels.hip) with complex taps
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fir_tuned_generic_kernel(const FrontParams p, uint32_t lds_b_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *buf[2] = {reinterpret_cast<float2 *>(smem_raw), reinterpret_cast<float2 *>(smem_raw) + lds_b_off};

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)p.num_stages;
    const int64_t j0 = (int64_t)blockIdx.x * kGenTile;
    GenLevel lv[kMaxStages + 1];
    int64_t off[kMaxStages];
    gen_levels(p, j0, kGenTile, lv, off);

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
                if (words && lane_id() == 0) words[((uint64_t)j0 + base + (tid & ~63u)) >> 6] = ball;
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

hipError_t launch_front_tuned_generic(const FrontParams &p, uint32_t num_captures, hipStream_t stream) {
    if (!p.tune || !p.ctaps || p.iq_f32 || p.halo_f32 || p.sample_fmt != kFmtSc16) return hipErrorInvalidValue;
    // level sizes of one tile, as launch_front_generic
    uint32_t len[kMaxStages + 1];
    const int S = (int)p.num_stages;
    len[S] = kGenTile;
    for (int s = S - 1; s >= 0; --s) len[s] = p.stage[s].decim * (len[s + 1] - 1) + p.stage[s].ntaps;
    uint32_t even = 0;
    for (int s = 0; s < S; s += 2) even = len[s] > even ? len[s] : even;
    const size_t lds = generic_lds_bytes(p);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    // cover every bit word of the capture so the tail words are written (as zeros)
    uint64_t tiles = (p.n_out + kGenTile - 1) / kGenTile;
    if (p.bits && p.words_per_cap * 64 / kGenTile > tiles) tiles = p.words_per_cap * 64 / kGenTile;
    if (tiles == 0) return hipSuccess;
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(&fir_tuned_generic_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fir_tuned_generic_kernel, dim3((uint32_t)tiles, num_captures), dim3(256), lds, stream, p, even + 1);
    return hipGetLastError();
}

}  // namespace ookd
