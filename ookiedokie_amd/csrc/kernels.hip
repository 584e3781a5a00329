// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the OOK rx path.
//
//   front end : SC16Q11 unpack -> FIR -> |.|^2 >= P* -> packed bit words
//               (reference: src/complexf.h:68-77, src/fir.c:302-395,
//                src/ookiedokie.c:171-179 with src/complexf.h:43-58)
//   edges     : bit words -> sorted list of level changes
//               (the content of --rx-rec-dig, src/ookiedokie.c:146-169)
//   fsm       : table-driven symbol state machine run over the edge list,
//               segment-parallel with a fix-point on the carried state
//               (reference per-sample form: src/state_machine.c:421-556,
//                buffer-skip rule: src/device.c:634-658)
//
// Compiled with -ffp-contract=off: every a*b+c below is a separately
// rounded multiply and add, exactly as the reference's scalar build; fused
// multiply-adds are written explicitly with __builtin_fmaf.
#include "kernels.hpp"
#include "common.hpp"
#include "front_dev.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace ookd {

// ---------------------------------------------------------------------------
// small helpers (the ones shared with fir_tuned.hip and survey_tuned.hip, fetch_raw among them: front_dev.hpp)
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// front end, 1 stage / decimation 1 (fs32_fs4, the 255-tap config)
// ---------------------------------------------------------------------------
//
// One wavefront = 64 lanes = 1024 consecutive outputs, working alone (a
// workgroup is just kFirWaves of them sharing an LDS allocation, no barrier);
// lane t owns outputs 16t..16t+15 and keeps their 32 partial sums in
// registers.  The wave loads its inputs plus the (padded) tap history raw,
// decides from them whether the filter can be skipped (quiet test), and
// otherwise unpacks them ONCE into its LDS window as float2.
// Taps are consumed in chunks of 32 held in SGPRs; within a chunk the lane
// streams 47 consecutive LDS samples, newest first, each feeding up to 16
// accumulators -- so every output sees its taps in the reference order
// (tap 0 / newest sample first, fir.c:313-318).
//
// LDS layout (slot<R>, front_dev.hpp): sample j lives at slot j + (j >> 4): one pad slot per 16
// samples makes the lane stride 17 float2 = 34 dwords, which is conflict
// free for ds_read_b64 (32-lane halves, 64 banks), and keeps every read of
// the unrolled body at  lane_base + compile-time immediate.

// Sequential, unfused recomputation of one output (guard-band path).
template <int R>
__device__ __noinline__ float2 fir1_exact_output(const float2 *lds, uint32_t j_out,
                                                 const float *taps, uint32_t ntaps) {
    float re = 0.0f, im = 0.0f;
    for (uint32_t k = 0; k < ntaps; ++k) {
        const float2 x = lds[slot<R>(j_out - k)];
        const float t = taps[k];
        const float pr = t * x.x;
        const float pi = t * x.y;
        re = re + pr;
        im = im + pi;
    }
    return make_float2(re, im);
}

// One complex multiply-accumulate acc(re,im) += tap * x(re,im) as a packed
// fp32 instruction with the tap read from an SGPR pair: `tp` holds two
// consecutive taps, HI picks which one is broadcast to both halves.  Plain
// v_fma_f32 issues at half the packed rate on gfx950 (measured: 77 vs 147
// TFLOP/s), so the packed form is what reaches the fp32 roof.
//   fused : v_pk_fma_f32                     (one rounding per step)
//   exact : v_pk_mul_f32 then v_pk_add_f32   (the reference's two roundings)
template <bool EXACT, bool HI>
__device__ __forceinline__ void cmac(v2f &acc, v2f tp, v2f x) {
    if (EXACT) {
        v2f prod;
        if (HI) {
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0]" : "=v"(prod) : "s"(tp), "v"(x));
        } else {
            asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(prod) : "s"(tp), "v"(x));
        }
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(prod));
    } else {
        if (HI) {
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(acc) : "s"(tp), "v"(x));
        } else {
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(tp), "v"(x));
        }
    }
}

// Compile-time unrolled body of one 32-tap chunk.  Window position W
// (newest first) feeds output r with tap kk = r - W when 0 <= kk < 32, so
// every output receives its taps in ascending order (fir.c:313-318).
template <bool EXACT, int R, int W, int... Rs>
__device__ __forceinline__ void fir1_wstep(v2f *acc, const v2f *tpair, const v2f *base,
                                           std::integer_sequence<int, Rs...>) {
    constexpr int cp = W + kTapChunk;                   // 1 .. R + 31
    const v2f x = base[cp + cp / R];
    ((void)((Rs - W >= 0 && Rs - W < kTapChunk)
                ? (cmac<EXACT, ((Rs - W) & 1) != 0>(acc[Rs], tpair[((Rs - W) & 31) >> 1], x), 0)
                : 0),
     ...);
}

template <bool EXACT, int R, int... Ws>
__device__ __forceinline__ void fir1_chunk(v2f *acc, const v2f *tpair, const v2f *base,
                                           std::integer_sequence<int, Ws...>) {
    (fir1_wstep<EXACT, R, R - 1 - Ws>(acc, tpair, base, std::make_integer_sequence<int, R>{}), ...);
}

// Everything behind the staged window of one wave tile: packed MACs over the
// tap chunks, threshold + guard band, bit packing, optional float output.
// Stores the tile's bit words and returns the tile info word
// (level changes inside the tile | first bit << 30 | last bit << 31).
template <bool EXACT, int R>
__device__ __forceinline__ uint32_t fir1_tile_compute(const FrontParams &p, float2 *lds, uint32_t Tp, uint64_t t0,
                                                      uint32_t tid, uint32_t cap, uint64_t *words) {
    uint32_t info = 0;
    // ---- accumulate ----------------------------------------------------------
    v2f acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = (v2f){0.0f, 0.0f};

    const uint32_t nchunks = Tp / kTapChunk;
    for (uint32_t c = 0; c < nchunks; ++c) {
        // 32 taps of this chunk -> 16 SGPR pairs
        const float *tp = p.taps + c * kTapChunk;
        v2f tpair[16];
        load_tap_chunk32(tp, tpair);

        // output r of this lane sits at window index Tp + R*tid + r; tap kc+kk reads
        // Tp + R*tid + r - kc - kk = R*tid + 32*m + (w + 32),  w = r - kk, m = (Tp - kc - 32)/32;
        // R*tid and 32*m are multiples of R, so their pad slots add up separately
        const uint32_t m = nchunks - 1 - c;
        const v2f *base = reinterpret_cast<const v2f *>(lds + (uint32_t)(R + 1) * tid + (32u + 32u / R) * m);
        fir1_chunk<EXACT, R>(acc, tpair, base, std::make_integer_sequence<int, R + kTapChunk - 1>{});
    }

    // ---- threshold, guard band, pack -----------------------------------------
    // Per output: power (packed square + add), one compare per bound whose
    // wave-wide result lands in an SGPR pair, and the lane's own bit shifted
    // into `mask` through the carry (r runs downwards so bit r ends at position
    // r).  The "inside the guard band" masks are OR-ed on the scalar unit.
    const uint64_t o0 = t0 + (uint64_t)tid * R;
    uint32_t mask = 0;
    uint64_t any_unsure = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
        float pw;
        if (EXACT) {
            pw = power_ref(acc[r].x, acc[r].y);
        } else {
            v2f sq;
            asm("v_pk_mul_f32 %0, %1, %1" : "=v"(sq) : "v"(acc[r]));
            pw = sq.x + sq.y;
        }
        const uint64_t ge_hi = __ballot(pw >= (EXACT ? p.p_star : p.p_hi));
        asm("v_addc_co_u32_e64 %0, vcc, %0, %0, %1" : "+v"(mask) : "s"(ge_hi) : "vcc");
        if (!EXACT) any_unsure |= __ballot(pw >= p.p_lo) & ~ge_hi;
    }
    if (!EXACT && any_unsure != 0) {
        // some lane of this wave has a sample inside the band: those lanes redo
        // their borderline samples in the reference's exact order
        uint32_t todo = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v2f sq;
            asm("v_pk_mul_f32 %0, %1, %1" : "=v"(sq) : "v"(acc[r]));
            const float pf = sq.x + sq.y;
            if (pf >= p.p_lo && !(pf >= p.p_hi) && o0 + r < p.n_out) todo |= 1u << r;
        }
        const uint32_t redo = (uint32_t)__popc(todo);
        while (todo) {                          // one copy of the recompute, whichever outputs need it
            const uint32_t r = (uint32_t)__ffs((int)todo) - 1u;
            todo &= todo - 1u;
            const float2 y = fir1_exact_output<R>(lds, Tp + R * tid + r, p.taps, p.stage[0].ntaps);
            const float pe = power_ref(y.x, y.y);
            mask = (mask & ~(1u << r)) | ((pe >= p.p_star ? 1u : 0u) << r);
        }
        if (redo && p.recompute_count) atomicAdd(p.recompute_count, (unsigned long long)redo);
    }
    // outputs past the end of the (padded) capture do not exist
    if (o0 + R > p.n_out) {
        const uint32_t keep = o0 >= p.n_out ? 0u : (uint32_t)(p.n_out - o0);
        mask &= (keep >= 32 ? 0xffffffffu : ((1u << keep) - 1u));
    }

    if (p.fir_out) {
        float2 *out = reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (o0 + r < p.n_out) out[o0 + r] = make_float2(acc[r].x, acc[r].y);
        }
    }

    // level changes inside the tile (what edge_count would find in these 1024 bits,
    // minus the comparison of the tile's first bit with the tile before)
    {
        const uint32_t keep = o0 >= p.n_out ? 0u : (o0 + R <= p.n_out ? (uint32_t)R : (uint32_t)(p.n_out - o0));
        const uint32_t prev_top = __shfl_up(mask >> (R - 1), 1);       // bit 15 of the lane before
        uint32_t ch = (mask ^ (mask << 1)) & ((1u << R) - 2u);
        if (tid != 0) ch |= (mask ^ prev_top) & 1u;
        ch &= keep >= 32 ? 0xffffffffu : ((1u << keep) - 1u);
        uint32_t cnt = __popc(ch);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mask & 1u));
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)((mask >> (R - 1)) & 1u), 63);
        // the word that holds the first change: lane l holds bits R l .. R l + R - 1 of the tile
        const uint64_t chl = __ballot(ch != 0);
        const uint32_t widx = chl ? ((uint32_t)__builtin_ctzll(chl) * (uint32_t)R) >> 6 : 0u;
        info = cnt | (widx << kTileWordShift) | (first << 30) | (last << 31) | p.stamp_bits;
    }

    // 64 / R lanes x R bits -> one 64-bit word
    constexpr uint32_t kLanesPerWord = 64u / R;
    uint64_t w64 = (uint64_t)mask << (R * (tid % kLanesPerWord));
#pragma unroll
    for (uint32_t d = 1; d < kLanesPerWord; d <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)w64, (int)d), hi = __shfl_xor((uint32_t)(w64 >> 32), (int)d);
        w64 |= (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if (tid % kLanesPerWord == 0) words[(t0 >> 6) + tid / kLanesPerWord] = w64;
    return info;
}

template <bool EXACT, int R>
__global__ __launch_bounds__(64 * kFirWgWaves) void fir1_bits_kernel(const FrontParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

    constexpr uint32_t kTile = 64u * R;                 // outputs per wavefront
    constexpr int kRounds = (kTile + 256 + 255) / 256;  // 16 B loads per lane (taps <= 256)
    const uint32_t tid = threadIdx.x & 63u;             // lane: every wavefront works alone
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t cap = blockIdx.y;
    const uint64_t t0 = (((uint64_t)blockIdx.x + p.tile_base) * kFirWgWaves + wave) * kTile;
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    float2 *lds = reinterpret_cast<float2 *>(smem_raw) + wave * fir1_wave_slots<R>(Tp);
    uint64_t *words = p.bits + (uint64_t)cap * p.words_per_cap;

    // ---- load the wave's window: slot j <-> input index t0 - Tp + j ------------
    // 64R + Tp samples in vectors of 4, lane + 64*i, kept RAW in
    // registers until the quiet test has decided whether they are needed.
    const uint32_t nvec = (kTile + Tp) >> 2;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const bool interior = aligned16 && t0 >= Tp && t0 + kTile <= p.n_valid;
    if (interior) {
        const uint4 *src4 = reinterpret_cast<const uint4 *>(src + (t0 - Tp));
        uint4 q[kRounds];
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            q[i] = (64u * (i + 1) <= kTile / 4 || v < nvec) ? ld_nt4(src4 + v) : make_uint4(0, 0, 0, 0);     // read once
        }
        // ---- quiet test ----------------------------------------------------------
        // |y_re|,|y_im| <= sum|h| * max|component|, so a wave whose whole window
        // stays below quiet_lsb cannot reach the threshold: its 1024 bits are 0
        // without running the filter -- exactly what the reference computes.
        v2s mx = (v2s){0, 0}, mn = (v2s){0, 0};
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].x), as_v2s(q[i].y)));
            mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].z), as_v2s(q[i].w)));
            mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].x), as_v2s(q[i].y)));
            mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].z), as_v2s(q[i].w)));
        }
        const int L = p.quiet_lsb;
        const bool loud = !(mx.x < L && mx.y < L && mn.x > -L && mn.y > -L);
        if (!p.fir_out && __ballot(loud) == 0) {
            // sparse output: nothing is stored; whatever the tile's words and info hold carries an older
            // run's stamp and reads as quiet (tile_live)
            if (!p.sparse) {
                if (tid < kTile / 64) words[(t0 >> 6) + tid] = 0;
                if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + t0 / kTile] = 0;
            }
            if (p.quiet_count && tid == 0) atomicAdd(p.quiet_count + (blockIdx.x % kQuietCounters), 1u);
            return;
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
    // the window is private to this wavefront and the LDS executes one wave's
    // accesses in order: no workgroup barrier, only keep the compiler from
    // moving reads above the writes
    wave_lds_fence();

    const uint32_t info = fir1_tile_compute<EXACT, R>(p, lds, Tp, t0, tid, cap, words);
    if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + t0 / kTile] = info;
}

// ---------------------------------------------------------------------------
// front end, two decimating stages (the backend default fs128_fs16_dec4:
// 16 taps / 2 then 32 taps / 2) -- SURVEY.md 8(f) row f1
// ---------------------------------------------------------------------------
//
// Same execution model as the 1-stage kernel: one wavefront = one tile, no
// workgroup barrier, raw loads -> quiet test -> unpack into a private LDS
// window -> register-blocked packed MACs with the taps in SGPRs.  Here the
// tile is F = 64*R2 final outputs; stage 1 first produces the L1 intermediate
// outputs stage 2 needs (its own halo recomputed per tile, ~12 %) into a
// second LDS window.  Stage output J reads inputs D*(J+1)-1-k (fir.c:290:
// the countdown starts at D); every stage's geometry is a compile-time
// constant, so all LDS addresses in the MAC bodies are lane_base + immediate.
//
// Arithmetic is always the reference's (separately rounded multiply and
// add): floats and bits are bit-identical, no guard band needed.
//
// LDS layout per level: lane t's block of P = D*R consecutive samples starts
// at slot t*(P+1) -- one pad per block makes the lane stride odd, i.e.
// conflict free for ds_read_b64.

// (Fir2Geom, the geometry both this kernel and fir2_tuned_kernel are built on: front_dev.hpp)

// One 16-tap chunk of a decimating stage: window position W (newest first)
// feeds output r with tap kk = D*r - D*(R-1) + W when 0 <= kk < 16.
__device__ __forceinline__ v2f lds_sample(const v2f *base, int i) { return base[i]; }
__device__ __forceinline__ v2f lds_sample(const uint32_t *base, int i) {       // raw SC16Q11 level
    const float2 v = unpack_iq(base[i]);
    return (v2f){v.x, v.y};
}

template <bool EXACT, int D, int R, int P, int CHUNK_OFF, int W, typename In, int... Rs>
__device__ __forceinline__ void fir2_wstep(v2f *acc, const v2f *tpair, const In *base,
                                           std::integer_sequence<int, Rs...>) {
    // sample index inside the lane's window: c = Tpad-1 + D*(R-1) - 16*chunk - W
    constexpr int c = CHUNK_OFF + D * (R - 1) - W;
    static_assert(c >= 0, "window underflow");
    const v2f x = lds_sample(base, c + c / P);
    ((void)((D * Rs - D * (R - 1) + W >= 0 && D * Rs - D * (R - 1) + W < 16)
                ? (cmac<EXACT, ((D * Rs - D * (R - 1) + W) & 1) != 0>(
                       acc[Rs], tpair[((D * Rs - D * (R - 1) + W) & 15) >> 1], x),
                   0)
                : 0),
     ...);
}

template <bool EXACT, int D, int R, int P, int CHUNK_OFF, typename In, int... Ws>
__device__ __forceinline__ void fir2_chunk_body(v2f *acc, const v2f *tpair, const In *base,
                                                std::integer_sequence<int, Ws...>) {
    (fir2_wstep<EXACT, D, R, P, CHUNK_OFF, Ws>(acc, tpair, base, std::make_integer_sequence<int, R>{}), ...);
}

// All chunks of one stage, taps kk ascending across chunks (reference order).
template <bool EXACT, int D, int R, int P, int TPAD, int CH, typename In>
__device__ __forceinline__ void fir2_stage_chunk(v2f *acc, const float *taps, const In *base) {
    v8f ta, tb;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\t"
                 "s_load_dwordx8 %1, %2, 0x20\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(ta), "=&s"(tb)
                 : "s"(taps + 16 * CH)
                 : "memory");
    const v2f tpair[8] = {
        __builtin_shufflevector(ta, ta, 0, 1), __builtin_shufflevector(ta, ta, 2, 3),
        __builtin_shufflevector(ta, ta, 4, 5), __builtin_shufflevector(ta, ta, 6, 7),
        __builtin_shufflevector(tb, tb, 0, 1), __builtin_shufflevector(tb, tb, 2, 3),
        __builtin_shufflevector(tb, tb, 4, 5), __builtin_shufflevector(tb, tb, 6, 7)};
    // tap k = 16*CH + kk of output r reads window sample (TPAD-1) + D*r - k
    fir2_chunk_body<EXACT, D, R, P, TPAD - 1 - 16 * CH>(acc, tpair, base,
                                                 std::make_integer_sequence<int, D*(R - 1) + 16>{});
}

template <bool EXACT, int D, int R, int P, int TPAD, typename In, int... CHs>
__device__ __forceinline__ void fir2_stage(v2f *acc, const float *taps, const In *base,
                                           std::integer_sequence<int, CHs...>) {
    (fir2_stage_chunk<EXACT, D, R, P, TPAD, CHs>(acc, taps, base), ...);
}

// Reference-order recomputation of one final output (guard-band path): the
// T2 stage-1 outputs it reads, each from the raw level-0 window, then stage 2.
// `j` = final output index inside the tile.
template <typename G>
__device__ __noinline__ float2 fir2_exact_output(const uint32_t *lds0, const float *taps1, uint32_t ntaps1,
                                                 const float *taps2, uint32_t ntaps2, uint32_t j) {
    float re2 = 0.0f, im2 = 0.0f;
    for (uint32_t k2 = 0; k2 < ntaps2; ++k2) {
        const uint32_t j1 = G::D2 * j + (G::T2 - 1) - k2;               // local stage-1 index
        float re1 = 0.0f, im1 = 0.0f;
        for (uint32_t k1 = 0; k1 < ntaps1; ++k1) {
            const uint32_t i = G::D1 * j1 + (G::T1 - 1) - k1;           // local input index
            const float2 x = unpack_iq(lds0[i + i / G::P1]);
            const float t = taps1[k1];
            const float pr = t * x.x;
            const float pi = t * x.y;
            re1 = re1 + pr;
            im1 = im1 + pi;
        }
        const float t2 = taps2[k2];
        const float pr = t2 * re1;
        const float pi = t2 * im1;
        re2 = re2 + pr;
        im2 = im2 + pi;
    }
    return make_float2(re2, im2);
}

constexpr int kFir2Waves = 1;           // single-wave workgroups: a loud wave must not pin the LDS / wave slots of finished quiet ones

template <typename G, bool EXACT>
__global__ __launch_bounds__(64 * kFir2Waves) void fir2_bits_kernel(const FrontParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t tid = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t cap = blockIdx.y;
    const uint64_t J0 = (((uint64_t)blockIdx.x + p.tile_base) * kFir2Waves + wave) * G::F;     // first final output
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    uint32_t *lds0 = reinterpret_cast<uint32_t *>(smem_raw + wave * G::wave_bytes);    // raw I,Q pairs
    float2 *lds1 = reinterpret_cast<float2 *>(lds0 + G::slots0);
    uint64_t *words = p.bits + (uint64_t)cap * p.words_per_cap;

    // global index of local stage-1 output 0 and of local input sample 0
    const int64_t j1_0 = (int64_t)G::D2 * (int64_t)J0 + (G::D2 - 1) - (G::T2 - 1);
    const int64_t a0 = (int64_t)G::D1 * j1_0 + (G::D1 - 1) - (G::T1 - 1);

    // ---- load + quiet test + unpack (as in fir1_bits_kernel) ---------------------
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const int64_t va = a0 & ~(int64_t)3;
    const bool interior = aligned16 && a0 >= 0 && (uint64_t)(va + 4 * G::kVecs) <= p.n_valid;
    if (interior) {
        const uint4 *src4 = reinterpret_cast<const uint4 *>(src + va);
        uint4 q[G::kVecRounds];
#pragma unroll
        for (int i = 0; i < G::kVecRounds; ++i) {
            const uint32_t v = tid + 64u * i;
            q[i] = (64 * (i + 1) <= G::kVecs || v < (uint32_t)G::kVecs) ? src4[v] : make_uint4(0, 0, 0, 0);
        }
        v2s mx = (v2s){0, 0}, mn = (v2s){0, 0};
#pragma unroll
        for (int i = 0; i < G::kVecRounds; ++i) {
            mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].x), as_v2s(q[i].y)));
            mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(as_v2s(q[i].z), as_v2s(q[i].w)));
            mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].x), as_v2s(q[i].y)));
            mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(as_v2s(q[i].z), as_v2s(q[i].w)));
        }
        const int L = p.quiet_lsb;
        const bool loud = !(mx.x < L && mx.y < L && mn.x > -L && mn.y > -L);
        if (!p.fir_out && __ballot(loud) == 0) {
            // (sparse output: nothing is stored -- what the tile's words and info hold carries an older run's stamp
            //  and reads as quiet, tile_live)
            if (!p.sparse) {
                if (tid < G::F / 64) words[(J0 >> 6) + tid] = 0;
                if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + J0 / G::F] = 0;
            }
            if (p.quiet_count && tid == 0) atomicAdd(p.quiet_count + (blockIdx.x % kQuietCounters), 1u);
            return;
        }
        const int shift = (int)(a0 - va);           // 0..3 samples of the first vector precede the window
#pragma unroll
        for (int i = 0; i < G::kVecRounds; ++i) {
            const int i0 = 4 * (int)(tid + 64u * i) - shift;        // local index of q[i].x
            const uint32_t w4[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int li = i0 + e;
                if (li >= 0 && li < G::L0) lds0[li + li / G::P1] = w4[e];
            }
        }
    } else {
        // first / last tiles, halo: values outside the capture are zeros or the
        // previous shard's samples -- all of them int16, so the level stays raw
        for (int li = (int)tid; li < G::L0; li += 64) {
            lds0[li + li / G::P1] = fetch_raw(p, src, a0 + li);
        }
    }
    wave_lds_fence();

    // ---- stage 1: lane t -> local outputs R1*t .. R1*t + R1-1 ---------------------------
    {
        v2f acc[G::R1];
#pragma unroll
        for (int r = 0; r < G::R1; ++r) acc[r] = (v2f){0.0f, 0.0f};
        const uint32_t *base = lds0 + (G::P1 + 1) * tid;
        fir2_stage<EXACT, G::D1, G::R1, G::P1, G::T1>(acc, p.taps + p.stage[0].tap_off, base,
                                               std::make_integer_sequence<int, G::N1>{});
#pragma unroll
        for (int r = 0; r < G::R1; ++r) {
            const int j = G::R1 * (int)tid + r;
            lds1[j + j / G::P2] = make_float2(acc[r].x, acc[r].y);
        }
    }
    wave_lds_fence();

    // ---- stage 2: lane t -> final outputs J0 + R2*t .. + R2-1 ------------------------------
    v2f acc[G::R2];
#pragma unroll
    for (int r = 0; r < G::R2; ++r) acc[r] = (v2f){0.0f, 0.0f};
    {
        const v2f *base = reinterpret_cast<const v2f *>(lds1 + (G::P2 + 1) * tid);
        fir2_stage<EXACT, G::D2, G::R2, G::P2, G::T2>(acc, p.taps + p.stage[1].tap_off, base,
                                               std::make_integer_sequence<int, G::N2>{});
    }

    // ---- threshold + pack: R2 bits per lane, 64 / R2 lanes per word ----------------------------
    static_assert(G::R2 == 4, "bit packing below assumes 4 outputs per lane");
    const uint64_t o0 = J0 + (uint64_t)tid * G::R2;
    uint32_t nib = 0;
    float2 *fout = p.fir_out ? reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out : nullptr;
#pragma unroll
    for (int r = 0; r < G::R2; ++r) {
        const bool valid = o0 + r < p.n_out;
        const float pw = power_ref(acc[r].x, acc[r].y);
        bool bit = pw >= (EXACT ? p.p_star : p.p_hi);
        if (!EXACT && valid && !bit && pw >= p.p_lo) {
            // inside the guard band: redo this output in the reference's exact order
            const float2 y = fir2_exact_output<G>(lds0, p.taps + p.stage[0].tap_off, p.stage[0].ntaps,
                                                  p.taps + p.stage[1].tap_off, p.stage[1].ntaps, G::R2 * tid + r);
            bit = power_ref(y.x, y.y) >= p.p_star;
            if (p.recompute_count) atomicAdd(p.recompute_count, 1ull);
        }
        nib |= ((valid && bit) ? 1u : 0u) << r;
        if (fout && valid) fout[o0 + r] = make_float2(acc[r].x, acc[r].y);
    }
    {
        // level changes inside the tile, as in the 1-stage kernel
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
        if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + J0 / G::F] = cnt | (widx << kTileWordShift) | (first << 30) | (last << 31) | p.stamp_bits;
    }
    uint32_t half = nib << (4u * (tid & 7u));
    half |= __shfl_xor(half, 1);
    half |= __shfl_xor(half, 2);
    half |= __shfl_xor(half, 4);                // lanes 8g..8g+7 hold outputs 32g..32g+31
    const uint32_t hi = __shfl_down(half, 8);
    if ((tid & 15u) == 0) words[(J0 >> 6) + (tid >> 4)] = (uint64_t)half | ((uint64_t)hi << 32);
}

// (Fir2Dec4, the one geometry it is instantiated for: front_dev.hpp)

// ---------------------------------------------------------------------------
// front end, generic: any number of stages / decimations, exact arithmetic
// ---------------------------------------------------------------------------
//
// One workgroup = `tile` final outputs (generic_tile(): kGenTile unless the
// level buffers only hold less).  Level 0 is the unpacked input,
// level s+1 the output of stage s; the slice of every level the tile needs
// is produced in LDS, ping-ponging between two buffers.  Stage output J
// (global) reads level-s inputs D*(J+1)-1-k (fir.c:290: the countdown starts
// at D, so the first output is at input index D-1): gen_levels, front_dev.hpp.

template <bool F32IN>
__global__ __launch_bounds__(256) void fir_generic_kernel(const FrontParams p, uint32_t lds_b_off, uint32_t tile) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *buf[2] = {reinterpret_cast<float2 *>(smem_raw),
                      reinterpret_cast<float2 *>(smem_raw) + lds_b_off};

    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const int S = (int)p.num_stages;
    const int64_t j0 = (int64_t)blockIdx.x * tile;
    GenLevel lv[kMaxStages + 1];
    int64_t off[kMaxStages];
    gen_levels(p, j0, tile, lv, off);

    const uint32_t *src = F32IN ? nullptr
                                : reinterpret_cast<const uint32_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    const float2 *srcf = F32IN ? reinterpret_cast<const float2 *>(p.iq_f32) + (uint64_t)cap * p.cap_stride
                               : nullptr;

    for (uint32_t i = tid; i < lv[0].len; i += 256) {
        buf[0][i] = fetch_sample(p, src, srcf, lv[0].a + (int64_t)i);
    }
    __syncthreads();

    uint64_t *words = p.bits ? p.bits + (uint64_t)cap * p.words_per_cap : nullptr;
    float2 *fout = p.fir_out ? reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out : nullptr;

    for (int s = 0; s < S; ++s) {
        const float2 *in = buf[s & 1];
        float2 *out = buf[(s + 1) & 1];
        const float *taps = p.taps + p.stage[s].tap_off;
        const int64_t D = p.stage[s].decim;
        const uint32_t T = p.stage[s].ntaps;
        const bool last = (s == S - 1);
        const uint32_t n = lv[s + 1].len;
        for (uint32_t base = 0; base < n; base += 256) {
            const uint32_t i = base + tid;
            float re = 0.0f, im = 0.0f;
            if (i < n) {
                const int64_t jl = lv[s + 1].a + (int64_t)i;
                const int64_t newest = D * jl + off[s] - lv[s].a;   // index into `in`
                for (uint32_t k = 0; k < T; ++k) {
                    const float2 x = in[newest - (int64_t)k];
                    const float t = taps[k];
                    const float pr = t * x.x;
                    const float pi = t * x.y;
                    re = re + pr;
                    im = im + pi;
                }
            }
            if (!last) {
                if (i < n) out[i] = make_float2(re, im);
            } else {
                const int64_t o = j0 + (int64_t)i;
                const bool valid = (i < n) && o >= 0 && (uint64_t)o < p.n_out;
                const bool bit = valid && (power_ref(re, im) >= p.p_star);
                const uint64_t ball = __ballot(bit);
                // (a tile below 256 outputs is one round: the waves past it own no word)
                if (words && lane_id() == 0 && base + (tid & ~63u) < tile) {
                    words[((uint64_t)j0 + base + (tid & ~63u)) >> 6] = ball;
                }
                if (fout && valid) fout[o] = make_float2(re, im);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// front end, no filter ("-F none", ookiedokie.c:260-263): threshold the
// unpacked samples directly.  16 B per lane loads; a wave covers 256 samples.
// ---------------------------------------------------------------------------
// One wavefront = 1024 samples (16 per lane, four 16 B loads issued up
// front), same tile / tile-info convention as the 1-stage FIR kernel.
// FMT (kFmt*): the 8-bit formats read their 16 samples as two 16 B loads and widen them in registers.
template <int FMT>
__device__ __forceinline__ uint32_t fetch_raw8(const FrontParams &p, const uint16_t *src, int64_t n) {
    if (n < 0) {
        const int64_t h = (int64_t)p.halo_len + n;
        if (h < 0 || !p.halo) return 0u;
        return widen8<FMT>(reinterpret_cast<const uint16_t *>(p.halo)[h]);
    }
    if ((uint64_t)n >= p.n_valid) return 0u;
    return widen8<FMT>(src[n]);
}

template <int FMT>
__global__ __launch_bounds__(64) void nofir_bits_kernel(const FrontParams p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t cap = blockIdx.y;
    const uint64_t t0 = ((uint64_t)blockIdx.x + p.tile_base) * kWaveTile;
    typedef typename std::conditional<FMT == (int)kFmtSc16, uint32_t, uint16_t>::type raw_t;
    const raw_t *src = reinterpret_cast<const raw_t *>(p.iq) + (uint64_t)cap * p.cap_stride;
    uint64_t *words = p.bits + (uint64_t)cap * p.words_per_cap;
    float2 *fout = p.fir_out ? reinterpret_cast<float2 *>(p.fir_out) + (uint64_t)cap * p.n_out : nullptr;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const uint64_t o0 = t0 + 16ull * tid;          // lane owns samples o0 .. o0+15
    uint32_t raw[16];
    if constexpr (FMT == (int)kFmtSc16) {
        if (aligned16 && t0 + kWaveTile <= p.n_valid) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src + o0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 q = s4[i];
                raw[4 * i] = q.x;
                raw[4 * i + 1] = q.y;
                raw[4 * i + 2] = q.z;
                raw[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) raw[i] = fetch_raw(p, src, (int64_t)(o0 + i));
        }
    } else {
        if (aligned16 && t0 + kWaveTile <= p.n_valid) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src + o0);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint4 q = s4[i];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    raw[8 * i + 2 * k] = widen8<FMT>(w[k] & 0xffffu);
                    raw[8 * i + 2 * k + 1] = widen8<FMT>(w[k] >> 16);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) raw[i] = fetch_raw8<FMT>(p, src, (int64_t)(o0 + i));
        }
    }
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float2 v = unpack_iq(raw[i]);
        const bool valid = o0 + i < p.n_out;
        mask |= ((valid && power_ref(v.x, v.y) >= p.p_star) ? 1u : 0u) << i;
        if (fout && valid) fout[o0 + i] = v;
    }
    {
        // level changes inside the tile (see fir1_bits_kernel)
        const uint32_t keep = o0 >= p.n_out ? 0u : (o0 + 16 <= p.n_out ? 16u : (uint32_t)(p.n_out - o0));
        const uint32_t prev_top = __shfl_up(mask >> 15, 1);
        uint32_t ch = (mask ^ (mask << 1)) & 0xfffeu;
        if (tid != 0) ch |= (mask ^ prev_top) & 1u;
        ch &= (1u << keep) - 1u;
        uint32_t cnt = __popc(ch);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mask & 1u));
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)((mask >> 15) & 1u), 63);
        const uint64_t chl = __ballot(ch != 0);         // (the word that holds the first change: 16 bits per lane)
        const uint32_t widx = chl ? (uint32_t)__builtin_ctzll(chl) >> 2 : 0u;
        if (tid == 0) p.tile_info[(uint64_t)cap * p.tiles_per_cap + (t0 >> 10)] = cnt | (widx << kTileWordShift) | (first << 30) | (last << 31) | p.stamp_bits;
    }
    const uint32_t pair = mask | (__shfl_xor(mask, 1) << 16);      // valid on even lanes
    const uint32_t hi = __shfl_xor(pair, 2);
    if ((tid & 3u) == 0) words[(t0 >> 6) + (tid >> 2)] = (uint64_t)pair | ((uint64_t)hi << 32);
}

// ---------------------------------------------------------------------------
// unpack only (SDR backend rx: complexf.h:68-77 on the GPU)
// ---------------------------------------------------------------------------
// (8-bit formats: v / 128.0f = the unpacked widened sample, exactly)
template <int FMT>
__global__ __launch_bounds__(256) void unpack_kernel(const void *iq, float2 *out, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if constexpr (FMT == (int)kFmtSc16) out[i] = unpack_iq(static_cast<const uint32_t *>(iq)[i]);
        else out[i] = unpack_iq(widen8<FMT>(static_cast<const uint16_t *>(iq)[i]));
    }
}

// ---------------------------------------------------------------------------
// 8-bit capture -> SC16Q11 staging copy, for the forms that have no fused 8-bit kernel (packed-VALU, exact,
// generic: test and fallback paths).  Four samples per lane and turn: one 8 B load, one 16 B store where both
// are aligned, sample by sample otherwise.
// ---------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(256) void widen_kernel(const uint16_t *src, uint32_t *dst, uint64_t n, uint64_t src_stride,
                                                    uint64_t dst_stride) {
    const uint16_t *s = src + (uint64_t)blockIdx.y * src_stride;
    uint32_t *d = dst + (uint64_t)blockIdx.y * dst_stride;
    const bool aligned = ((reinterpret_cast<uintptr_t>(s) & 7u) | (reinterpret_cast<uintptr_t>(d) & 15u)) == 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 4;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (aligned && i + 4 <= n) {
            const uint2 q = *reinterpret_cast<const uint2 *>(s + i);
            *reinterpret_cast<uint4 *>(d + i) = make_uint4(widen8<FMT>(q.x & 0xffffu), widen8<FMT>(q.x >> 16),
                                                           widen8<FMT>(q.y & 0xffffu), widen8<FMT>(q.y >> 16));
        } else {
            for (uint64_t k = i; k < n && k < i + 4; ++k) d[k] = widen8<FMT>(s[k]);
        }
    }
}

// ---------------------------------------------------------------------------
// pack only (post-filter recorder: complexf.h:87-96 on the GPU)
// ---------------------------------------------------------------------------
// (int16_t)(x * 2048.0f): truncate towards zero to a 32-bit integer, keep the
// low 16 bits (what the reference's cast compiles to on x86-64).
__device__ __forceinline__ uint32_t pack_iq(float2 v) {
    const int32_t re = (int32_t)(v.x * 2048.0f);
    const int32_t im = (int32_t)(v.y * 2048.0f);
    return ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
}

__global__ __launch_bounds__(256) void pack_kernel(const float2 *in, uint32_t *iq, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        iq[i] = pack_iq(in[i]);
    }
}

// ---------------------------------------------------------------------------
// synthetic capture generator
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void synth_kernel(const SynthRun *runs, uint64_t num_runs, uint64_t seed,
                                                    uint32_t noise, uint64_t first, uint64_t count,
                                                    uint32_t *iq) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 4;
    for (uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < count; base += stride) {
        const uint64_t n0 = first + base;
        // last run with start <= n0
        uint64_t lo = 0, hi = num_runs;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (runs[mid].start <= n0) lo = mid;
            else hi = mid;
        }
        uint64_t ri = lo;
        uint32_t out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t n = n0 + i;
            while (ri + 1 < num_runs && runs[ri + 1].start <= n) ri++;
            int ni, nq;
            synth_noise(seed, n, noise, ni, nq);
            int vi = (num_runs && runs[ri].start <= n ? runs[ri].i_level : 0) + ni;
            int vq = (num_runs && runs[ri].start <= n ? runs[ri].q_level : 0) + nq;
            vi = max(-32768, min(32767, vi));
            vq = max(-32768, min(32767, vq));
            out[i] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
        }
        if (base + 3 < count && ((reinterpret_cast<uintptr_t>(iq + base) & 15u) == 0)) {
            *reinterpret_cast<uint4 *>(iq + base) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            for (int i = 0; i < 4; ++i) {
                if (base + i < count) iq[base + i] = out[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// small tiles only pay through the quiet shortcut: none without it (quiet_lsb 0)
static int fir1_R(const FrontParams &p) {
    if (front_uses_mfma(p)) return (int)kMfmaTile / 64;
    return (p.stage[0].ntaps_pad <= kFir1ShortTaps && p.quiet_lsb > 0) ? kFir1RShort : kFir1RLong;
}

static size_t fir1_lds_bytes(const FrontParams &p) {
    const uint32_t Tp = p.stage[0].ntaps_pad;
    const uint32_t slots = fir1_R(p) == kFir1RShort ? fir1_wave_slots<kFir1RShort>(Tp) : fir1_wave_slots<kFir1RLong>(Tp);
    return (size_t)kFirWgWaves * slots * sizeof(float2);
}

// the tiles of a launch: every output, and every bit word of the capture so the tail words are written (as zeros;
// words_per_cap is a multiple of kBlockWords, a tile a power of two of at least one word)
static uint64_t generic_tiles(const FrontParams &p, uint32_t tile) {
    uint64_t tiles = (p.n_out + tile - 1) / tile;
    if (p.bits && p.words_per_cap * 64 / tile > tiles) tiles = p.words_per_cap * 64 / tile;
    return tiles;
}

hipError_t launch_front_generic(const FrontParams &p, uint32_t num_captures, hipStream_t stream) {
    const GenTile g = generic_tile(p.stage, p.num_stages);
    if (!g.tile) return hipErrorInvalidValue;       // (plan_front / ookd_fir_create refuse such a filter)
    const size_t lds = (size_t)g.lds_bytes;
    const uint64_t tiles = generic_tiles(p, g.tile);
    if (tiles == 0) return hipSuccess;
    dim3 grid((uint32_t)tiles, num_captures);
    hipError_t e;
    if (p.iq_f32) {
        e = ensure_dynamic_lds(reinterpret_cast<const void *>(&fir_generic_kernel<true>), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fir_generic_kernel<true>, grid, dim3(256), lds, stream, p, g.lds_b_off, g.tile);
    } else {
        e = ensure_dynamic_lds(reinterpret_cast<const void *>(&fir_generic_kernel<false>), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fir_generic_kernel<false>, grid, dim3(256), lds, stream, p, g.lds_b_off, g.tile);
    }
    return hipGetLastError();
}

hipError_t ensure_dynamic_lds(const void *func, size_t bytes) {
    struct Granted {
        const void *func;
        int dev;
        size_t bytes;
    };
    static thread_local std::vector<Granted> granted;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (Granted &g : granted) {
        if (g.func == func && g.dev == dev) {
            if (g.bytes >= bytes) return hipSuccess;
            const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e == hipSuccess) g.bytes = bytes;
            return e;
        }
    }
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) granted.push_back({func, dev, bytes});
    return e;
}

static bool use_fir1(const FrontParams &p) {
    // (the tuned kernels' load rounds cover a tap history of up to 256 samples; longer filters: generic kernel)
    return p.num_stages == 1 && p.stage[0].decim == 1 && p.origin == 0 && !p.iq_f32 &&
           p.stage[0].ntaps_pad <= 256u && fir1_lds_bytes(p) <= 160 * 1024;
}

static bool use_fir2(const FrontParams &p) {
    // every level's phase is D-1 when the origin is a multiple of the total decimation
    return p.num_stages == 2 && !p.iq_f32 && !p.halo_f32 && p.stage[0].decim == 2 && p.stage[1].decim == 2 &&
           p.stage[0].ntaps <= Fir2Dec4::T1 && p.stage[1].ntaps <= Fir2Dec4::T2 && p.origin % 4 == 0;
}

// (8-bit formats: the three *_8 forms read the capture as it is; any other number means the 16-bit kernel of that
//  number, on a widened copy)
uint32_t front_form(const FrontParams &p, bool exact) {
    const bool s8 = p.sample_fmt != kFmtSc16;
    // a tuned context (fir_tuned.hip): its forms, all on SC16Q11 samples (8-bit captures are widened first)
    if (p.tune && p.num_stages) {
        if (front_uses_tuned_fir1(p) && !exact) return OOKD_FRONT_TUNED_FIR1;
        return front_uses_tuned_fir2(p) && !exact ? OOKD_FRONT_TUNED_FIR2 : OOKD_FRONT_TUNED_GENERIC;
    }
    if (p.num_stages == 0) return s8 ? OOKD_FRONT_NO_FILTER_8 : OOKD_FRONT_NO_FILTER;
    if (use_fir1(p)) {
        if (front_uses_mfma(p) && !exact) return s8 ? OOKD_FRONT_FIR1_MFMA_8 : OOKD_FRONT_FIR1_MFMA;
        return exact ? OOKD_FRONT_FIR1_VALU_EXACT : OOKD_FRONT_FIR1_VALU;
    }
    if (use_fir2(p)) {
        if (front_uses_mfma2(p) && !exact) return s8 ? OOKD_FRONT_FIR2_MFMA_8 : OOKD_FRONT_FIR2_MFMA;
        return exact ? OOKD_FRONT_FIR2_VALU_EXACT : OOKD_FRONT_FIR2_VALU;
    }
    return OOKD_FRONT_GENERIC;
}

uint64_t front_wave_tiles(const FrontParams &p) {
    if (p.tune && p.num_stages) {
        if (front_uses_tuned_fir2(p)) return (p.n_out + kTunedFir2Tile - 1) / kTunedFir2Tile;
        return front_uses_tuned_fir1(p) ? ((p.n_out + kFirTile - 1) / kFirTile) * (kFirTile / tuned_fir1_tile_bits(p)) : 0;
    }
    if (p.num_stages == 0) return ((p.n_out + kFirTile - 1) / kFirTile) * (kFirTile / kWaveTile);
    if (use_fir1(p)) return ((p.n_out + kFirTile - 1) / kFirTile) * (kFirTile / (64 * fir1_R(p)));
    if (use_fir2(p)) {
        const uint64_t per_wg = (uint64_t)kFir2Waves * Fir2Dec4::F;
        return ((p.n_out + per_wg - 1) / per_wg) * kFir2Waves;
    }
    return 0;
}

uint32_t front_tile_bits(const FrontParams &p) {
    if (p.tune && p.num_stages) {
        if (front_uses_tuned_fir2(p)) return kTunedFir2Tile;
        return front_uses_tuned_fir1(p) ? tuned_fir1_tile_bits(p) : 0;
    }
    if (p.num_stages == 0) return kWaveTile;
    if (use_fir1(p)) return 64 * fir1_R(p);
    if (use_fir2(p)) return Fir2Dec4::F;
    return 0;
}

// t0 / t1 (optional): events that take the kernel's own start / end time stamps.  For the
// one-kernel front ends they ride on the dispatch itself (hipExtLaunchKernel): no marker
// packets in front of and behind the dominant kernel, and their difference is the kernel's
// duration as a profiler sees it.
hipError_t launch_front(const FrontParams &p, uint32_t num_captures, bool exact, hipStream_t stream,
                        hipEvent_t t0, hipEvent_t t1, uint64_t tile_begin, uint64_t tile_count) {
    if (p.n_out == 0) {
        if (t0 && hipEventRecord(t0, stream) != hipSuccess) return hipGetLastError();
        if (t1 && hipEventRecord(t1, stream) != hipSuccess) return hipGetLastError();
        return hipSuccess;
    }
    // [tile_begin, tile_begin + tile_count) of the capture's wave tiles (tuned kernels only), default: all
    auto range = [&](uint64_t all, uint64_t &grid, FrontParams &pp) {
        const uint64_t b = tile_begin < all ? tile_begin : all;
        grid = tile_count < all - b ? tile_count : all - b;
        pp.tile_base = (uint32_t)b;
    };
    FrontParams pp = p;
    void *args[] = {&pp};
    uint64_t grid = 0;
    const uint32_t form = front_form(p, exact);
    if (p.sample_fmt != kFmtSc16 && form != OOKD_FRONT_NO_FILTER_8 && form != OOKD_FRONT_FIR1_MFMA_8 &&
        form != OOKD_FRONT_FIR2_MFMA_8) {
        return hipErrorInvalidValue;        // no 8-bit kernel of this form: the caller widens first
    }
    if (form == OOKD_FRONT_TUNED_FIR1) return launch_front_tuned_fir1(p, num_captures, stream, t0, t1, tile_begin, tile_count);
    if (form == OOKD_FRONT_TUNED_FIR2) return launch_front_tuned_fir2(p, num_captures, stream, t0, t1, tile_begin, tile_count);
    if (form == OOKD_FRONT_TUNED_GENERIC) {
        if (tile_begin != 0 || tile_count != ~0ull) return hipErrorInvalidValue;     // whole captures only
        if (t0 && hipEventRecord(t0, stream) != hipSuccess) return hipGetLastError();
        const hipError_t e = launch_front_tuned_generic(p, num_captures, stream);
        if (e != hipSuccess) return e;
        if (t1 && hipEventRecord(t1, stream) != hipSuccess) return hipGetLastError();
        return hipSuccess;
    }
    if (form == OOKD_FRONT_NO_FILTER || form == OOKD_FRONT_NO_FILTER_8) {
        // whole 4096-sample blocks, so every bit word of the capture is written
        range((p.n_out + kFirTile - 1) / kFirTile * kFirWaves, grid, pp);
        if (grid == 0) return hipSuccess;
        const void *fn = p.sample_fmt == kFmtCs8   ? reinterpret_cast<const void *>(&nofir_bits_kernel<(int)kFmtCs8>)
                         : p.sample_fmt == kFmtCu8 ? reinterpret_cast<const void *>(&nofir_bits_kernel<(int)kFmtCu8>)
                                                   : reinterpret_cast<const void *>(&nofir_bits_kernel<(int)kFmtSc16>);
        const hipError_t e = hipExtLaunchKernel(fn,
                                                dim3((uint32_t)grid, num_captures), dim3(64), args, 0, stream, t0, t1, 0);
        return e != hipSuccess ? e : hipGetLastError();
    }
    if (form == OOKD_FRONT_FIR1_MFMA || form == OOKD_FRONT_FIR1_MFMA_8) {
        return launch_front_mfma(p, num_captures, stream, t0, t1, tile_begin, tile_count);
    }
    if (form == OOKD_FRONT_FIR1_VALU || form == OOKD_FRONT_FIR1_VALU_EXACT) {
        const size_t lds = fir1_lds_bytes(p);
        // whole 4096-output blocks, so every bit word of the capture is written
        const int R = fir1_R(p);
        range((p.n_out + kFirTile - 1) / kFirTile * (kFirTile / (64 * R) / kFirWgWaves), grid, pp);
        if (grid == 0) return hipSuccess;
        const void *fn;
        if (R == kFir1RShort) {
            fn = exact ? reinterpret_cast<const void *>(&fir1_bits_kernel<true, kFir1RShort>)
                       : reinterpret_cast<const void *>(&fir1_bits_kernel<false, kFir1RShort>);
        } else {
            fn = exact ? reinterpret_cast<const void *>(&fir1_bits_kernel<true, kFir1RLong>)
                       : reinterpret_cast<const void *>(&fir1_bits_kernel<false, kFir1RLong>);
        }
        static const size_t lds_pad = dev_getenv("OOKD_FIR1_LDS_PAD") ? (size_t)atoi(dev_getenv("OOKD_FIR1_LDS_PAD")) : 0;   // experiment: caps the waves per CU
        const size_t lds_req = lds + lds_pad;
        hipError_t e = ensure_dynamic_lds(fn, lds_req);
        if (e != hipSuccess) return e;
        e = hipExtLaunchKernel(fn, dim3((uint32_t)grid, num_captures), dim3(64 * kFirWgWaves), args, lds_req, stream, t0, t1, 0);
        return e != hipSuccess ? e : hipGetLastError();
    }
    if (form == OOKD_FRONT_FIR2_MFMA || form == OOKD_FRONT_FIR2_MFMA_8) {
        return launch_front_mfma2(p, num_captures, stream, t0, t1, tile_begin, tile_count);
    }
    if (form == OOKD_FRONT_FIR2_VALU || form == OOKD_FRONT_FIR2_VALU_EXACT) {
        const size_t lds = (size_t)kFir2Waves * Fir2Dec4::wave_bytes;
        range((p.n_out + (uint64_t)kFir2Waves * Fir2Dec4::F - 1) / ((uint64_t)kFir2Waves * Fir2Dec4::F), grid, pp);
        if (grid == 0) return hipSuccess;
        const void *fn = exact ? reinterpret_cast<const void *>(&fir2_bits_kernel<Fir2Dec4, true>)
                               : reinterpret_cast<const void *>(&fir2_bits_kernel<Fir2Dec4, false>);
        const hipError_t e = hipExtLaunchKernel(fn, dim3((uint32_t)grid, num_captures), dim3(64 * kFir2Waves), args, lds,
                                                stream, t0, t1, 0);
        return e != hipSuccess ? e : hipGetLastError();
    }
    if (tile_begin != 0 || tile_count != ~0ull) return hipErrorInvalidValue;     // the generic kernel runs whole captures
    // several kernels: bracket them
    if (t0 && hipEventRecord(t0, stream) != hipSuccess) return hipGetLastError();
    const hipError_t e = launch_front_generic(p, num_captures, stream);
    if (e != hipSuccess) return e;
    if (t1 && hipEventRecord(t1, stream) != hipSuccess) return hipGetLastError();
    return hipSuccess;
}

bool front_sparse_capable(const FrontParams &p) {
    // (round 3: the two-stage kernels too -- their quiet tiles stored 36 bytes each, 150 MB of small stores per
    //  16 GiB capture beside the read stream: the backend default filter ran 15 % behind the 1-stage one for it)
    if (p.tune && p.num_stages) return (front_uses_tuned_fir1(p) || front_uses_tuned_fir2(p)) && p.quiet_lsb > 0 && !p.fir_out;
    return (use_fir1(p) || use_fir2(p)) && p.quiet_lsb > 0 && !p.fir_out;
}

// ---------------------------------------------------------------------------
// sparse front-end output: making the bit words dense again
// ---------------------------------------------------------------------------
// With FrontParams::sparse the tuned kernels (1 stage; 2 x decimate-by-2) store nothing for quiet
// tiles, and what an earlier run left there is told apart by the run stamp in
// the tile info (tile_live): no pass over the tiles between runs (round 2 first
// zeroed the previous run's tiles before every run: 60 us and 107 MB of
// stores per 16 GiB capture, beside another context's front end).  This kernel
// zeroes words + info of every tile that does not carry `keep_stamp_bits` (0:
// every tile with a non-zero info): for readers of the raw words
// (ookd_rx_get_bits), when the run geometry changes, when the stamp wraps.
__global__ __launch_bounds__(256) void clear_tiles_kernel(uint32_t *tile_info, uint64_t *bits, uint64_t ntiles,
                                                          uint32_t tiles_per_cap, uint64_t words_per_cap,
                                                          uint32_t words_per_tile, uint32_t keep_stamp_bits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 4;
    for (uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; t < ntiles; t += stride) {
        const uint4 q = *reinterpret_cast<const uint4 *>(tile_info + t);       // tiles_per_cap is a multiple of 8
        if ((q.x | q.y | q.z | q.w) == 0) continue;
        uint32_t info[4] = {q.x, q.y, q.z, q.w};
        for (uint32_t k = 0; k < 4; ++k) {
            if (!info[k]) continue;
            if (keep_stamp_bits && !((info[k] ^ keep_stamp_bits) & kTileStampMask)) continue;      // this run's
            const uint64_t tt = t + k;
            const uint64_t cap = tt / tiles_per_cap, tile = tt - cap * tiles_per_cap;
            uint64_t *w = bits + cap * words_per_cap + tile * words_per_tile;
            for (uint32_t i = 0; i < words_per_tile; i += 2) *reinterpret_cast<uint4 *>(w + i) = make_uint4(0, 0, 0, 0);
            info[k] = 0;
        }
        *reinterpret_cast<uint4 *>(tile_info + t) = make_uint4(info[0], info[1], info[2], info[3]);
    }
}

hipError_t launch_clear_tiles(uint32_t *tile_info, uint64_t *bits, uint64_t ntiles, uint32_t tiles_per_cap,
                              uint64_t words_per_cap, uint32_t tile_bits, uint32_t keep_stamp_bits, hipStream_t stream) {
    if (ntiles == 0) return hipSuccess;
    uint64_t blocks = (ntiles / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(clear_tiles_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, tile_info, bits, ntiles,
                       tiles_per_cap, words_per_cap, tile_bits / 64u, keep_stamp_bits);
    return hipGetLastError();
}

hipError_t launch_unpack(const void *iq, uint32_t fmt, float *out, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    float2 *o = reinterpret_cast<float2 *>(out);
    if (fmt == kFmtCs8) hipLaunchKernelGGL(unpack_kernel<(int)kFmtCs8>, dim3((uint32_t)blocks), dim3(256), 0, stream, iq, o, n);
    else if (fmt == kFmtCu8) hipLaunchKernelGGL(unpack_kernel<(int)kFmtCu8>, dim3((uint32_t)blocks), dim3(256), 0, stream, iq, o, n);
    else hipLaunchKernelGGL(unpack_kernel<(int)kFmtSc16>, dim3((uint32_t)blocks), dim3(256), 0, stream, iq, o, n);
    return hipGetLastError();
}

hipError_t launch_widen(const void *src, uint32_t fmt, int16_t *dst, uint64_t n, uint32_t num_captures,
                        uint64_t src_stride, uint64_t dst_stride, hipStream_t stream) {
    if (n == 0 || num_captures == 0) return hipSuccess;
    if (fmt != kFmtCs8 && fmt != kFmtCu8) return hipErrorInvalidValue;
    uint64_t blocks = (n / 4 + 256) / 256;
    if (blocks > 4096) blocks = 4096;
    const uint16_t *s = static_cast<const uint16_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    if (fmt == kFmtCs8) {
        hipLaunchKernelGGL(widen_kernel<(int)kFmtCs8>, dim3((uint32_t)blocks, num_captures), dim3(256), 0, stream, s, d, n,
                           src_stride, dst_stride);
    } else {
        hipLaunchKernelGGL(widen_kernel<(int)kFmtCu8>, dim3((uint32_t)blocks, num_captures), dim3(256), 0, stream, s, d, n,
                           src_stride, dst_stride);
    }
    return hipGetLastError();
}

hipError_t launch_pack(const float *in, int16_t *iq, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream,
                       reinterpret_cast<const float2 *>(in), reinterpret_cast<uint32_t *>(iq), n);
    return hipGetLastError();
}

hipError_t launch_synth(const SynthRun *runs, uint64_t num_runs, uint64_t seed, uint32_t noise,
                        uint64_t first, uint64_t count, int16_t *iq, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    uint64_t blocks = (count / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(synth_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, runs, num_runs, seed,
                       noise, first, count, reinterpret_cast<uint32_t *>(iq));
    return hipGetLastError();
}

}  // namespace ookd
