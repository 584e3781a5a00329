// front_dev.hpp -- device code shared by the kernel files with a register-blocked 1-stage FIR (kernels.hip,
// fir_tuned.hip, survey_tuned.hip) and by the survey's sample fetch (survey_dev.hpp): sample unpacking, the
// 1-stage kernels' LDS window layout and wave-private fence, the tap-chunk load into SGPR pairs, the tuned
// contract's tap step and the complex-tap chunk body, and everything behind a tile's accumulators (threshold,
// guard band, bit packing, tile info).  Compiled with -ffp-contract=off: every a*b+c is a separately rounded
// multiply and add; fused multiply-adds are written explicitly.
#pragma once

#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include <utility>

#pragma clang fp contract(off)

namespace ookd {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// complexf.h:68-77: (float)v * (1.0f/2048.0f), exact.
__device__ __forceinline__ float2 unpack_iq(uint32_t w) {
    const float s = 1.0f / 2048.0f;
    float2 r;
    r.x = (float)(int16_t)(w & 0xffffu) * s;
    r.y = (float)(int16_t)(w >> 16) * s;
    return r;
}

// One input sample of a capture as float2, honouring halo (index < 0) and
// zero padding (index >= n_valid; bladeRF_file.c:113-117).
__device__ __forceinline__ float2 fetch_sample(const FrontParams &p, const uint32_t *src,
                                               const float2 *srcf, int64_t n) {
    if (n < 0) {
        const int64_t h = (int64_t)p.halo_len + n;
        if (h < 0) return make_float2(0.0f, 0.0f);
        if (p.halo_f32) return reinterpret_cast<const float2 *>(p.halo_f32)[h];
        if (p.halo) return unpack_iq(reinterpret_cast<const uint32_t *>(p.halo)[h]);
        return make_float2(0.0f, 0.0f);
    }
    if ((uint64_t)n >= p.n_valid) return make_float2(0.0f, 0.0f);
    if (srcf) return srcf[n];
    return unpack_iq(src[n]);
}

// fetch_sample for int16 inputs, returned raw (packed I | Q << 16).
__device__ __forceinline__ uint32_t fetch_raw(const FrontParams &p, const uint32_t *src, int64_t n) {
    if (n < 0) {
        const int64_t h = (int64_t)p.halo_len + n;
        if (h < 0 || !p.halo) return 0u;
        return reinterpret_cast<const uint32_t *>(p.halo)[h];
    }
    if ((uint64_t)n >= p.n_valid) return 0u;
    return src[n];
}

// ---- geometry of the kernels for two decimating stages (fir2_bits_kernel, kernels.hip; fir2_tuned_kernel,
// fir_tuned.hip): one wave = one tile of F final outputs; lane t's block of P = D * R consecutive samples of a level
// starts at slot t * (P + 1) ----
template <int D1_, int N1_, int D2_, int N2_, int R2_>
struct Fir2Geom {
    static constexpr int D1 = D1_, D2 = D2_, R2 = R2_;
    static constexpr int T1 = 16 * N1_, T2 = 16 * N2_;         // padded tap counts
    static constexpr int N1 = N1_, N2 = N2_;
    static constexpr int F = 64 * R2;                           // final outputs per wave
    static constexpr int L1need = D2 * (F - 1) + T2;            // stage-1 outputs stage 2 reads
    static constexpr int R1 = (L1need + 63) / 64;
    static constexpr int L1 = 64 * R1;                          // stage-1 outputs computed
    static constexpr int L0 = D1 * (L1 - 1) + T1;               // input samples read
    static constexpr int P1 = D1 * R1, P2 = D2 * R2;
    static constexpr int kVecs = (L0 + 3 + 3) / 4;              // 16 B loads (the window may start mid-vector)
    static constexpr int kVecRounds = (kVecs + 63) / 64;
    static constexpr int slots0 = (L0 + L0 / P1 + 2 + 1) & ~1;  // level 0 stays RAW: 4 B per sample
    static constexpr int slots1 = L1 + L1 / P2 + 2;             // level 1: float2
    static constexpr int wave_bytes = ((slots0 * 4 + slots1 * 8) + 15) & ~15;
};
typedef Fir2Geom<2, 1, 2, 2, 4> Fir2Dec4;      // fs128_fs16_dec4: (D 2, 16 taps), (D 2, 32 taps)

// ookiedokie.c:171-179: bit = sqrtf(re*re + im*im) >= thr.  sqrtf is
// correctly rounded and monotone, so this equals power >= P*, P* being the
// smallest float whose sqrtf is >= thr (host computes it).  The power keeps
// the reference's three roundings (complexf.h:45).
__device__ __forceinline__ float power_ref(float re, float im) {
    const float rr = re * re;
    const float ii = im * im;
    return rr + ii;
}

// ---- LDS window of the 1-stage kernels ----------------------------------------
// sample j lives at slot j + (j / R): one pad slot per R samples (R = outputs per lane, a power of two)
// makes the lane stride R + 1 float2, which is conflict free for ds_read_b64 (32-lane halves, 64 banks),
// and keeps every read of the unrolled MAC bodies at  lane_base + compile-time immediate.
template <int R>
__host__ __device__ __forceinline__ uint32_t slot(uint32_t j) { return j + j / (uint32_t)R; }

// float2 slots of one wavefront's private window (kept a multiple of 2 = 16 B)
template <int R>
__host__ __device__ __forceinline__ uint32_t fir1_wave_slots(uint32_t Tp) {
    return (slot<R>(64u * R + Tp) + 2u) & ~1u;
}

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v8f __attribute__((ext_vector_type(8)));
typedef short v2s __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// non-temporal 16 B load: the capture is streamed through once (tools/stream_bw.hip: +7 % over plain loads)
__device__ __forceinline__ uint4 ld_nt4(const uint4 *p) {
    const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ v2s as_v2s(uint32_t w) { return __builtin_bit_cast(v2s, w); }

// One 16-byte vector v of an interior window, unpacked into its slots: 4 SC16Q11 samples or 8 8-bit ones.  They
// never straddle a pad slot (R is 8 or 16).
template <int FMT, int R>
__device__ __forceinline__ void store_unpacked(float2 *lds, uint32_t v, uint4 q) {
    if (FMT == (int)kFmtSc16) {
        float2 *dst = lds + slot<R>(4u * v);
        dst[0] = unpack_iq(q.x);
        dst[1] = unpack_iq(q.y);
        dst[2] = unpack_iq(q.z);
        dst[3] = unpack_iq(q.w);
    } else {
        float2 *dst = lds + slot<R>(8u * v);
        dst[0] = unpack_iq(widen8<FMT>(q.x & 0xffffu));
        dst[1] = unpack_iq(widen8<FMT>(q.x >> 16));
        dst[2] = unpack_iq(widen8<FMT>(q.y & 0xffffu));
        dst[3] = unpack_iq(widen8<FMT>(q.y >> 16));
        dst[4] = unpack_iq(widen8<FMT>(q.z & 0xffffu));
        dst[5] = unpack_iq(widen8<FMT>(q.z >> 16));
        dst[6] = unpack_iq(widen8<FMT>(q.w & 0xffffu));
        dst[7] = unpack_iq(widen8<FMT>(q.w >> 16));
    }
}

// Orders a wavefront's LDS writes against its own later reads (or the other way round) where the memory is
// private to the wave: the LDS executes one wave's accesses in order, so no workgroup barrier is needed -- this
// only keeps the compiler from moving accesses across it.  Each call site says why its memory is wave-private.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 32 floats at tp (wave-uniform, 4-byte aligned) -> 16 SGPR pairs: 32 real taps, or 16 complex ones as (re, im).
__device__ __forceinline__ void load_tap_chunk32(const float *tp, v2f *tpair) {
    v8f ta, tb, tc, td;
    asm volatile("s_load_dwordx8 %0, %4, 0x0\n\t"
                 "s_load_dwordx8 %1, %4, 0x20\n\t"
                 "s_load_dwordx8 %2, %4, 0x40\n\t"
                 "s_load_dwordx8 %3, %4, 0x60\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(ta), "=&s"(tb), "=&s"(tc), "=&s"(td)
                 : "s"(tp)
                 : "memory");
    tpair[0] = __builtin_shufflevector(ta, ta, 0, 1);
    tpair[1] = __builtin_shufflevector(ta, ta, 2, 3);
    tpair[2] = __builtin_shufflevector(ta, ta, 4, 5);
    tpair[3] = __builtin_shufflevector(ta, ta, 6, 7);
    tpair[4] = __builtin_shufflevector(tb, tb, 0, 1);
    tpair[5] = __builtin_shufflevector(tb, tb, 2, 3);
    tpair[6] = __builtin_shufflevector(tb, tb, 4, 5);
    tpair[7] = __builtin_shufflevector(tb, tb, 6, 7);
    tpair[8] = __builtin_shufflevector(tc, tc, 0, 1);
    tpair[9] = __builtin_shufflevector(tc, tc, 2, 3);
    tpair[10] = __builtin_shufflevector(tc, tc, 4, 5);
    tpair[11] = __builtin_shufflevector(tc, tc, 6, 7);
    tpair[12] = __builtin_shufflevector(td, td, 0, 1);
    tpair[13] = __builtin_shufflevector(td, td, 2, 3);
    tpair[14] = __builtin_shufflevector(td, td, 4, 5);
    tpair[15] = __builtin_shufflevector(td, td, 6, 7);
}

// ---- complex taps: the tuned contract (include/ookiedokie_amd.h at ookd_filter_tuned_taps) --------------------
// One tap c = (cr, ci) on sample x of one stage output, float32, unfused, tap 0 on the newest sample, the
// accumulators from +0: the contract's four statements, in its order.  This is the only copy; every kernel that
// computes the contract's value calls it (the generic tuned front end and survey, the guard-band recompute).
__device__ __forceinline__ void tuned_step(float &ar, float &ai, float cr, float ci, float2 x) {
    ar = ar + cr * x.x;
    ar = ar - ci * x.y;
    ai = ai + cr * x.y;
    ai = ai + ci * x.x;
}

// acc(re, im) += c * x for one complex tap c = tp (re, im) held in an SGPR pair, two components at a time:
//   (ar, ai) += (cr, cr) * (xr, xi)            op_sel_hi:[0,1(,1)]: both halves read tp.lo
//   (ar, ai) += (-ci, ci) * (xi, xr)           both halves read tp.hi, x's halves swapped, the low product negated
//   fused : two v_pk_fma_f32, one rounding per step (four FMAs per sample-tap where cmac, kernels.hip, has two)
//   exact : v_pk_mul_f32 then v_pk_add_f32 twice, every product and every sum rounded on its own -- tuned_step's
//           four statements: ar receives cr*xr first and ci*xi second (x + (-y) is x - y bit for bit), ai cr*xi
//           first and ci*xr second
template <bool EXACT>
__device__ __forceinline__ void cmac_tuned(v2f &acc, v2f tp, v2f x) {
    if (EXACT) {
        v2f p1, p2;
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(p1) : "s"(tp), "v"(x));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(p1));
        asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[1,0]" : "=v"(p2) : "s"(tp), "v"(x));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(p2));
    } else {
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(tp), "v"(x));
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(acc) : "s"(tp), "v"(x));
    }
}

// Compile-time unrolled body of one chunk of kTunedChunk = 16 complex taps.  Window position W (newest first)
// feeds output r with tap kk = r - W when 0 <= kk < 16, so every output receives its taps in ascending order.
template <bool EXACT, int R, int W, int... Rs>
__device__ __forceinline__ void tuned_wstep(v2f *acc, const v2f *tpair, const v2f *base,
                                            std::integer_sequence<int, Rs...>) {
    constexpr int cp = W + kTunedChunk;                 // 1 .. R + 15
    const v2f x = base[cp + cp / R];
    ((void)((Rs - W >= 0 && Rs - W < kTunedChunk) ? (cmac_tuned<EXACT>(acc[Rs], tpair[(Rs - W) & 15], x), 0) : 0), ...);
}

template <bool EXACT, int R, int... Ws>
__device__ __forceinline__ void tuned_chunk(v2f *acc, const v2f *tpair, const v2f *base,
                                            std::integer_sequence<int, Ws...>) {
    (tuned_wstep<EXACT, R, R - 1 - Ws>(acc, tpair, base, std::make_integer_sequence<int, R>{}), ...);
}

// Everything behind the accumulators of one wave tile of a 1-stage kernel (lane `tid` holds outputs
// t0 + R tid .. + R - 1 in acc): threshold + guard band, bit packing, optional float output.  `exact(r)`
// recomputes the lane's output r in the reference's (the contract's) unfused order.  Stores the tile's bit
// words and returns the tile info word (level changes inside the tile | first bit << 30 | last bit << 31).
// (fir1_bits_kernel keeps its own inlined copy of this text in fir1_tile_compute, kernels.hip: routed through this
// function its register allocation moved, and its instruction stream is pinned by measurements.)
template <bool EXACT, int R, typename Exact>
__device__ __forceinline__ uint32_t fir1_tile_finish(const FrontParams &p, const v2f *acc, uint64_t t0, uint32_t tid,
                                                     uint32_t cap, uint64_t *words, Exact exact) {
    uint32_t info = 0;
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
            const float2 y = exact(r);
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

// ---- generic kernels: the slice of every level one tile of final outputs needs ----------
// Level 0 is the unpacked input, level s+1 the output of stage s.  Stage output J (global) reads
// level-s inputs D*(J+1)-1-k (fir.c:290: the countdown starts at D, so the first output is at
// input index D-1).
struct GenLevel {
    int64_t a;          // first local index needed at this level
    uint32_t len;       // samples needed
};

__device__ __forceinline__ void gen_levels(const FrontParams &p, int64_t j0, uint32_t L,
                                           GenLevel *lv, int64_t *off) {
    // global origin of each level: g_{s+1} = floor(g_s / D_s)
    uint64_t g = p.origin;
    const int S = (int)p.num_stages;
    for (int s = 0; s < S; ++s) {
        const uint64_t D = p.stage[s].decim;
        const uint64_t gn = g / D;
        off[s] = (int64_t)(D * gn + D - 1) - (int64_t)g;    // = D-1-(g mod D)
        g = gn;
    }
    lv[S].a = j0;
    lv[S].len = L;
    for (int s = S - 1; s >= 0; --s) {
        const int64_t D = p.stage[s].decim;
        const int64_t T = p.stage[s].ntaps;
        lv[s].a = D * lv[s + 1].a + off[s] - (T - 1);
        lv[s].len = (uint32_t)(D * ((int64_t)lv[s + 1].len - 1) + T);
    }
}

}  // namespace ookd
