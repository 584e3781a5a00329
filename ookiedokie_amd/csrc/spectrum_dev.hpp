// spectrum_dev.hpp -- the 1024-point Hann frame transform of one wave (gfx950, wave64), shared by spectrum.hip (the
// Welch spectrum of whole captures) and burst_spectra.hip (the same over the frames of every burst).  Device code
// only; the host-built tables are spectrum_tables() in kernels.hpp / spectrum.cpp.
//
//   unpack (v / 2048, 16 v for the 8-bit formats first) -> periodic Hann -> X[k] = sum_n w[n] x[n] e^{-j 2 pi k n / 1024}
//
// The raw frame of a lane is sample n = 256 j + 4 L + i, j, i = 0..3.  1024 = 4 x 16 x 16, decimation in frequency:
//
//   A. over j, in registers: k = kj + 4 k', y_kj[r] = W1024^(r kj) sum_j x[r + 256 j] W4^(j kj), r = 4 L + i;
//      what is left are four 256-point transforms X[kj + 4 k'] = FFT256(y_kj)[k'].
//   B. exchange through LDS: lane (kj, s) takes y_kj[s + 16 t], t = 0..15, and computes
//      z[kt] = W256^(s kt) sum_t y_kj[s + 16 t] W16^(t kt)          (16 points in registers, radix 4 x 4)
//   C. exchange through LDS: lane l = kj + 4 kt takes z_kj[s][kt], s = 0..15, and computes
//      X[l + 64 ks] = sum_s W16^(s ks) z_kj[s][kt]                   (16 points in registers)
//
// so lane l ends with bins l + 64 ks.  Both exchanges use the wave's own 8.5 KiB of LDS and 8-byte accesses, laid
// out after the LDS banking rules (ds_write_b64: 16 consecutive lanes over 32 dword banks; ds_read_b64: 32 lanes
// over 64) so that no access should collide -- B: y_kj[4 L + i] at kj * 272 + i * 68 + L, 16 lanes write 128
// contiguous bytes, and the 32 lanes (two kj, sixteen s) of a read fall on 64 different banks; C: s rows of 65
// float2.  A wave is in lockstep and its LDS operations complete in order, so no workgroup barrier is needed
// between frames.  The twiddles and the window come from tables the host builds in double and rounds to float,
// copied to LDS once per workgroup and laid out in the order the lanes read them (SpectrumParams::twiddle):
// W1024^((4 L + i) kj) at (kj - 1) * 256 + i * 64 + L, W256^(s kt) at 768 + 16 kt + s, so a read is contiguous
// across the lanes (the four kj of step B read the same address).  No sincosf.
//
// Multiplications by twiddles are written with explicit fmaf (every kernel of the library is compiled with
// -ffp-contract=off; nothing is fused that is not spelled out).
#pragma once

#include "kernels.hpp"
#include "common.hpp"

#pragma clang fp contract(off)

namespace ookd {

constexpr int kSpecQuarter = 68;                // float2 per i quarter of a kj plane of exchange B: 64 + 4
constexpr int kSpecPlane = 4 * kSpecQuarter;    // float2 per kj plane: 272 (odd planes sit 32 banks on)
constexpr int kSpecRow = 65;                    // float2 per s row of exchange C: 64 + 1
constexpr int kSpecXchg = 4 * kSpecPlane;       // float2 per wave (>= 16 * kSpecRow)
static_assert(kSpecXchg >= 16 * kSpecRow, "exchange C fits the wave's region");
static_assert((size_t)kSpecWaves * kSpecXchg * sizeof(float2) >= (size_t)kSpecBins * sizeof(double),
              "the workgroup's final sums fit the exchange regions");

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * w: two products and two fused multiply-adds
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(__fmaf_rn(a.x, w.x, -(a.y * w.y)), __fmaf_rn(a.x, w.y, a.y * w.x));
}
// a * (-j)
__device__ __forceinline__ float2 mulmj(float2 a) { return make_float2(a.y, -a.x); }

// X[k] = sum_n a_n W4^(n k), W4 = -j
__device__ __forceinline__ void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 b0 = cadd(a0, a2), b1 = csub(a0, a2), b2 = cadd(a1, a3), b3 = mulmj(csub(a1, a3));
    a0 = cadd(b0, b2);
    a1 = cadd(b1, b3);
    a2 = csub(b0, b2);
    a3 = csub(b1, b3);
}

// a * W16^M, W16 = e^{-j 2 pi / 16}; the constants are the doubles rounded to float
template <int M>
__device__ __forceinline__ float2 mulw16(float2 a) {
    constexpr float c1 = 0.92387953251128673848f;   // cos(pi / 8)
    constexpr float s1 = 0.38268343236508978178f;   // sin(pi / 8)
    constexpr float h = 0.70710678118654752440f;    // sqrt(1/2)
    if (M == 0) return a;
    if (M == 1) return cmul(a, make_float2(c1, -s1));
    if (M == 2) return cmul(a, make_float2(h, -h));
    if (M == 3) return cmul(a, make_float2(s1, -c1));
    if (M == 4) return mulmj(a);
    if (M == 6) return cmul(a, make_float2(-h, -h));
    return cmul(a, make_float2(-c1, s1));           // M == 9
}

// in place, natural order: v[k] = sum_n v[n] W16^(n k).  n = r + 4 j, k = kj + 4 k':
// u_r[kj] = W16^(r kj) sum_j v[r + 4 j] W4^(j kj);  X[kj + 4 k'] = sum_r u_r[kj] W4^(r k')
__device__ __forceinline__ void fft16(float2 (&v)[16]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dft4(v[r], v[r + 4], v[r + 8], v[r + 12]);      // v[r + 4 kj] = u_r[kj] untwiddled
    v[5] = mulw16<1>(v[5]);
    v[9] = mulw16<2>(v[9]);
    v[13] = mulw16<3>(v[13]);
    v[6] = mulw16<2>(v[6]);
    v[10] = mulw16<4>(v[10]);
    v[14] = mulw16<6>(v[14]);
    v[7] = mulw16<3>(v[7]);
    v[11] = mulw16<6>(v[11]);
    v[15] = mulw16<9>(v[15]);
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) dft4(v[4 * kj], v[4 * kj + 1], v[4 * kj + 2], v[4 * kj + 3]);
    // v[4 kj + k'] holds X[kj + 4 k']: transpose the 4 x 4
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a + 1; b < 4; ++b) {
            const float2 t = v[4 * a + b];
            v[4 * a + b] = v[4 * b + a];
            v[4 * b + a] = t;
        }
}

// the raw frame of a lane: sample (j, i) = n = 256 j + 4 L + i.  SC16Q11: one dword per sample, w[4 j + i];
// 8-bit: two bytes per sample, two samples per dword, w[2 j + i / 2]
template <int FMT>
struct RawFrame {
    static constexpr int kWords = FMT == (int)kFmtSc16 ? 16 : 8;
    uint32_t w[kWords];
};

// the frame that begins `frame` frames behind src.  ALIGNED: src is on a 16-byte boundary (8 for the 8-bit formats),
// one vector load per lane and quarter; otherwise single samples.  Reads exactly the frame's 1024 samples.
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void load_frame(RawFrame<FMT> &raw, const unsigned char *src, uint64_t frame,
                                           uint32_t lane) {
    const unsigned char *base = src + frame * (uint64_t)(kSpecBins * sample_bytes((uint32_t)FMT));
    if (FMT == (int)kFmtSc16) {
        if (ALIGNED) {
            const uint4 *q = reinterpret_cast<const uint4 *>(base);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 t = q[64 * j + lane];
                raw.w[4 * j] = t.x;
                raw.w[4 * j + 1] = t.y;
                raw.w[4 * j + 2] = t.z;
                raw.w[4 * j + 3] = t.w;
            }
        } else {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(base);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) raw.w[4 * j + i] = q[256 * j + 4 * lane + i];
        }
    } else {
        if (ALIGNED) {
            const uint2 *q = reinterpret_cast<const uint2 *>(base);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint2 t = q[64 * j + lane];
                raw.w[2 * j] = t.x;
                raw.w[2 * j + 1] = t.y;
            }
        } else {
            const uint16_t *q = reinterpret_cast<const uint16_t *>(base);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    raw.w[2 * j + i] = (uint32_t)q[256 * j + 4 * lane + 2 * i] |
                                       ((uint32_t)q[256 * j + 4 * lane + 2 * i + 1] << 16);
        }
    }
}

template <int FMT>
__device__ __forceinline__ float2 frame_sample(const RawFrame<FMT> &raw, int j, int i) {
    const float s = 1.0f / 2048.0f;
    uint32_t w;
    if (FMT == (int)kFmtSc16) w = raw.w[4 * j + i];
    else w = widen8<FMT>((raw.w[2 * j + i / 2] >> (16 * (i & 1))) & 0xffffu);
    return make_float2((float)(int16_t)(w & 0xffffu) * s, (float)(int16_t)(w >> 16) * s);
}

// orders this wave's LDS traffic across an exchange (the lanes of a wave run in lockstep)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The tables of a workgroup in LDS: s_tw[1024] and s_win[1024], filled from SpectrumParams' twiddle and window by
// all kSpecThreads threads; the caller's __syncthreads() follows.
__device__ __forceinline__ void load_spectrum_tables(float2 *s_tw, float *s_win, const float2 *twiddle,
                                                     const float *window, uint32_t tid) {
    for (uint32_t i = tid; i < (uint32_t)kSpecBins; i += kSpecThreads) {
        s_tw[i] = twiddle[i];
        s_win[i] = window[i];
    }
}

// Window and steps A-C over one raw frame: v[ks] receives X[lane + 64 ks].  xw is the wave's own exchange region
// (kSpecXchg float2), free again on return.
template <int FMT>
__device__ __forceinline__ void frame_transform(const RawFrame<FMT> &raw, float2 (&v)[16], float2 *xw,
                                                const float2 *s_tw, const float *s_win, uint32_t lane) {
    const uint32_t b_kj = lane >> 4, b_s = lane & 15u;      // this lane's 16-point transform of step B
    // window, step A: v[4 j + i], then v[4 kj + i]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 w = reinterpret_cast<const float4 *>(s_win)[64 * j + lane];
        const float wi[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 x = frame_sample<FMT>(raw, j, i);
            v[4 * j + i] = make_float2(x.x * wi[i], x.y * wi[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dft4(v[i], v[4 + i], v[8 + i], v[12 + i]);
#pragma unroll
        for (int kj = 1; kj < 4; ++kj) v[4 * kj + i] = cmul(v[4 * kj + i], s_tw[(kj - 1) * 256 + i * 64 + lane]);
    }
    // exchange B: y_kj[4 L + i] at kj * 272 + i * 68 + L; r = s + 16 t is i = s & 3, L = (s >> 2) + 4 t
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int i = 0; i < 4; ++i) xw[kj * kSpecPlane + i * kSpecQuarter + lane] = v[4 * kj + i];
    wave_lds_sync();
    {
        const float2 *yb = xw + b_kj * kSpecPlane + (b_s & 3u) * kSpecQuarter + (b_s >> 2);
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = yb[4 * t];
    }
    fft16(v);
#pragma unroll
    for (int kt = 1; kt < 16; ++kt) v[kt] = cmul(v[kt], s_tw[768 + 16 * kt + b_s]);
    wave_lds_sync();
    // exchange C: z_kj[s][kt] at s * 65 + 4 kt + kj
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) xw[b_s * kSpecRow + 4 * kt + b_kj] = v[kt];
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; ++s) v[s] = xw[s * kSpecRow + lane];
    wave_lds_sync();
    fft16(v);
}

// pw[ks] += |v[ks]|^2, the one form of the sum both kernels use
__device__ __forceinline__ void add_frame_power(float (&pw)[16], const float2 (&v)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) pw[k] = pw[k] + __fmaf_rn(v[k].x, v[k].x, v[k].y * v[k].y);
}

}  // namespace ookd
