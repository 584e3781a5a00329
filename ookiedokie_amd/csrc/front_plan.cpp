// front_plan.cpp -- plan_front: everything about an rx context's front end that its creation arguments decide,
// computed on the host without a device (front_plan.hpp).  The bits are the reference's by construction only if
// these numbers are right: tests/test_front_plan_host.py holds every one of them against recorded values.
#include <algorithm>
#include <cstring>
#include <string>

#include "front_plan.hpp"

namespace ookd {

namespace {

// smallest float p with sqrtf(p) >= thr  (SURVEY.md hard part 3)
float power_threshold(float thr) {
    if (std::isnan(thr)) return NAN;
    if (thr <= 0.0f) return 0.0f;
    if (std::isinf(thr)) return INFINITY;
    float p = (float)((double)thr * (double)thr);
    while (p > 0.0f && sqrtf(nextafterf(p, 0.0f)) >= thr) p = nextafterf(p, 0.0f);
    while (!std::isinf(p) && sqrtf(p) < thr) p = nextafterf(p, INFINITY);
    return p;
}

// Guard band for the fused-multiply-add FIR (1 stage): any sample whose
// FMA-computed power lies in [p_lo, p_hi) is recomputed in reference order.
// e bounds |y_fma - y_ref| per component: both chains are within
// gamma_T * sum|h||x| of the exact sum (one rounding per step for fma, two
// for mul+add), inputs are bounded by x_max = 32768/2048 = 16 (in units of 2048 LSB; 1 for a tile whose samples
// all lie within +-2048).
//
// Several stages: the fused and the reference chain of stage s+1 start from
// inputs that already differ by e_s, which the stage amplifies by at most
// sum|h_{s+1}|, and add their own rounding difference on values bounded by
// 16 * prod sum|h|:  e = 2.2 u * 16 * prod_s S_s * sum_s (T_s + 1).
double guard_error(const std::vector<FilterStage> &stages, double x_max) {
    const double u = std::ldexp(1.0, -24);
    double S = 1.0, T = 0.0, Tsum = 0.0;
    for (const auto &st : stages) {
        double ss = 0.0;
        for (float t : st.taps) ss += std::fabs((double)t);
        S *= std::max(ss, 1.0);         // a stage with gain < 1 still adds its own roundings
        T += (double)st.taps.size() + 1.0;
        Tsum += (double)st.taps.size();
    }
    return 2.2 * T * u * S * x_max * (stages.size() > 1 ? 1.01 : 1.0) + Tsum * std::ldexp(1.0, -140);
}

// [p_lo, p_hi) around p_star for a filter output known to within e per component
void band_from_error(double e, float p_star, float &p_lo, float &p_hi) {
    if (std::isnan(p_star) || std::isinf(p_star) || p_star <= 0.0f) {
        p_lo = p_hi = p_star;
        return;
    }
    const double u = std::ldexp(1.0, -24);
    const double P = (double)p_star;
    // |p_ref - p_fma| <= m(p) = 3.003*e*sqrt(p) + 3e^2 + 6u*p
    // upper edge: smallest s = sqrt(p) with (1-6u)s^2 - 3.003e s - (3e^2 + P) >= 0
    {
        const double a = 1.0 - 6.0 * u, b = 3.003 * e, c = 3.0 * e * e + P;
        double s = (b + std::sqrt(b * b + 4.0 * a * c)) / (2.0 * a);
        double ph = s * s * (1.0 + 1e-6);
        ph = std::max(ph, 4.0 * e * e);     // p - m(p) is increasing beyond ~2.3e^2
        float f = (float)ph;
        if ((double)f < ph) f = nextafterf(f, INFINITY);
        f = nextafterf(f, INFINITY);
        p_hi = std::max(f, p_star);
    }
    // lower edge: largest s with (1+6u)s^2 + 3.003e s + 3e^2 - P < 0
    {
        const double a = 1.0 + 6.0 * u, b = 3.003 * e, c = 3.0 * e * e - P;
        if (c >= 0.0) {
            p_lo = 0.0f;
        } else {
            double s = (-b + std::sqrt(b * b - 4.0 * a * c)) / (2.0 * a);
            double pl = s > 0.0 ? s * s * (1.0 - 1e-6) : 0.0;
            float f = (float)pl;
            if ((double)f > pl) f = nextafterf(f, 0.0f);
            f = nextafterf(f, 0.0f);
            p_lo = std::max(f, 0.0f);
        }
    }
}

// stages and their (padded) real taps
bool plan_filter(FrontPlan &pl, const ookd_filter &filter) {
    if (filter.stages.size() > (size_t)kMaxStages) {
        set_error("filter has %zu stages, this build supports %d", filter.stages.size(), kMaxStages);
        return false;
    }
    pl.fp.num_stages = (uint32_t)filter.stages.size();
    pl.total_decim = filter.total_decimation;
    uint64_t mult = 1;
    for (uint32_t s = 0; s < pl.fp.num_stages; ++s) {
        const auto &st = filter.stages[s];
        FirStageDev d{};
        d.decim = st.decimation;
        d.ntaps = (uint32_t)st.taps.size();
        d.ntaps_pad = ((d.ntaps + kTapChunk - 1) / kTapChunk) * kTapChunk;
        d.tap_off = (uint32_t)pl.taps.size();
        pl.taps.insert(pl.taps.end(), st.taps.begin(), st.taps.end());
        // zero padding keeps sums bit-identical: acc + (+-0) == acc
        pl.taps.resize(d.tap_off + d.ntaps_pad, 0.0f);
        pl.fp.stage[s] = d;
        pl.halo_needed += (uint64_t)(d.ntaps - 1) * mult;
        mult *= d.decim;
    }
    return true;
}

// The matrix-core form of the front end (fir_mfma.hip) for the taps prepared in pl.mfma, whose output is known to
// within e_n (inputs up to 1, in units of 2048 LSB) or e_w (up to 16) per component.  Filters the band
// scaling does not suit stay on the packed-VALU kernels.
MfmaUse plan_mfma(FrontPlan &pl, double e_n, double e_w) {
    FrontParams &fp = pl.fp;
    const MfmaTaps &mt = pl.mfma;
    pl.err_n = e_n;
    pl.err_w = e_w;
    float lo_n, hi_n, lo_w, hi_w;
    band_from_error(e_n, fp.p_star, lo_n, hi_n);
    band_from_error(e_w, fp.p_star, lo_w, hi_w);
    // the kernel compares in accumulator units; thresholds so far from the filter's range that the
    // power-of-two scaling leaves the normal floats stay on the packed-VALU loop
    if (!(mfma_scale_band(mt, lo_n, fp.p_lo_n) && mfma_scale_band(mt, hi_n, fp.p_hi_n) &&
          mfma_scale_band(mt, lo_w, fp.p_lo_w) && mfma_scale_band(mt, hi_w, fp.p_hi_w))) {
        return MfmaUse::kBandScale;
    }
    // fl(y^2) = c^2 fl(z^2) needs y^2 clear of the subnormals (and of overflow) wherever it decides a bit
    if (fp.p_star > 0.0f && !(fp.p_star >= 0x1p-100f && fp.p_star <= 0x1p100f)) return MfmaUse::kThresholdRange;
    fp.mfma_c = mt.c;
    // wave tiles per wave of a workgroup: more for the long filters, whose workgroups fill a CU and
    // fetch a 20 / 36 KB image each (config2 sweep: 474 / 545 / 599 / 623 / 635 Gsamples/s at 2 / 4 / 8 / 16 / 32)
    fp.mfma_g = mt.ksteps <= 6 ? 4u : mt.ksteps <= 10 ? 16u : 32u;
    if (const char *g = dev_getenv("OOKD_MFMA_G")) fp.mfma_g = (uint32_t)std::min(4096, std::max(1, atoi(g)));
    // one contiguous run of tiles per XCD: where the halo is a good share of a tile's window -- the decimate-by-4
    // filter (96 of 1120 samples: 3.0 -> 2.8-2.9 ms per 16 GiB) and the long 1-stage filters (272 of 1296: 1 %)
    fp.mfma_xcd = 2u | (mt.ksteps >= 10 ? 1u : 0u);
    if (const char *x = dev_getenv("OOKD_MFMA_XCD")) fp.mfma_xcd = (uint32_t)atoi(x);
    return MfmaUse::kTaken;
}

// Guard band of the tuned kernels (1 stage / decimation 1, and 2 x decimation 2; the generic kernel
// always computes in reference order and ignores it), and the matrix-core form where the shape has one
// and the caller does not ask for the packed-VALU loop.
MfmaUse plan_real_form(FrontPlan &pl, const ookd_filter &filter, uint32_t flags) {
    FrontParams &fp = pl.fp;
    const auto &st = filter.stages;
    pl.err_valu = guard_error(st, 16.0);
    band_from_error(pl.err_valu, fp.p_star, fp.p_lo, fp.p_hi);
    if ((flags & OOKD_RX_FIR_VALU) || dev_getenv("OOKD_FIR_VALU")) return MfmaUse::kValuAsked;
    if (fp.num_stages == 2 && fp.stage[0].decim == 2 && fp.stage[1].decim == 2 &&
        mfma_prepare_taps2(st[0].taps.data(), fp.stage[0].ntaps, st[1].taps.data(), fp.stage[1].ntaps, pl.mfma)) {
        // the backend default shape (two decimate-by-2 stages) folded into one decimate-by-4 product
        return plan_mfma(pl, mfma_error_bound2(pl.mfma, guard_error(st, 1.0), false),
                         mfma_error_bound2(pl.mfma, guard_error(st, 16.0), true));
    }
    // 1 stage, decimation 1, <= 256 taps
    if (fp.num_stages == 1 && fp.stage[0].decim == 1 && mfma_prepare_taps(st[0].taps.data(), fp.stage[0].ntaps, pl.mfma)) {
        return plan_mfma(pl, mfma_error_bound(pl.mfma, fp.stage[0].ntaps, false), mfma_error_bound(pl.mfma, fp.stage[0].ntaps, true));
    }
    pl.mfma = MfmaTaps{};
    return MfmaUse::kShape;
}

// The quiet shortcut: input levels below quiet_lsb cannot reach the threshold.
void plan_quiet_skip(FrontPlan &pl, const ookd_filter &filter, float threshold, uint32_t flags) {
    if (!(threshold > 0.0f) || !std::isfinite(threshold) || (flags & OOKD_RX_NO_QUIET_SKIP)) return;
    // |y_re|, |y_im| <= S * m with S = prod over stages of sum|h|, m = max |component| in
    // the window, so |y| <= sqrt(2) * S * m; 0.1 % slack covers every rounding of the
    // reference's float arithmetic (relative 1e-5 at most) many times over
    double S = 1.0;
    for (const auto &st : filter.stages) {
        double ss = 0.0;
        for (float t : st.taps) ss += std::fabs((double)t);
        S *= ss;
    }
    if (S > 0.0) {
        // |v| < quiet_lsb  <=>  |v|/2048 < level (complexf.h:68-77 scaling)
        const double lvl = (double)threshold * 0.999 / (1.41421356237309515 * S) * 2048.0;
        pl.fp.quiet_lsb = lvl >= 32767.0 ? 32767 : (int)std::ceil(lvl);
    }
}

// Guard band of a tuned carrier.  One component of an output is a sum of 2T products (T taps, a real and an
// imaginary tap part each), sum_k |terms| <= S x_max with S = sum_k (|re[k]| + |im[k]|) and x_max = 16
// (32768 / 2048).  The fused chain rounds once per step, the contract's chain twice (product, sum): both stay
// within gamma_{2T} resp. gamma_{2T+1} of the exact sum times sum|terms| (gamma_n = n u / (1 - n u), u = 2^-24), so
// they differ by at most (4T + 1) u S x_max (1 + O(T u)) <= 2.2 (2T + 1) u S x_max -- guard_error's form with twice
// the roundings per tap and both tap parts in S; the 2^-140 term covers products and sums that round in the
// subnormals.  band_from_error turns it into [p_lo, p_hi) as for the real-tap kernels.  Several stages: as
// guard_error (each stage amplifies what it is handed by at most its S and adds its own term); the generic tuned
// kernel computes in the contract's order and needs no band, the figure is reported all the same.
double tuned_guard_error(const std::vector<std::vector<float>> &re, const std::vector<std::vector<float>> &im, double x_max) {
    const double u = std::ldexp(1.0, -24);
    double S = 1.0, T = 0.0, Tsum = 0.0;
    for (size_t s = 0; s < re.size(); ++s) {
        double ss = 0.0;
        for (size_t k = 0; k < re[s].size(); ++k) ss += std::fabs((double)re[s][k]) + std::fabs((double)im[s][k]);
        S *= std::max(ss, 1.0);
        T += 2.0 * (double)re[s].size() + 1.0;
        Tsum += 2.0 * (double)re[s].size();
    }
    return 2.2 * T * u * S * x_max * (re.size() > 1 ? 1.01 : 1.0) + Tsum * std::ldexp(1.0, -140);
}

// Quiet test of fir1_tuned_kernel.  For any constant d:  y = sum_k c[k] (x[n-k] - d) + d sum_k c[k], so
//     |y| <= A max|x - d| + G |d|,   A = sum_k |c[k]|,  G = |sum_k c[k]|  (the rounded taps' response at 0 Hz).
// The kernel takes d = the midpoint of the window's component ranges: with a = the larger range and b = the
// larger |min + max| (raw LSB), max|x - d| <= sqrt(2) a / 2 and |d| <= sqrt(2) b / 2.  The contract's float chain
// is within gamma_{2T+1} S x_max of y per component (S as above, x_max <= (a + b) / 2 LSB), sqrt(2) times that in
// magnitude.  So the computed |y| stays below the threshold when
//     sqrt(2) / (2 * 2048) * ((A + e) a + (G + e) b) < 0.999 thr,      e = 1.01 (2T + 1) u S,
// the 0.1 % covering the power's own three roundings and this test's float evaluation.  Only interior windows
// are tested (every sample a capture sample), and only the 1-stage kernel has the test.
bool tuned_quiet_weights(const std::vector<float> &re, const std::vector<float> &im, float threshold, uint32_t flags,
                         float &quiet_a, float &quiet_b) {
    if (!(threshold > 0.0f) || !std::isfinite(threshold) || (flags & OOKD_RX_NO_QUIET_SKIP)) return false;
    double A = 0.0, S = 0.0, gr = 0.0, gi = 0.0;
    for (size_t k = 0; k < re.size(); ++k) {
        A += std::hypot((double)re[k], (double)im[k]);
        S += std::fabs((double)re[k]) + std::fabs((double)im[k]);
        gr += (double)re[k];
        gi += (double)im[k];
    }
    if (!(A > 0.0)) return false;
    const double G = std::hypot(gr, gi) + 1e-12 * S;        // (the double sums' own rounding)
    const double e = 1.01 * (2.0 * (double)re.size() + 1.0) * std::ldexp(1.0, -24) * S;
    const double scale = 1.41421356237309515 / (2.0 * 2048.0) / (0.999 * (double)threshold);
    const double qa = (A + e) * scale, qb = (G + e) * scale;
    if (!(qa < 1e30) || !(qb < 1e30)) return false;
    quiet_a = nextafterf((float)qa, INFINITY);
    quiet_b = nextafterf((float)qb, INFINITY);
    return true;
}

// Quiet test of fir2_tuned_kernel: the same bound through two stages.  For any constant d and exact arithmetic
//     y1 = sum_k c1[k] (x - d) + d C1,      y2 = sum_k c2[k] (y1 - d C1) + d C1 C2,
// so |y2| <= A1 A2 max|x - d| + |C1| |C2| |d| with A_s = sum_k |c_s[k]|, C_s = sum_k c_s[k] over the rounded taps of
// stage s: the window's spread against all the taps, its offset against the chain's response at 0 Hz.  With a, b of
// the tile's whole input window as above the tile is quiet when
//     sqrt(2) / (2 * 2048) * ((A + e) a + (G + e) b) < 0.999 thr,
//     A = A1 A2,  G = |C1| |C2| + 1e-12 S,  e = 1.01 (2 T1 + 1 + 2 T2 + 1) u S,  S = prod_s max(sum_k (|re| + |im|), 1)
// (e: the contract's float chain against the exact one, as tuned_guard_error counts it).  Folded into the two
// weights exactly as tuned_quiet_weights does.
bool tuned_quiet_weights2(const std::vector<std::vector<float>> &re, const std::vector<std::vector<float>> &im, float threshold,
                          uint32_t flags, float &quiet_a, float &quiet_b) {
    if (!(threshold > 0.0f) || !std::isfinite(threshold) || (flags & OOKD_RX_NO_QUIET_SKIP)) return false;
    double A = 1.0, G = 1.0, S = 1.0, T = 0.0;
    for (size_t s = 0; s < re.size(); ++s) {
        double as = 0.0, ss = 0.0, gr = 0.0, gi = 0.0;
        for (size_t k = 0; k < re[s].size(); ++k) {
            as += std::hypot((double)re[s][k], (double)im[s][k]);
            ss += std::fabs((double)re[s][k]) + std::fabs((double)im[s][k]);
            gr += (double)re[s][k];
            gi += (double)im[s][k];
        }
        A *= as;
        G *= std::hypot(gr, gi);
        S *= std::max(ss, 1.0);
        T += 2.0 * (double)re[s].size() + 1.0;
    }
    if (!(A > 0.0)) return false;
    G += 1e-12 * S;                                         // (the double sums' own rounding)
    const double e = 1.01 * T * std::ldexp(1.0, -24) * S;
    const double scale = 1.41421356237309515 / (2.0 * 2048.0) / (0.999 * (double)threshold);
    const double qa = (A + e) * scale, qb = (G + e) * scale;
    if (!(qa < 1e30) || !(qb < 1e30)) return false;
    quiet_a = nextafterf((float)qa, INFINITY);
    quiet_b = nextafterf((float)qb, INFINITY);
    return true;
}

// One carrier at c.nu with c.threshold / c.p_star: its taps appended to pl.ctaps in the device layout (stage s at
// 2 * tap_off, zero padded to ntaps_pad pairs) and, unless the context computes in the contract's order throughout,
// its forward bound, guard band and quiet weights.  -> the quiet test applies to this carrier
bool plan_carrier(FrontPlan &pl, const ookd_filter &filter, uint32_t flags, CarrierPlan &c) {
    const FrontParams &fp = pl.fp;
    std::vector<std::vector<float>> re, im;
    c.tap_off = (uint32_t)pl.ctaps.size();
    uint64_t before = 1;
    for (uint32_t s = 0; s < fp.num_stages; ++s) {
        const std::vector<float> &h = filter.stages[s].taps;
        re.emplace_back(h.size());
        im.emplace_back(h.size());
        tuned_stage_taps(h, c.nu, before, re[s].data(), im[s].data());
        before *= filter.stages[s].decimation;
        // zero padding keeps sums bit-identical, as in plan_filter
        pl.ctaps.resize(c.tap_off + 2 * (size_t)(fp.stage[s].tap_off + fp.stage[s].ntaps_pad), 0.0f);
        for (size_t k = 0; k < h.size(); ++k) {
            pl.ctaps[c.tap_off + 2 * (fp.stage[s].tap_off + k)] = re[s][k];
            pl.ctaps[c.tap_off + 2 * (fp.stage[s].tap_off + k) + 1] = im[s][k];
        }
    }
    if (pl.exact) return false;
    c.err_valu = tuned_guard_error(re, im, 16.0);
    band_from_error(c.err_valu, c.p_star, c.p_lo, c.p_hi);
    // (the shapes front_uses_tuned_fir1 and, where asked for, front_uses_tuned_fir2 take: the tuned kernels with a
    //  quiet test)
    if (fp.tuned_fir2 && tuned_fir2_shape(fp.stage, fp.num_stages)) {
        return tuned_quiet_weights2(re, im, c.threshold, flags, c.quiet_a, c.quiet_b);
    }
    return fp.num_stages == 1 && fp.stage[0].decim == 1 && fp.stage[0].ntaps_pad <= 256u &&
           tuned_quiet_weights(re[0], im[0], c.threshold, flags, c.quiet_a, c.quiet_b);
}

}  // namespace

bool plan_front(uint32_t flags, float threshold, const ookd_filter *filter, double nu, const ookd_rx_carrier *carriers,
                uint32_t num_carriers, FrontPlan &pl) {
    pl = FrontPlan{};
    FrontParams &fp = pl.fp;
    if (!(std::fabs(nu) <= 0.5)) {
        set_error("ookd_rx_create_tuned: nu must be within [-0.5, 0.5] cycles per sample");
        return false;
    }
    if (nu != 0.0 && !filter) {
        set_error("ookd_rx_create_tuned: nu != 0 needs a filter: without one the slicer sees |x|, which does not depend on nu");
        return false;
    }
    if (num_carriers && !filter) {
        set_error("ookd_rx_create_carriers needs a filter: without one the slicer sees |x|, which does not depend on nu");
        return false;
    }
    if ((flags & OOKD_RX_SAMPLES_CS8) && (flags & OOKD_RX_SAMPLES_CU8)) {
        set_error("ookd_rx_create: OOKD_RX_SAMPLES_CS8 and OOKD_RX_SAMPLES_CU8 are both set: a context has one sample format");
        return false;
    }
    pl.exact = (flags & OOKD_RX_EXACT_FIR) != 0;
    fp.mfma_xcd = 2u;           // (what every context passes; only the matrix-core launchers read it: plan_mfma)
    fp.sample_fmt = (flags & OOKD_RX_SAMPLES_CS8) ? kFmtCs8 : (flags & OOKD_RX_SAMPLES_CU8) ? kFmtCu8 : kFmtSc16;
    if (filter && !plan_filter(pl, *filter)) return false;
    fp.p_star = power_threshold(threshold);
    fp.p_lo = fp.p_hi = fp.p_star;
    // A tuned context is one carrier, a carrier context K of them (fir_tuned.hip): each with the packed-FMA kernel's
    // guard band and quiet test in place of the real-tap ones; a carrier context also gets the fused kernel's table.
    const uint32_t K = num_carriers ? num_carriers : nu != 0.0 ? 1u : 0u;
    // (OOKD_RX_TUNED_FIR2 says something to a tuned or carrier context only; the shape: front_uses_tuned_fir2)
    fp.tuned_fir2 = (K && filter && (flags & OOKD_RX_TUNED_FIR2)) ? 1u : 0u;
    for (uint32_t k = 0; k < K; ++k) {
        CarrierPlan c;
        c.nu = num_carriers ? carriers[k].nu : nu;
        if (c.nu == 0.0) c.nu = 0.0;        // (-0)
        c.threshold = num_carriers ? carriers[k].threshold : threshold;
        c.p_star = c.p_lo = c.p_hi = power_threshold(c.threshold);
        // (a carrier without a quiet test keeps its infinite weights: never quiet)
        if (plan_carrier(pl, *filter, flags, c)) fp.quiet_lsb = 1;      // "the shortcut applies": the kernels test with the weights
        if (num_carriers) pl.carrier_tab.push_back({c.tap_off, c.p_star, c.p_lo, c.p_hi, c.quiet_a, c.quiet_b, {0u, 0u}});
        pl.carriers.push_back(c);
    }
    if (K) {
        // the template carries carrier 0's: the tuned kernel reads them there (its weights only when it has a test);
        // the fused kernel reads the table, the generic one's per-carrier launches are handed their carrier's p_star
        fp.p_lo = pl.carriers[0].p_lo;
        fp.p_hi = pl.carriers[0].p_hi;
        fp.p_star = pl.carriers[0].p_star;
        if (!num_carriers && fp.quiet_lsb) fp.quiet_a = pl.carriers[0].quiet_a, fp.quiet_b = pl.carriers[0].quiet_b;
    } else if (filter) {
        if (!pl.exact) pl.mfma_use = plan_real_form(pl, *filter, flags);
        if (pl.mfma_use != MfmaUse::kTaken) pl.mfma.image.clear();
        plan_quiet_skip(pl, *filter, threshold, flags);
    }
    fp.tune = pl.carriers.empty() ? 0u : (pl.exact ? 2u : 1u);

    // The kernel that runs: the launchers' own predicates (launch_front dispatches on them), asked once.  They only
    // test the pointers for null, so for this one call they point at the host images.
    FrontParams probe = fp;
    probe.taps = pl.taps.data();
    probe.mfma_a = pl.mfma.image.empty() ? nullptr : pl.mfma.image.data();
    probe.ctaps = pl.ctaps.empty() ? nullptr : pl.ctaps.data();
    probe.fir_out = (flags & OOKD_RX_KEEP_FIR) ? pl.taps.data() : nullptr;      // (no filter: no sparse form either)
    pl.form = front_form(probe, pl.exact);
    // (a carrier context's fused 1-stage form has its own number; OOKD_FRONT_TUNED_FIR2 runs once per carrier)
    if (pl.carrier_context() && pl.form != OOKD_FRONT_TUNED_FIR2) {
        pl.form = pl.form == OOKD_FRONT_TUNED_FIR1 ? OOKD_FRONT_TUNED_MULTI : OOKD_FRONT_TUNED_GENERIC;
    }
    pl.tile_bits = front_tile_bits(probe);
    pl.sparse_capable = front_sparse_capable(probe);
    // a filter only the generic kernels serve is refused here, not by every run's launch
    if (pl.form == OOKD_FRONT_GENERIC || pl.form == OOKD_FRONT_TUNED_GENERIC) {
        const char *who = num_carriers ? "ookd_rx_create_carriers" : nu != 0.0 ? "ookd_rx_create_tuned" : "ookd_rx_create";
        if (!generic_tile_fits(fp.stage, fp.num_stages, who)) return false;
        pl.gen_tile = generic_tile(fp.stage, fp.num_stages).tile;
    }
    return true;
}

GenTile generic_tile(const FirStageDev *stage, uint32_t num_stages) {
    GenTile g;
    for (uint32_t tile = kGenTile; tile >= (uint32_t)kGenTileMin; tile >>= 1) {
        // (64 bits, and a level of 2^30 samples -- 8 GiB -- stands for anything longer: a deep decimation chain
        //  overflows 32 bits, and 64 without the cap)
        uint64_t len = tile, even = 0, odd = 0;
        for (int s = (int)num_stages - 1; s >= 0; --s) {    // the final level is not stored
            len = std::min<uint64_t>((uint64_t)stage[s].decim * (len - 1) + stage[s].ntaps, 1ull << 30);
            uint64_t &m = (s & 1) ? odd : even;
            if (len > m) m = len;
        }
        g.lds_bytes = (even + odd + 2) * sizeof(float2);    // (of the smallest tile when none fits)
        if (g.lds_bytes <= kGenLdsBytes) {
            g.tile = tile;
            g.lds_b_off = (uint32_t)even + 1;
            return g;
        }
    }
    return g;
}

bool generic_tile_fits(const FirStageDev *stage, uint32_t num_stages, const char *who) {
    const GenTile g = generic_tile(stage, num_stages);
    if (g.tile) return true;
    uint64_t dec = 1;
    bool more = false;          // (the product left 2^31: the text says "at least")
    std::string taps;
    for (uint32_t s = 0; s < num_stages; ++s) {
        if (dec >> 31) more = true;
        else dec *= stage[s].decim;
        taps += (s ? ", " : "") + std::to_string(stage[s].ntaps);
    }
    set_error("%s: a filter of total decimation %s%llu with tap counts [%s] needs %llu bytes of LDS for the generic kernel's "
              "smallest tile of %d outputs; the limit is %zu bytes", who, more ? "at least " : "", (unsigned long long)dec,
              taps.c_str(), (unsigned long long)g.lds_bytes, kGenTileMin, kGenLdsBytes);
    return false;
}

ookd_front_info front_info(const FrontPlan &pl, uint32_t k) {
    ookd_front_info f{};
    f.form = pl.form;
    f.mfma_ksteps = pl.mfma.ksteps;
    f.mfma_c = pl.fp.mfma_c;
    f.err_nominal = pl.err_n;
    f.err_wide = pl.err_w;
    f.mfma_delta = pl.mfma.delta;
    const CarrierPlan *c = pl.carriers.empty() ? nullptr : &pl.carriers[k];
    f.p_star = c ? c->p_star : pl.fp.p_star;
    f.p_lo = c ? c->p_lo : pl.fp.p_lo;
    f.p_hi = c ? c->p_hi : pl.fp.p_hi;
    f.err_valu = c ? c->err_valu : pl.err_valu;
    return f;
}

}  // namespace ookd

using namespace ookd;

extern "C" int ookd_front_plan_digest(uint32_t flags, float threshold, const ookd_filter *filter, double nu,
                                      const ookd_rx_carrier *carriers, uint32_t num_carriers,
                                      ookd_front_plan_digest_out *out) {
    if (!out || num_carriers > OOKD_RX_MAX_CARRIERS || (num_carriers && !carriers)) return OOKD_ERR_ARG;
    FrontPlan pl;
    if (!plan_front(flags, threshold, filter, nu, carriers, num_carriers, pl)) return OOKD_ERR_ARG;
    ookd_front_plan_digest_out d{};
    d.num_records = std::max<uint32_t>(1u, (uint32_t)pl.carriers.size());
    d.form = pl.form;
    d.tile_bits = pl.tile_bits;
    d.sparse_capable = pl.sparse_capable ? 1u : 0u;
    d.mfma_g = pl.fp.mfma_g;
    d.mfma_xcd = pl.fp.mfma_xcd;
    d.quiet_lsb = pl.fp.quiet_lsb;
    d.mfma_use = (uint32_t)pl.mfma_use;
    d.gen_tile = pl.gen_tile;
    const float bands[4] = {pl.fp.p_lo_n, pl.fp.p_hi_n, pl.fp.p_lo_w, pl.fp.p_hi_w};
    memcpy(d.band_bits, bands, sizeof(bands));
    auto fnv = [](const auto &v) { return fnv1a(kFnvBasis, v.data(), v.size() * sizeof(v[0])); };
    d.image_fnv[0] = fnv(pl.taps);
    d.image_fnv[1] = fnv(pl.mfma.image);
    d.image_fnv[2] = fnv(pl.ctaps);
    d.image_fnv[3] = fnv(pl.carrier_tab);
    for (uint32_t k = 0; k < d.num_records; ++k) {
        d.info[k] = front_info(pl, k);
        // (an untuned context has no weights: the template's zeros)
        const float q[2] = {pl.carriers.empty() ? pl.fp.quiet_a : pl.carriers[k].quiet_a,
                            pl.carriers.empty() ? pl.fp.quiet_b : pl.carriers[k].quiet_b};
        memcpy(d.quiet_bits[k], q, sizeof(q));
    }
    *out = d;
    return OOKD_OK;
}
