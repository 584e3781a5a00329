// survey.cpp -- envelope survey: the C ABI around survey.hip's histogram kernel, and the host-only half --
// the bin rule and the threshold suggestion (include/ookiedokie_amd.h states both as a contract).
#include <cmath>
#include <cstring>
#include <memory>

#include "scan_ctx.hpp"

using namespace ookd;

static_assert(OOKD_LEVEL_BINS == kLevelBins, "OOKD_LEVEL_BINS");

struct ookd_survey : ScanCtx {
    uint32_t total_decim = 1;
    SurveyParams params{};          // stages, taps, tile geometry
    size_t lds_bytes = 0;
    float *d_taps = nullptr;
    // tuned survey (ookd_survey_create_tuned with nu != 0): the form its runs take, the complex taps as (re, im)
    // pairs, and the register-blocked form's shape
    uint32_t form = OOKD_SURVEY_GENERIC;
    double tune_nu = 0.0;
    float *d_ctaps = nullptr;
    uint32_t fir1_R = kSurveyFir1R, fir1_waves = kSurveyFir1Waves;
    bool fir2_thin = true;          // OOKD_SURVEY_TUNED_MULTI_FIR2 at strides 32, 64: stage 0 thinned
    unsigned long long *d_hist = nullptr;
    uint32_t num_captures = 0;      // of the last run
    uint64_t samples = 0;           // floor(n / D) of the last run
    std::vector<uint64_t> hist;     // [num_captures][kLevelBins]; a carriers survey: [num_captures][K][kLevelBins]
    // carriers survey (ookd_survey_create_carriers): K > 0, the stride, every carrier's nu, and -- where the shape
    // has no OOKD_SURVEY_TUNED_MULTI form -- one tuned survey per carrier on this context's stream
    uint32_t num_carriers = 0, stride = 1;
    std::vector<std::unique_ptr<ookd_survey>> singles;

    ~ookd_survey() {
        if (dev < 0) return;
        (void)hipSetDevice(dev);
        if (d_taps) (void)hipFree(d_taps);
        if (d_ctaps) (void)hipFree(d_ctaps);
        if (d_hist) (void)hipFree(d_hist);
    }
};

// ---- the suggestion's exact arithmetic -----------------------------------------------------------------------
// Otsu's criterion compares d^2 / (a b) between splits, d up to 2^136 for 2^64 samples: cross-multiplied,
// d1^2 a2 b2 against d2^2 a1 b1, in unsigned integers of 16 x 32 bits.
namespace {

struct Wide {
    static constexpr int N = 16;
    uint32_t w[N] = {};
    Wide() = default;
    explicit Wide(unsigned __int128 v) {
        for (int i = 0; i < 4; ++i) w[i] = (uint32_t)(v >> (32 * i));
    }
    Wide operator*(const Wide &o) const {       // operands here never overflow 512 bits
        Wide r;
        for (int i = 0; i < N; ++i) {
            if (!w[i]) continue;
            uint64_t carry = 0;
            for (int j = 0; i + j < N; ++j) {
                const uint64_t t = (uint64_t)w[i] * o.w[j] + r.w[i + j] + carry;
                r.w[i + j] = (uint32_t)t;
                carry = t >> 32;
            }
        }
        return r;
    }
    int compare(const Wide &o) const {
        for (int i = N - 1; i >= 0; --i)
            if (w[i] != o.w[i]) return w[i] < o.w[i] ? -1 : 1;
        return 0;
    }
};

struct Split {
    Wide d2;            // (n s0 - a S)^2
    Wide ab;            // a (n - a)
};

uint32_t median_bin(const uint64_t *h, uint32_t lo, uint32_t hi, unsigned __int128 count) {
    const unsigned __int128 half = (count + 1) / 2;
    unsigned __int128 c = 0;
    for (uint32_t b = lo; b < hi; ++b) {
        c += h[b];
        if (c >= half) return b;
    }
    return hi - 1;
}

float bin_amplitude(uint32_t bin) {
    if (bin == 0) return 0.0f;
    const double lo = (double)ookd_level_bin_lower(bin), hi = (double)ookd_level_bin_lower(bin + 1);
    return (float)std::sqrt(std::sqrt(lo * hi));
}

}  // namespace

extern "C" {

uint32_t ookd_level_bin(float power) {
    uint32_t bits;
    memcpy(&bits, &power, sizeof bits);
    return level_bin_of_bits(bits);
}

float ookd_level_bin_lower(uint32_t bin) {
    if (bin == 0) return 0.0f;
    const uint64_t e = (uint64_t)bin + kLevelBinBase;
    if (e >= (255ull << 2)) return INFINITY;
    const uint32_t bits = (uint32_t)e << 21;
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
}

int ookd_suggest_threshold(const ookd_level_hist *h, ookd_threshold_suggestion *out) {
    clear_error();
    if (!h || !out) {
        set_error("ookd_suggest_threshold: NULL argument");
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    const uint64_t *bins = h->bins;
    unsigned __int128 n = 0, S = 0;
    uint32_t first = kLevelBins, lastb = 0;
    for (uint32_t b = 0; b < (uint32_t)kLevelBins; ++b) {
        n += bins[b];
        S += (unsigned __int128)bins[b] * b;
        if (bins[b]) {
            if (first == (uint32_t)kLevelBins) first = b;
            lastb = b;
        }
    }
    if (n == 0) return OOKD_OK;
    if (first == lastb) {               // one level: no split
        out->off_bin = out->on_bin = out->split_bin = first;
        return OOKD_OK;
    }
    bool have = false;
    Split best;
    uint32_t k_first = 0, k_last = 0;
    unsigned __int128 a = 0, s0 = 0;
    for (uint32_t k = 0; k + 1 < (uint32_t)kLevelBins; ++k) {
        a += bins[k];
        s0 += (unsigned __int128)bins[k] * k;
        if (a == 0 || a == n) continue;
        // d = n s0 - a S <= 0 (the lower side's mean is the smaller one): take |d| = a S - n s0
        const Wide aS = Wide(a) * Wide(S), ns0 = Wide(n) * Wide(s0);
        Wide d;
        {                               // d = aS - ns0
            int64_t borrow = 0;
            for (int i = 0; i < Wide::N; ++i) {
                const int64_t t = (int64_t)aS.w[i] - (int64_t)ns0.w[i] - borrow;
                d.w[i] = (uint32_t)t;
                borrow = t < 0 ? 1 : 0;
            }
        }
        Split cur;
        cur.d2 = d * d;
        cur.ab = Wide(a) * Wide(n - a);
        const int c = have ? (cur.d2 * best.ab).compare(best.d2 * cur.ab) : 1;
        if (c > 0) {
            best = cur;
            have = true;
            k_first = k_last = k;
        } else if (c == 0) {
            k_last = k;
        }
    }
    const uint32_t k = (k_first + k_last) / 2;
    unsigned __int128 n_off = 0;
    for (uint32_t b = 0; b <= k; ++b) n_off += bins[b];
    const unsigned __int128 n_on = n - n_off;
    out->split_bin = k;
    out->off_bin = median_bin(bins, 0, k + 1, n_off);
    out->on_bin = median_bin(bins, k + 1, kLevelBins, n_on);
    out->off_level = bin_amplitude(out->off_bin);
    out->on_level = bin_amplitude(out->on_bin);
    out->on_fraction = (double)n_on / (double)n;
    if (out->on_bin - out->off_bin >= OOKD_LEVEL_MIN_SEPARATION && n_off >= OOKD_LEVEL_MIN_SIDE &&
        n_on >= OOKD_LEVEL_MIN_SIDE) {
        out->found = 1;
        out->threshold = (out->off_level + out->on_level) / 2.0f;
    }
    return OOKD_OK;
}

// One implementation behind both entry points; `who` names the caller in the messages.  nu == 0 is the untuned
// survey whatever `exact` says.
static ookd_survey *survey_create(const char *who, int32_t hip_device, const ookd_filter *filter,
                                  uint32_t sample_flags, uint32_t max_captures, void *stream, double nu, bool exact) {
    if (!scan_ctx_check_create(who, sample_flags, max_captures)) return nullptr;
    if (filter && (filter->stages.empty() || filter->stages.size() > (size_t)kMaxStages)) {
        set_error("%s: filters of 1 .. %d stages are supported", who, kMaxStages);
        return nullptr;
    }
    std::unique_ptr<ookd_survey> s(new ookd_survey());
    if (!scan_ctx_open(*s, who, hip_device, sample_flags, max_captures, stream)) return nullptr;
    s->tune_nu = nu != 0.0 ? nu : 0.0;
    std::vector<float> taps;
    SurveyParams &p = s->params;
    p.sample_fmt = s->fmt;
    if (filter) {
        p.num_stages = (uint32_t)filter->stages.size();
        s->total_decim = filter->total_decimation;
        for (uint32_t i = 0; i < p.num_stages; ++i) {
            const auto &st = filter->stages[i];
            if (st.taps.empty() || st.decimation == 0) {
                set_error("%s: stage %u has no taps or no decimation", who, i);
                return nullptr;
            }
            FirStageDev d{};
            d.decim = st.decimation;
            d.ntaps = d.ntaps_pad = (uint32_t)st.taps.size();
            d.tap_off = (uint32_t)taps.size();
            taps.insert(taps.end(), st.taps.begin(), st.taps.end());
            p.stage[i] = d;
        }
    }
    std::vector<float> ctaps;           // tuned: (re, im) pairs, stage s at 2 * tap_off
    if (nu != 0.0) {
        const bool fir1 = !exact && p.num_stages == 1 && p.stage[0].decim == 1 && p.stage[0].ntaps <= 256u;
        s->form = fir1 ? OOKD_SURVEY_TUNED_FIR1 : OOKD_SURVEY_TUNED_GENERIC;
        const size_t pad = (taps.size() + kTunedChunk - 1) / kTunedChunk * kTunedChunk;
        ctaps.assign(2 * pad, 0.0f);
        uint64_t before = 1;
        for (uint32_t i = 0; i < p.num_stages; ++i) {
            const auto &h = filter->stages[i].taps;
            std::vector<float> re(h.size()), im(h.size());
            tuned_stage_taps(h, nu, before, re.data(), im.data());
            for (size_t k = 0; k < h.size(); ++k) {
                ctaps[2 * (p.stage[i].tap_off + k)] = re[k];
                ctaps[2 * (p.stage[i].tap_off + k) + 1] = im[k];
            }
            before *= filter->stages[i].decimation;
        }
        if (fir1) {
            // the measured shape; OOKD_SURVEY_TUNED_SHAPE=<R>x<waves> is the experiment hook the
            // rate tool sweeps with
            if (const char *e = dev_getenv("OOKD_SURVEY_TUNED_SHAPE")) {
                unsigned R = 0, w = 0;
                if (sscanf(e, "%ux%u", &R, &w) != 2 || !survey_tuned_fir1_shape(R, w)) {
                    set_error("%s: OOKD_SURVEY_TUNED_SHAPE must be 8x1 .. 16x4, not '%s'", who, e);
                    return nullptr;
                }
                s->fir1_R = R;
                s->fir1_waves = w;
            }
            p.stage[0].ntaps_pad = (uint32_t)pad;
            p.tile = 64u * s->fir1_R;
        }
    }
    if (s->form != OOKD_SURVEY_TUNED_FIR1 &&
        !survey_tile(p, &s->lds_bytes, s->form == OOKD_SURVEY_TUNED_GENERIC ? 2u : 1u)) {
        set_error("%s: the filter's history does not fit the kernel's LDS window", who);
        return nullptr;
    }
    const size_t tap_bytes = (taps.empty() ? 1 : taps.size()) * sizeof(float);
    if (hipMalloc(reinterpret_cast<void **>(&s->d_taps), tap_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_hist),
                  (size_t)max_captures * kLevelBins * sizeof(unsigned long long)) != hipSuccess ||
        (!taps.empty() &&
         hipMemcpy(s->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) ||
        (!ctaps.empty() &&
         (hipMalloc(reinterpret_cast<void **>(&s->d_ctaps), ctaps.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(s->d_ctaps, ctaps.data(), ctaps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    p.taps = s->d_taps;
    p.hist = s->d_hist;
    return s.release();
}

ookd_survey *ookd_survey_create(int32_t hip_device, const ookd_filter *filter, uint32_t sample_flags,
                                uint32_t max_captures, void *stream) {
    clear_error();
    return survey_create("ookd_survey_create", hip_device, filter, sample_flags, max_captures, stream, 0.0, false);
}

ookd_survey *ookd_survey_create_tuned(int32_t hip_device, const ookd_filter *filter, uint32_t flags,
                                      uint32_t max_captures, void *stream, const ookd_tune *tune) {
    clear_error();
    const uint32_t both = OOKD_RX_SAMPLES_CS8 | OOKD_RX_SAMPLES_CU8;
    if ((flags & ~(both | OOKD_RX_EXACT_FIR)) || (flags & both) == both) {
        set_error("ookd_survey_create_tuned: flags must be 0, OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8, with or "
                  "without OOKD_RX_EXACT_FIR");
        return nullptr;
    }
    const double nu = tune ? tune->nu : 0.0;
    if (!(std::fabs(nu) <= 0.5)) {
        set_error("ookd_survey_create_tuned: nu must be within [-0.5, 0.5] cycles per sample");
        return nullptr;
    }
    if (tune && (tune->reserved[0] | tune->reserved[1] | tune->reserved[2])) {
        set_error("ookd_survey_create_tuned: ookd_tune.reserved must be zero");
        return nullptr;
    }
    if (nu != 0.0 && !filter) {
        set_error("ookd_survey_create_tuned: nu != 0 needs a filter: without one the power is |x|^2, which does not "
                  "depend on nu");
        return nullptr;
    }
    return survey_create("ookd_survey_create_tuned", hip_device, filter, flags & both, max_captures, stream, nu,
                         (flags & OOKD_RX_EXACT_FIR) != 0);
}

// The rest of ookd_survey_create_carriers for OOKD_SURVEY_TUNED_MULTI_FIR2 (survey_carriers_fir2.hip): both stages'
// complex taps per carrier, zero padded to 16 and 32 pairs.
static bool survey_carriers_fir2(const char *who, std::unique_ptr<ookd_survey> &s, const ookd_filter *filter,
                                 const ookd_tune *tunes) {
    s->form = OOKD_SURVEY_TUNED_MULTI_FIR2;
    SurveyParams &p = s->params;
    p.sample_fmt = s->fmt;
    p.num_stages = 2;
    const uint32_t pad[2] = {16u, 32u};
    for (uint32_t i = 0; i < 2; ++i) {
        p.stage[i].decim = 2;
        p.stage[i].ntaps = (uint32_t)filter->stages[i].taps.size();
        p.stage[i].ntaps_pad = pad[i];
        p.stage[i].tap_off = i ? pad[0] : 0u;
        p.num_taps += p.stage[i].ntaps;
    }
    p.tile = kSurveyFir2Tile;
    // the measured choice; OOKD_SURVEY_FIR2_THIN=0 is the experiment hook the rate tool compares with
    if (const char *e = dev_getenv("OOKD_SURVEY_FIR2_THIN")) s->fir2_thin = atoi(e) != 0;
    const uint32_t K = s->num_carriers;
    std::vector<float> ctaps((size_t)K * kSurveyFir2TapFloats, 0.0f);
    for (uint32_t k = 0; k < K; ++k) {
        uint64_t before = 1;
        for (uint32_t i = 0; i < 2; ++i) {
            const std::vector<float> &h = filter->stages[i].taps;
            std::vector<float> re(h.size()), im(h.size());
            tuned_stage_taps(h, tunes[k].nu, before, re.data(), im.data());
            float *dst = ctaps.data() + (size_t)kSurveyFir2TapFloats * k + 2 * p.stage[i].tap_off;
            for (size_t t = 0; t < h.size(); ++t) {
                dst[2 * t] = re[t];
                dst[2 * t + 1] = im[t];
            }
            before *= filter->stages[i].decimation;
        }
    }
    if (hipMalloc(reinterpret_cast<void **>(&s->d_hist),
                  (size_t)s->max_captures * K * kLevelBins * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_ctaps), ctaps.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(s->d_ctaps, ctaps.data(), ctaps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return false;
    }
    p.hist = s->d_hist;
    return true;
}

ookd_survey *ookd_survey_create_carriers(int32_t hip_device, const ookd_filter *filter, uint32_t flags,
                                         uint32_t max_captures, void *stream, const ookd_tune *tunes,
                                         uint32_t num_carriers, uint32_t stride) {
    static const char who[] = "ookd_survey_create_carriers";
    static_assert(OOKD_SURVEY_MAX_CARRIERS == kSurveyMaxCarriers && OOKD_SURVEY_MAX_STRIDE == kSurveyMaxStride,
                  "OOKD_SURVEY_MAX_*");
    clear_error();
    const uint32_t both = OOKD_RX_SAMPLES_CS8 | OOKD_RX_SAMPLES_CU8;
    if ((flags & ~(both | OOKD_RX_EXACT_FIR | OOKD_RX_TUNED_FIR2)) || (flags & both) == both) {
        set_error("%s: flags must be 0, OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8, with or without OOKD_RX_EXACT_FIR "
                  "and OOKD_RX_TUNED_FIR2", who);
        return nullptr;
    }
    if (num_carriers == 0 || num_carriers > OOKD_SURVEY_MAX_CARRIERS) {
        set_error("%s: num_carriers must be 1 .. %d, not %u", who, OOKD_SURVEY_MAX_CARRIERS, num_carriers);
        return nullptr;
    }
    if (!tunes) {
        set_error("%s: tunes is NULL", who);
        return nullptr;
    }
    for (uint32_t k = 0; k < num_carriers; ++k) {
        if (!(std::fabs(tunes[k].nu) <= 0.5)) {
            set_error("%s: carrier %u: nu must be within [-0.5, 0.5] cycles per sample", who, k);
            return nullptr;
        }
        if (tunes[k].reserved[0] | tunes[k].reserved[1] | tunes[k].reserved[2]) {
            set_error("%s: carrier %u: ookd_tune.reserved must be zero", who, k);
            return nullptr;
        }
    }
    if (!filter) {
        set_error("%s: a carriers survey needs a filter: without one the power is |x|^2 for every carrier", who);
        return nullptr;
    }
    if (stride == 0 || stride > OOKD_SURVEY_MAX_STRIDE || (stride & (stride - 1u))) {
        set_error("%s: stride must be a power of two in 1 .. %d, not %u", who, OOKD_SURVEY_MAX_STRIDE, stride);
        return nullptr;
    }
    if (!scan_ctx_check_create(who, flags & both, max_captures)) return nullptr;
    if (filter->stages.empty() || filter->stages.size() > (size_t)kMaxStages) {
        set_error("%s: filters of 1 .. %d stages are supported", who, kMaxStages);
        return nullptr;
    }
    for (size_t i = 0; i < filter->stages.size(); ++i)
        if (filter->stages[i].taps.empty() || filter->stages[i].decimation == 0) {
            set_error("%s: stage %zu has no taps or no decimation", who, i);
            return nullptr;
        }
    const bool exact = (flags & OOKD_RX_EXACT_FIR) != 0;
    const bool multi = !exact && filter->stages.size() == 1 && filter->stages[0].decimation == 1 &&
                       filter->stages[0].taps.size() <= 256u;
    // OOKD_RX_TUNED_FIR2 asks for the fused two-stage form where the shape has one (the front end's shape test); on
    // every other shape and beside OOKD_RX_EXACT_FIR it has no effect, as on an rx context
    bool fir2 = false;
    if ((flags & OOKD_RX_TUNED_FIR2) && !exact && filter->stages.size() == 2) {
        FirStageDev st[2] = {};
        for (int i = 0; i < 2; ++i) {
            st[i].decim = filter->stages[i].decimation;
            st[i].ntaps = filter->stages[i].taps.size() > 0xffffu ? 0xffffu : (uint32_t)filter->stages[i].taps.size();
        }
        fir2 = tuned_fir2_shape(st, 2);
    }
    if (!multi && !fir2 && stride != 1) {
        set_error("%s: stride %u needs the OOKD_SURVEY_TUNED_MULTI form: 1 stage, decimation 1, at most 256 taps, no "
                  "OOKD_RX_EXACT_FIR; every other survey counts every output (stride 1)", who, stride);
        return nullptr;
    }
    std::unique_ptr<ookd_survey> s(new ookd_survey());
    if (!scan_ctx_open(*s, who, hip_device, flags & both, max_captures, stream)) return nullptr;
    s->num_carriers = num_carriers;
    s->stride = stride;
    s->tune_nu = tunes[0].nu != 0.0 ? tunes[0].nu : 0.0;
    s->total_decim = filter->total_decimation;
    if (fir2) return survey_carriers_fir2(who, s, filter, tunes) ? s.release() : nullptr;
    if (!multi) {
        // the tuned contract's generic form, carrier by carrier (nu = 0: the untuned survey, the same counts)
        s->form = OOKD_SURVEY_TUNED_GENERIC;
        for (uint32_t k = 0; k < num_carriers; ++k) {
            ookd_survey *one = survey_create(who, hip_device, filter, flags & both, max_captures, s->stream,
                                             tunes[k].nu, true);
            if (!one) return nullptr;
            s->singles.emplace_back(one);
        }
        return s.release();
    }
    s->form = OOKD_SURVEY_TUNED_MULTI;
    const std::vector<float> &h = filter->stages[0].taps;
    const size_t pad = (h.size() + kTunedChunk - 1) / kTunedChunk * kTunedChunk;
    SurveyParams &p = s->params;
    p.sample_fmt = s->fmt;
    p.num_stages = 1;
    p.stage[0].decim = 1;
    p.stage[0].ntaps = (uint32_t)h.size();
    p.stage[0].ntaps_pad = (uint32_t)pad;
    p.stage[0].tap_off = 0;
    // the measured shape per stride; OOKD_SURVEY_MULTI_R=<8|16|32|64> is the experiment hook the rate
    // tool compares the two with
    uint32_t R = survey_multi_R(stride);
    if (const char *e = dev_getenv("OOKD_SURVEY_MULTI_R")) {
        R = (uint32_t)strtoul(e, nullptr, 10);
        if (!survey_multi_shape(R, stride)) {
            set_error("%s: OOKD_SURVEY_MULTI_R must be 8 or 16, or 32 or 64 up to the stride, not '%s'", who, e);
            return nullptr;
        }
    }
    p.tile = 64u * R;
    p.num_taps = (uint32_t)h.size();
    std::vector<float> ctaps((size_t)num_carriers * 2 * pad, 0.0f);     // carrier k's pairs at 2 * pad * k
    std::vector<float> re(h.size()), im(h.size());
    for (uint32_t k = 0; k < num_carriers; ++k) {
        tuned_stage_taps(h, tunes[k].nu, 1, re.data(), im.data());
        for (size_t t = 0; t < h.size(); ++t) {
            ctaps[2 * (pad * k + t)] = re[t];
            ctaps[2 * (pad * k + t) + 1] = im[t];
        }
    }
    if (hipMalloc(reinterpret_cast<void **>(&s->d_hist),
                  (size_t)max_captures * num_carriers * kLevelBins * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_ctaps), ctaps.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(s->d_ctaps, ctaps.data(), ctaps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    p.hist = s->d_hist;
    return s.release();
}

double ookd_survey_tune(const ookd_survey *s) { return s ? s->tune_nu : 0.0; }

uint32_t ookd_survey_form(const ookd_survey *s) { return s ? s->form : 0u; }

void ookd_survey_destroy(ookd_survey *s) { delete s; }

// A carriers survey without the multi form: the tuned survey of every carrier in turn, on the one stream.
static int survey_singles_device(ookd_survey *s, const void *d_iq, uint32_t num_captures, uint64_t samples_per_capture,
                                 uint64_t capture_stride_samples) {
    const uint32_t K = s->num_carriers;
    s->hist.assign((size_t)num_captures * K * kLevelBins, 0);
    s->num_captures = 0;
    s->kernel_ms = 0.0f;
    for (uint32_t k = 0; k < K; ++k) {
        ookd_survey *one = s->singles[k].get();
        const int rc = ookd_survey_device(one, d_iq, num_captures, samples_per_capture, capture_stride_samples);
        if (rc != OOKD_OK) return rc;
        for (uint32_t c = 0; c < num_captures; ++c)
            memcpy(s->hist.data() + ((size_t)c * K + k) * kLevelBins, one->hist.data() + (size_t)c * kLevelBins,
                   kLevelBins * sizeof(uint64_t));
        s->kernel_ms += one->kernel_ms;
        s->samples = one->samples;
    }
    s->num_captures = num_captures;
    return OOKD_OK;
}

int ookd_survey_device(ookd_survey *s, const void *d_iq, uint32_t num_captures, uint64_t samples_per_capture,
                       uint64_t capture_stride_samples) {
    clear_error();
    const int rc = scan_ctx_check_run(s, "ookd_survey_device", d_iq, num_captures, samples_per_capture,
                                      capture_stride_samples, false);
    if (rc != OOKD_OK) return rc;
    if (!s->singles.empty())
        return survey_singles_device(s, d_iq, num_captures, samples_per_capture, capture_stride_samples);
    (void)hipSetDevice(s->dev);
    SurveyParams p = s->params;
    p.iq = d_iq;
    p.cap_stride = capture_stride_samples;
    p.n_out = samples_per_capture / s->total_decim;
    p.num_tiles = (p.n_out + p.tile - 1) / p.tile;
    const size_t per_capture = (size_t)(s->num_carriers ? s->num_carriers : 1u) * kLevelBins;
    const size_t hist_bytes = (size_t)num_captures * per_capture * sizeof(unsigned long long);
    s->hist.assign((size_t)num_captures * per_capture, 0);
    s->num_captures = 0;
    s->kernel_ms = 0.0f;
    bool ok = hipMemsetAsync(s->d_hist, 0, hist_bytes, s->stream) == hipSuccess;
    ok = ok && hipEventRecord(s->t0, s->stream) == hipSuccess;
    if (s->form == OOKD_SURVEY_TUNED_MULTI_FIR2)
        ok = ok && launch_survey_tuned_multi_fir2(p, s->d_ctaps, num_captures, s->num_carriers, s->stride,
                                                  samples_per_capture, s->fir2_thin, s->stream) == hipSuccess;
    else if (s->form == OOKD_SURVEY_TUNED_MULTI)
        ok = ok && launch_survey_tuned_multi(p, s->d_ctaps, num_captures, s->num_carriers, s->stride, s->stream) == hipSuccess;
    else if (s->form == OOKD_SURVEY_TUNED_FIR1)
        ok = ok && launch_survey_tuned_fir1(p, s->d_ctaps, num_captures, s->fir1_R, s->fir1_waves, s->stream) == hipSuccess;
    else        // (d_ctaps is null unless the form is OOKD_SURVEY_TUNED_GENERIC)
        ok = ok && launch_survey(p, s->d_ctaps, num_captures, s->lds_bytes, s->stream) == hipSuccess;
    ok = ok && hipEventRecord(s->t1, s->stream) == hipSuccess;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram word");
    ok = ok && hipMemcpyAsync(s->hist.data(), s->d_hist, hist_bytes, hipMemcpyDeviceToHost, s->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) {
        set_error("ookd_survey_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    if (p.num_tiles) (void)hipEventElapsedTime(&s->kernel_ms, s->t0, s->t1);
    s->num_captures = num_captures;
    s->samples = (p.n_out + s->stride - 1) / s->stride;     // (stride is 1 but for a carriers survey)
    return OOKD_OK;
}

int ookd_survey_host(ookd_survey *s, const void *iq, uint64_t num_samples) {
    clear_error();
    void *d_iq = nullptr;               // this run's alone: freed again below
    size_t capacity = 0;
    int rc = scan_ctx_stage(s, "ookd_survey_host", iq, num_samples, &d_iq, &capacity);
    if (rc == OOKD_OK) rc = ookd_survey_device(s, d_iq, 1, num_samples, num_samples);
    if (d_iq) (void)hipFree(d_iq);
    return rc;
}

int ookd_survey_get_hist(const ookd_survey *s, uint32_t capture, ookd_level_hist *out) {
    clear_error();
    if (!s || !out || capture >= s->num_captures) {
        set_error("ookd_survey_get_hist: bad argument (capture %u of %u)", capture, s ? s->num_captures : 0);
        return OOKD_ERR_ARG;
    }
    out->samples = s->samples;
    // (a carriers survey: carrier 0)
    memcpy(out->bins, s->hist.data() + (size_t)capture * (s->num_carriers ? s->num_carriers : 1u) * kLevelBins,
           sizeof out->bins);
    return OOKD_OK;
}

int ookd_survey_get_carrier_hist(const ookd_survey *s, uint32_t capture, uint32_t carrier, ookd_level_hist *out) {
    clear_error();
    if (!s || !out || !s->num_carriers || capture >= s->num_captures || carrier >= s->num_carriers) {
        set_error("ookd_survey_get_carrier_hist: bad argument (capture %u of %u, carrier %u of %u)", capture,
                  s ? s->num_captures : 0, carrier, s ? s->num_carriers : 0);
        return OOKD_ERR_ARG;
    }
    out->samples = s->samples;
    memcpy(out->bins, s->hist.data() + ((size_t)capture * s->num_carriers + carrier) * kLevelBins, sizeof out->bins);
    return OOKD_OK;
}

uint32_t ookd_survey_num_carriers(const ookd_survey *s) { return s ? s->num_carriers : 0u; }

uint32_t ookd_survey_stride(const ookd_survey *s) { return s ? s->stride : 0u; }

float ookd_survey_kernel_ms(const ookd_survey *s) { return s ? s->kernel_ms : 0.0f; }

}  // extern "C"
