// survey.cpp -- envelope survey: the C ABI around survey.hip's histogram kernel, and the host-only half --
// the bin rule and the threshold suggestion (include/ookiedokie_amd.h states both as a contract).
#include <cmath>
#include <cstring>
#include <memory>

#include "common.hpp"
#include "kernels.hpp"

using namespace ookd;

static_assert(OOKD_LEVEL_BINS == kLevelBins, "OOKD_LEVEL_BINS");

struct ookd_survey {
    int dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t fmt = kFmtSc16;
    uint32_t max_captures = 1;
    uint32_t total_decim = 1;
    SurveyParams params{};          // stages, taps, tile geometry
    size_t lds_bytes = 0;
    float *d_taps = nullptr;
    unsigned long long *d_hist = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    float kernel_ms = 0.0f;
    uint32_t num_captures = 0;      // of the last run
    uint64_t samples = 0;           // floor(n / D) of the last run
    std::vector<uint64_t> hist;     // [num_captures][kLevelBins]

    ~ookd_survey() {
        (void)hipSetDevice(dev);
        if (d_taps) (void)hipFree(d_taps);
        if (d_hist) (void)hipFree(d_hist);
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
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

ookd_survey *ookd_survey_create(int32_t hip_device, const ookd_filter *filter, uint32_t sample_flags,
                                uint32_t max_captures, void *stream) {
    clear_error();
    const uint32_t both = OOKD_RX_SAMPLES_CS8 | OOKD_RX_SAMPLES_CU8;
    if ((sample_flags & ~both) || (sample_flags & both) == both) {
        set_error("ookd_survey_create: sample_flags must be 0, OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8");
        return nullptr;
    }
    if (max_captures == 0 || max_captures > 65535u) {
        set_error("ookd_survey_create: max_captures must be 1 .. 65535");
        return nullptr;
    }
    if (filter && (filter->stages.empty() || filter->stages.size() > (size_t)kMaxStages)) {
        set_error("ookd_survey_create: filters of 1 .. %d stages are supported", kMaxStages);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || hip_device < 0 || hip_device >= ndev) {
        set_error("no HIP device %d available: libookiedokie_amd has no CPU fallback", hip_device);
        return nullptr;
    }
    std::unique_ptr<ookd_survey> s(new ookd_survey());
    s->dev = hip_device;
    s->max_captures = max_captures;
    s->fmt = (sample_flags & OOKD_RX_SAMPLES_CS8) ? kFmtCs8 : (sample_flags & OOKD_RX_SAMPLES_CU8) ? kFmtCu8 : kFmtSc16;
    (void)hipSetDevice(hip_device);
    std::vector<float> taps;
    SurveyParams &p = s->params;
    p.sample_fmt = s->fmt;
    if (filter) {
        p.num_stages = (uint32_t)filter->stages.size();
        s->total_decim = filter->total_decimation;
        for (uint32_t i = 0; i < p.num_stages; ++i) {
            const auto &st = filter->stages[i];
            if (st.taps.empty() || st.decimation == 0) {
                set_error("ookd_survey_create: stage %u has no taps or no decimation", i);
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
    if (!survey_tile(p, &s->lds_bytes)) {
        set_error("ookd_survey_create: the filter's history does not fit the kernel's LDS window");
        return nullptr;
    }
    if (stream) {
        s->stream = static_cast<hipStream_t>(stream);
    } else {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("ookd_survey_create: hipStreamCreate failed: %s", hipGetErrorString(hipGetLastError()));
            return nullptr;
        }
        s->own_stream = true;
    }
    const size_t tap_bytes = (taps.empty() ? 1 : taps.size()) * sizeof(float);
    if (hipMalloc(reinterpret_cast<void **>(&s->d_taps), tap_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_hist),
                  (size_t)max_captures * kLevelBins * sizeof(unsigned long long)) != hipSuccess ||
        (!taps.empty() &&
         hipMemcpy(s->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) ||
        hipEventCreate(&s->t0) != hipSuccess || hipEventCreate(&s->t1) != hipSuccess) {
        set_error("ookd_survey_create: device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    p.taps = s->d_taps;
    p.hist = s->d_hist;
    return s.release();
}

void ookd_survey_destroy(ookd_survey *s) { delete s; }

int ookd_survey_device(ookd_survey *s, const void *d_iq, uint32_t num_captures, uint64_t samples_per_capture,
                       uint64_t capture_stride_samples) {
    clear_error();
    if (!s || num_captures == 0 || num_captures > s->max_captures || (!d_iq && samples_per_capture) ||
        (num_captures > 1 && capture_stride_samples < samples_per_capture)) {
        set_error("ookd_survey_device: bad argument (captures %u of at most %u, %llu samples, stride %llu)",
                  num_captures, s ? s->max_captures : 0, (unsigned long long)samples_per_capture,
                  (unsigned long long)capture_stride_samples);
        return OOKD_ERR_ARG;
    }
    if (samples_per_capture >> 48) {
        set_error("ookd_survey_device: captures of 2^48 samples and more are not supported");
        return OOKD_ERR_ARG;
    }
    (void)hipSetDevice(s->dev);
    SurveyParams p = s->params;
    p.iq = d_iq;
    p.cap_stride = capture_stride_samples;
    p.n_out = samples_per_capture / s->total_decim;
    p.num_tiles = (p.n_out + p.tile - 1) / p.tile;
    const size_t hist_bytes = (size_t)num_captures * kLevelBins * sizeof(unsigned long long);
    s->hist.assign((size_t)num_captures * kLevelBins, 0);
    s->num_captures = 0;
    s->kernel_ms = 0.0f;
    bool ok = hipMemsetAsync(s->d_hist, 0, hist_bytes, s->stream) == hipSuccess;
    ok = ok && hipEventRecord(s->t0, s->stream) == hipSuccess;
    ok = ok && launch_survey(p, num_captures, s->lds_bytes, s->stream) == hipSuccess;
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
    s->samples = p.n_out;
    return OOKD_OK;
}

int ookd_survey_host(ookd_survey *s, const void *iq, uint64_t num_samples) {
    clear_error();
    if (!s || (!iq && num_samples)) {
        set_error("ookd_survey_host: bad argument");
        return OOKD_ERR_ARG;
    }
    (void)hipSetDevice(s->dev);
    void *d_iq = nullptr;
    const size_t bytes = (size_t)num_samples * sample_bytes(s->fmt);
    if (bytes) {
        if (hipMalloc(&d_iq, bytes) != hipSuccess) {
            set_error("ookd_survey_host: cannot allocate %zu bytes of device memory", bytes);
            return OOKD_ERR_NOMEM;
        }
        if (hipMemcpy(d_iq, iq, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            set_error("ookd_survey_host: HIP failure: %s", hipGetErrorString(hipGetLastError()));
            (void)hipFree(d_iq);
            return OOKD_ERR_HIP;
        }
    }
    const int rc = ookd_survey_device(s, d_iq, 1, num_samples, num_samples);
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
    memcpy(out->bins, s->hist.data() + (size_t)capture * kLevelBins, sizeof out->bins);
    return OOKD_OK;
}

float ookd_survey_kernel_ms(const ookd_survey *s) { return s ? s->kernel_ms : 0.0f; }

}  // extern "C"
