// spectrum.cpp -- carrier survey: the C ABI around spectrum.hip's Welch spectrum, and the host-only half -- the
// bin-to-nu rule and the carrier suggestion (include/ookiedokie_amd.h states both as a contract).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "scan_ctx.hpp"

using namespace ookd;

static_assert(OOKD_SPECTRUM_BINS == kSpecBins, "OOKD_SPECTRUM_BINS");

struct ookd_spectrum : ScanCtx {
    int cus = 0;
    float2 *d_twiddle = nullptr;
    float *d_window = nullptr;
    double *d_partial = nullptr;
    size_t partial_rows = 0;        // rows of 1024 doubles d_partial holds
    double *d_power = nullptr;      // [max_captures][1024]
    void *d_stage = nullptr;        // ookd_spectrum_host's copy of the capture, kept and grown
    size_t stage_bytes = 0;
    uint32_t num_captures = 0;      // of the last run
    uint64_t frames = 0;            // floor(n / 1024) of the last run
    std::vector<double> power;      // [num_captures][1024]

    ~ookd_spectrum() {
        if (dev < 0) return;
        (void)hipSetDevice(dev);
        if (d_twiddle) (void)hipFree(d_twiddle);
        if (d_window) (void)hipFree(d_window);
        if (d_partial) (void)hipFree(d_partial);
        if (d_power) (void)hipFree(d_power);
        if (d_stage) (void)hipFree(d_stage);
    }
};

namespace ookd {

// the tables, in double, rounded once: the angle is reduced to an exact multiple of 1/1024 turn first
void spectrum_tables(float2 *tw, float *win) {
    const double two_pi = 6.283185307179586476925286766559;
    auto w1024 = [&](int m) {               // e^{-j 2 pi m / 1024}
        const double a = two_pi * (double)(m % kSpecBins) / (double)kSpecBins;
        return make_float2((float)std::cos(a), (float)-std::sin(a));
    };
    for (int m = 0; m < kSpecBins; ++m) win[m] = (float)(0.5 - 0.5 * std::cos(two_pi * (double)m / (double)kSpecBins));
    for (int kj = 1; kj < 4; ++kj)          // the order the lanes read them (kernels.hpp, SpectrumParams::twiddle)
        for (int i = 0; i < 4; ++i)
            for (int L = 0; L < 64; ++L) tw[(kj - 1) * 256 + i * 64 + L] = w1024((4 * L + i) * kj);
    for (int kt = 0; kt < 16; ++kt)
        for (int s = 0; s < 16; ++s) tw[768 + 16 * kt + s] = w1024(4 * s * kt);
}

}  // namespace ookd

extern "C" {

double ookd_spectrum_bin_nu(uint32_t bin) {
    bin &= (uint32_t)(OOKD_SPECTRUM_BINS - 1);
    return (bin < OOKD_SPECTRUM_BINS / 2 ? (double)bin : (double)bin - OOKD_SPECTRUM_BINS) / OOKD_SPECTRUM_BINS;
}

int ookd_suggest_carriers(const ookd_spectrum_result *sp, double min_ratio, uint32_t min_spacing_bins,
                          ookd_carrier *out, uint32_t capacity, uint32_t *count, double *floor) {
    clear_error();
    if (!sp || !count || (!out && capacity)) {
        set_error("ookd_suggest_carriers: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (!(min_ratio >= 0.0)) {
        set_error("ookd_suggest_carriers: min_ratio must be 0 (the default) or positive");
        return OOKD_ERR_ARG;
    }
    if (min_ratio == 0.0) min_ratio = OOKD_CARRIER_MIN_RATIO;
    if (min_spacing_bins == 0) min_spacing_bins = OOKD_CARRIER_MIN_SPACING;
    *count = 0;
    constexpr uint32_t N = OOKD_SPECTRUM_BINS;
    std::vector<double> sorted(sp->power, sp->power + N);
    std::sort(sorted.begin(), sorted.end());
    const double fl = (sorted[N / 2 - 1] + sorted[N / 2]) / 2.0;
    if (floor) *floor = fl;
    if (sp->frames == 0) return OOKD_OK;
    bool live[N];
    for (uint32_t k = 0; k < N; ++k) live[k] = true;
    while (*count < capacity) {
        int best = -1;
        for (uint32_t k = 0; k < N; ++k)
            if (live[k] && (best < 0 || sp->power[k] > sp->power[best])) best = (int)k;
        if (best < 0) break;
        const double pk = sp->power[best];
        if (!(pk > 0.0) || pk < min_ratio * fl) break;
        ookd_carrier &c = out[(*count)++];
        c.bin = best < (int)(N / 2) ? best : best - (int)N;
        c.nu = ookd_spectrum_bin_nu((uint32_t)best);
        c.at_dc = (c.bin >= -1 && c.bin <= 1) ? 1u : 0u;
        c.power = pk;
        c.ratio = pk / fl;
        if (min_spacing_bins >= N / 2) break;       // every bin is within reach
        for (uint32_t d = 0; d <= min_spacing_bins; ++d) {
            live[((uint32_t)best + d) % N] = false;
            live[((uint32_t)best + N - d) % N] = false;
        }
    }
    return OOKD_OK;
}

ookd_spectrum *ookd_spectrum_create(int32_t hip_device, uint32_t sample_flags, uint32_t max_captures, void *stream) {
    clear_error();
    const char *who = "ookd_spectrum_create";
    if (!scan_ctx_check_create(who, sample_flags, max_captures)) return nullptr;
    std::unique_ptr<ookd_spectrum> s(new ookd_spectrum());
    if (!scan_ctx_open(*s, who, hip_device, sample_flags, max_captures, stream)) return nullptr;
    if (hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess || s->cus < 1) {
        set_error("ookd_spectrum_create: cannot read the device's CU count");
        return nullptr;
    }
    std::vector<float2> tw(kSpecBins);
    std::vector<float> win(kSpecBins);
    spectrum_tables(tw.data(), win.data());
    if (hipMalloc(reinterpret_cast<void **>(&s->d_twiddle), tw.size() * sizeof(float2)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_window), win.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->d_power), (size_t)max_captures * kSpecBins * sizeof(double)) !=
            hipSuccess ||
        hipMemcpy(s->d_twiddle, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->d_window, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("ookd_spectrum_create: device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return s.release();
}

void ookd_spectrum_destroy(ookd_spectrum *s) { delete s; }

int ookd_spectrum_device(ookd_spectrum *s, const void *d_iq, uint32_t num_captures, uint64_t samples_per_capture,
                         uint64_t capture_stride_samples) {
    clear_error();
    const int rc = scan_ctx_check_run(s, "ookd_spectrum_device", d_iq, num_captures, samples_per_capture,
                                      capture_stride_samples, true);
    if (rc != OOKD_OK) return rc;
    const uint32_t sb = sample_bytes(s->fmt);
    (void)hipSetDevice(s->dev);
    SpectrumParams p{};
    p.iq = d_iq;
    p.sample_fmt = s->fmt;
    p.cap_stride = capture_stride_samples;
    p.frames = samples_per_capture / kSpecBins;
    p.aligned = ((uintptr_t)d_iq % 16 == 0 && (num_captures == 1 || (capture_stride_samples * sb) % 16 == 0)) ? 1u : 0u;
    p.twiddle = s->d_twiddle;
    p.window = s->d_window;
    p.power = s->d_power;
    const uint32_t groups = spectrum_groups(p.frames, num_captures, s->cus);
    const size_t rows = (size_t)groups * num_captures;
    s->power.assign((size_t)num_captures * kSpecBins, 0.0);
    s->num_captures = 0;
    s->kernel_ms = 0.0f;
    if (rows > s->partial_rows) {
        if (s->d_partial) (void)hipFree(s->d_partial);
        s->d_partial = nullptr;
        s->partial_rows = 0;
        if (hipMalloc(reinterpret_cast<void **>(&s->d_partial), rows * kSpecBins * sizeof(double)) != hipSuccess) {
            set_error("ookd_spectrum_device: cannot allocate %zu rows of partial sums", rows);
            return OOKD_ERR_NOMEM;
        }
        s->partial_rows = rows;
    }
    p.partial = s->d_partial;
    if (groups) {
        const size_t bytes = (size_t)num_captures * kSpecBins * sizeof(double);
        bool ok = hipEventRecord(s->t0, s->stream) == hipSuccess;
        ok = ok && launch_spectrum(p, num_captures, groups, s->stream) == hipSuccess;
        ok = ok && hipEventRecord(s->t1, s->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(s->power.data(), s->d_power, bytes, hipMemcpyDeviceToHost, s->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
        if (!ok) {
            set_error("ookd_spectrum_device: HIP failure: %s", hipGetErrorString(hipGetLastError()));
            return OOKD_ERR_HIP;
        }
        (void)hipEventElapsedTime(&s->kernel_ms, s->t0, s->t1);
    }
    s->num_captures = num_captures;
    s->frames = p.frames;
    return OOKD_OK;
}

int ookd_spectrum_host(ookd_spectrum *s, const void *iq, uint64_t num_samples) {
    clear_error();
    // the staging buffer stays with the context and only grows
    const int rc = scan_ctx_stage(s, "ookd_spectrum_host", iq, num_samples, s ? &s->d_stage : nullptr,
                                  s ? &s->stage_bytes : nullptr);
    if (rc != OOKD_OK) return rc;
    return ookd_spectrum_device(s, num_samples ? s->d_stage : nullptr, 1, num_samples, num_samples);
}

int ookd_spectrum_get(const ookd_spectrum *s, uint32_t capture, ookd_spectrum_result *out) {
    clear_error();
    if (!s || !out || capture >= s->num_captures) {
        set_error("ookd_spectrum_get: bad argument (capture %u of %u)", capture, s ? s->num_captures : 0);
        return OOKD_ERR_ARG;
    }
    out->frames = s->frames;
    memcpy(out->power, s->power.data() + (size_t)capture * kSpecBins, sizeof out->power);
    return OOKD_OK;
}

float ookd_spectrum_kernel_ms(const ookd_spectrum *s) { return s ? s->kernel_ms : 0.0f; }

}  // extern "C"
