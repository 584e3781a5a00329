// burst_spectra.cpp -- burst spectra: the C ABI around burst_spectra.hip's kernels, the span rule, and the host-only
// rule ookd_suggest_burst_carriers (include/ookiedokie_amd.h states all three as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "burst_spectra.hpp"
#include "edge_pass.hpp"
#include "front_plan.hpp"
#include "run_levels.hpp"

using namespace ookd;

static_assert(sizeof(ookd_burst_spectrum) == sizeof(BurstSpecSummary), "the device summary is ookd_burst_spectrum");
static_assert(OOKD_BURST_SPECTRA_MIN_SPAN == kBurstSpecMinSpan && OOKD_BURST_SPECTRA_MAX_ROWS == kBurstSpecMaxRows, "the span rule");

namespace ookd {

struct BurstSpectraCtx : EdgePass {
    float2 *d_twiddle = nullptr;        // spectrum_tables(), made by the first call that launches
    float *d_window = nullptr;
    double *d_rows = nullptr;           // [rows][1024] (grown, never shrunk)
    uint64_t rows = 0;
    double *d_keyed_rows = nullptr;     // [keyed_spans][1024]
    uint64_t keyed_spans = 0;
    hipEvent_t mid = nullptr;           // between the first kernel and the rest
    uint64_t asked = 0;                 // orders the raw and the clean form's context, as BurstCtx::asked
    // of run `serial`, per capture
    struct Capture {
        bool valid = false;
        uint64_t made = 0;              // BurstTableRef::made of the table that was read
        uint32_t span = 0, flags = 0;
        uint64_t spans = 0, total = 0, total_frames = 0;
        float reduce_ms = 0.0f;
        std::vector<ookd_burst_spectrum> summary;
        std::vector<double> keyed;      // [1024]
    };
    std::vector<Capture> caps;
    std::vector<uint64_t> host;         // the result words of the last pass

    ~BurstSpectraCtx() override {
        if (d_twiddle) (void)hipFree(d_twiddle);
        if (d_window) (void)hipFree(d_window);
        if (d_rows) (void)hipFree(d_rows);
        if (d_keyed_rows) (void)hipFree(d_keyed_rows);
        if (mid) (void)hipEventDestroy(mid);
    }
};

}  // namespace ookd

namespace {

uint64_t g_asked = 0;

// the span rule: see ookd_burst_spectra_span
int span_rule(const char *who, uint64_t total, uint32_t span, uint32_t *used) {
    if (span != 0 && (span < kBurstSpecMinSpan || (span & (span - 1u)) != 0)) {
        set_error("%s: span_frames %u is neither 0 nor a power of two of at least %u", who, span, kBurstSpecMinSpan);
        return OOKD_ERR_ARG;
    }
    uint32_t fit = kBurstSpecMinSpan;
    while (2u * burst_spec_spans(total, fit) > kBurstSpecMaxRows) {
        if (fit >= 0x80000000u) {
            set_error("%s: a cut of %llu samples fits no span", who, (unsigned long long)total);
            return OOKD_ERR_CAPACITY;
        }
        fit *= 2u;
    }
    if (span != 0 && span < fit) {
        set_error("%s: span_frames %u needs %llu partial rows for a cut of %llu samples, the workspace holds %llu: the "
                  "smallest span that fits is %u", who, span, (unsigned long long)(2u * burst_spec_spans(total, span)),
                  (unsigned long long)total, (unsigned long long)kBurstSpecMaxRows, fit);
        return OOKD_ERR_CAPACITY;
    }
    *used = span ? span : fit;
    return OOKD_OK;
}

template <typename T>
bool grow(T *&p, uint64_t want) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(reinterpret_cast<void **>(&p), (size_t)want * sizeof(T)) == hipSuccess;
}

// tables, events and the rows of `spans` spans
int reserve(BurstSpectraCtx &c, const char *who, int dev, uint64_t spans) {
    if (hipSetDevice(dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    bool ok = true;
    if (!c.d_twiddle) {
        std::vector<float2> tw(kSpecBins);
        std::vector<float> win(kSpecBins);
        spectrum_tables(tw.data(), win.data());
        ok = grow(c.d_twiddle, kSpecBins) && grow(c.d_window, kSpecBins) &&
             hipMemcpy(c.d_twiddle, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(c.d_window, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            if (c.d_twiddle) (void)hipFree(c.d_twiddle);
            if (c.d_window) (void)hipFree(c.d_window);
            c.d_twiddle = nullptr;
            c.d_window = nullptr;
        }
    }
    if (ok && c.rows < 2u * spans) {
        c.rows = 0;
        ok = grow(c.d_rows, 2u * spans * kSpecBins);
        if (ok) c.rows = 2u * spans;
    }
    if (ok && c.keyed_spans < spans) {
        c.keyed_spans = 0;
        ok = grow(c.d_keyed_rows, spans * kSpecBins);
        if (ok) c.keyed_spans = spans;
    }
    if (!ok) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    if (!c.mid && hipEventCreate(&c.mid) != hipSuccess) {
        set_error("%s: hipEventCreate failed", who);
        return OOKD_ERR_HIP;
    }
    return OOKD_OK;
}

EdgePassId pass_of(const BurstTableRef &t) { return t.clean ? kEdgePassCleanBurstSpectra : kEdgePassBurstSpectra; }

// what both launches read of the run: false + error when the capture is not at hand
bool fill_source(const char *who, const ookd_rx *rx, const EdgeRun &run, uint32_t capture, const BurstTableRef &t,
                 BurstSpectraParams &p) {
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    if (!src.iq || !t.d_table || hipSetDevice(run.dev) != hipSuccess) {
        set_error("%s: the run's capture is not at hand", who);
        return false;
    }
    const uint32_t fmt = src.plan->fp.sample_fmt;
    const uint32_t from = src.plan->carrier_context() ? 0u : capture;      // every carrier's list cuts the one capture
    p.table = t.d_table;
    p.num_bursts = t.num_bursts;
    p.total = t.total;
    p.src = static_cast<const char *>(src.iq) + (size_t)from * src.stride * sample_bytes(fmt);
    p.n = src.n_valid;
    p.sample_fmt = fmt;
    return true;
}

// The result of `capture` about the table the copy calls are about, or null + error.
const BurstSpectraCtx::Capture *result_of(const char *who, const ookd_rx *rx, uint32_t capture, BurstSpectraCtx **ctx_out = nullptr,
                                          EdgeRun *run_out = nullptr, BurstTableRef *table_out = nullptr) {
    EdgeRun run;
    BurstTableRef t;
    if (!burst_table_ref(who, rx, capture, run, t)) return nullptr;
    BurstSpectraCtx *c = static_cast<BurstSpectraCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), pass_of(t)).get());
    if (!c || c->serial != run.serial || capture >= c->caps.size() || !c->caps[capture].valid || c->caps[capture].made != t.made) {
        set_error("%s: no burst spectra of capture %u's burst table (ookd_rx_burst_spectra first)", who, capture);
        return nullptr;
    }
    if (ctx_out) *ctx_out = c;
    if (run_out) *run_out = run;
    if (table_out) *table_out = t;
    return &c->caps[capture];
}

}  // namespace

extern "C" {

int ookd_burst_spectra_span(uint64_t total_samples, uint32_t span_frames, uint32_t *span_used) {
    clear_error();
    if (!span_used) {
        set_error("ookd_burst_spectra_span: NULL argument");
        return OOKD_ERR_ARG;
    }
    return span_rule("ookd_burst_spectra_span", total_samples, span_frames, span_used);
}

int ookd_rx_burst_spectra(ookd_rx *rx, uint32_t capture, uint32_t span_frames) {
    const char *who = "ookd_rx_burst_spectra";
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    BurstTableRef t;
    if (!burst_table_ref(who, rx, capture, run, t)) return OOKD_ERR_ARG;
    uint32_t span = 0;
    if (const int rc = span_rule(who, t.total, span_frames, &span); rc != OOKD_OK) return rc;
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, pass_of(t));
    if (!slot) slot.reset(new (std::nothrow) BurstSpectraCtx());
    BurstSpectraCtx *ctx = static_cast<BurstSpectraCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial != run.serial) {            // a new run: nothing of the last one holds
        ctx->caps.clear();
        ctx->serial = 0;
        ctx->kernel_ms = 0.0f;
    }
    ctx->caps.resize(run.captures);
    BurstSpectraCtx::Capture &cap = ctx->caps[capture];
    if (ctx->serial == run.serial && cap.valid && cap.made == t.made && cap.span == span) {
        ctx->asked = ++g_asked;
        return OOKD_OK;
    }
    cap = BurstSpectraCtx::Capture();
    const uint64_t spans = t.num_bursts ? burst_spec_spans(t.total, span) : 0;
    std::vector<ookd_burst_spectrum> summary((size_t)t.num_bursts);
    std::vector<double> keyed(kSpecBins, 0.0);
    if (t.num_bursts) memset(summary.data(), 0, summary.size() * sizeof(ookd_burst_spectrum));
    float reduce_ms = 0.0f;
    if (spans != 0) {
        if (const int rc = reserve(*ctx, who, run.dev, spans); rc != OOKD_OK) return rc;
        BurstSpectraParams p{};
        if (!fill_source(who, rx, run, capture, t, p)) return OOKD_ERR_HIP;
        p.span_frames = span;
        p.spans = spans;
        p.only = kBurstSpecAll;
        p.twiddle = ctx->d_twiddle;
        p.window = ctx->d_window;
        p.rows = ctx->d_rows;
        p.keyed_rows = ctx->d_keyed_rows;
        const size_t sum_words = (size_t)t.num_bursts * (sizeof(BurstSpecSummary) / 8u);
        ctx->host.assign(sum_words + kSpecBins, 0);
        const int rc = ctx->run(who, run, ctx->host.size(), ctx->host.data(), [&](unsigned long long *d) {
            p.summary = reinterpret_cast<BurstSpecSummary *>(d);
            p.keyed = reinterpret_cast<double *>(d + sum_words);
            p.one = nullptr;
            return launch_burst_spectra(p, ctx->mid, run.stream);
        });
        if (rc != OOKD_OK) {
            ctx->caps.clear();                  // (run() has forgotten the run: so do the captures)
            return rc;
        }
        if (hipEventElapsedTime(&reduce_ms, ctx->mid, ctx->t1) != hipSuccess) reduce_ms = 0.0f;
        memcpy(summary.data(), ctx->host.data(), sum_words * 8u);
        memcpy(keyed.data(), ctx->host.data() + sum_words, kSpecBins * sizeof(double));
    } else {
        ctx->kernel_ms = 0.0f;
    }
    ctx->serial = run.serial;
    cap.valid = true;
    cap.made = t.made;
    cap.span = span;
    cap.flags = t.clean ? (uint32_t)OOKD_BURSTS_CLEAN : 0u;
    cap.spans = spans;
    cap.total = t.total;
    cap.reduce_ms = reduce_ms;
    for (const ookd_burst_spectrum &s : summary) cap.total_frames += s.frames;
    cap.summary.swap(summary);
    cap.keyed.swap(keyed);
    ctx->asked = ++g_asked;
    return OOKD_OK;
}

int ookd_rx_get_burst_spectra(const ookd_rx *rx, uint32_t capture, ookd_burst_spectrum *out, uint64_t capacity,
                              uint64_t *num_bursts) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_get_burst_spectra: NULL argument");
        return OOKD_ERR_ARG;
    }
    const BurstSpectraCtx::Capture *c = result_of("ookd_rx_get_burst_spectra", rx, capture);
    if (!c) return OOKD_ERR_ARG;
    if (num_bursts) *num_bursts = c->summary.size();
    const uint64_t take = out ? std::min<uint64_t>(c->summary.size(), capacity) : 0;
    if (take) memcpy(out, c->summary.data(), (size_t)take * sizeof(ookd_burst_spectrum));
    return OOKD_OK;
}

int ookd_rx_get_keyed_spectrum(const ookd_rx *rx, uint32_t capture, ookd_spectrum_result *out) {
    clear_error();
    if (!rx || !out) {
        set_error("ookd_rx_get_keyed_spectrum: NULL argument");
        return OOKD_ERR_ARG;
    }
    const BurstSpectraCtx::Capture *c = result_of("ookd_rx_get_keyed_spectrum", rx, capture);
    if (!c) return OOKD_ERR_ARG;
    out->frames = c->total_frames;
    memcpy(out->power, c->keyed.data(), sizeof out->power);
    return OOKD_OK;
}

int ookd_rx_get_burst_spectra_info(const ookd_rx *rx, uint32_t capture, ookd_burst_spectra_info *out) {
    clear_error();
    if (!rx || !out) {
        set_error("ookd_rx_get_burst_spectra_info: NULL argument");
        return OOKD_ERR_ARG;
    }
    const BurstSpectraCtx::Capture *c = result_of("ookd_rx_get_burst_spectra_info", rx, capture);
    if (!c) return OOKD_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->num_bursts = c->summary.size();
    out->total_frames = c->total_frames;
    out->spans = c->spans;
    out->partial_rows = 2u * c->spans;
    out->span_frames = c->span;
    out->flags = c->flags;
    out->reduce_kernel_ms = c->reduce_ms;
    return OOKD_OK;
}

int ookd_rx_burst_spectrum(ookd_rx *rx, uint32_t capture, uint64_t burst, ookd_spectrum_result *out) {
    const char *who = "ookd_rx_burst_spectrum";
    clear_error();
    if (!rx || !out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    BurstSpectraCtx *ctx = nullptr;
    EdgeRun run;
    BurstTableRef t;
    const BurstSpectraCtx::Capture *c = result_of(who, rx, capture, &ctx, &run, &t);
    if (!c) return OOKD_ERR_ARG;
    if (burst >= c->summary.size() || burst >= t.num_bursts) {
        set_error("%s: burst %llu of %llu", who, (unsigned long long)burst, (unsigned long long)c->summary.size());
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    const uint64_t F = c->summary[burst].frames;
    out->frames = F;
    if (F == 0 || c->spans == 0) return OOKD_OK;
    const BurstDev &e = t.table[burst];
    const uint64_t width = (uint64_t)c->span * kSpecBins;
    const uint64_t g_first = e.offset / width, g_last = (e.offset + (F - 1u) * kSpecBins) / width;
    BurstSpectraParams p{};
    if (!fill_source(who, rx, run, capture, t, p)) return OOKD_ERR_HIP;
    p.span_frames = c->span;
    p.spans = c->spans;
    p.only = burst;
    p.twiddle = ctx->d_twiddle;
    p.window = ctx->d_window;
    p.rows = ctx->d_rows;
    p.keyed_rows = ctx->d_keyed_rows;
    if (g_last >= c->spans || 2u * c->spans > ctx->rows) {
        set_error("%s: the burst table and its spectra do not belong together", who);
        return OOKD_ERR_ARG;
    }
    // (a timed pass of its own on the same buffers: the summaries' time stays what it was)
    const float ms = ctx->kernel_ms;
    std::vector<uint64_t> words(kSpecBins, 0);
    const int rc = ctx->run(who, run, words.size(), words.data(), [&](unsigned long long *d) {
        p.one = reinterpret_cast<double *>(d);
        return launch_burst_spectrum_one(p, g_first, g_last - g_first + 1u, run.stream);
    });
    if (rc != OOKD_OK) {
        ctx->caps.clear();
        return rc;
    }
    ctx->kernel_ms = ms;
    memcpy(out->power, words.data(), sizeof out->power);
    return OOKD_OK;
}

float ookd_rx_burst_spectra_kernel_ms(const ookd_rx *rx) {
    if (!rx) return 0.0f;
    EdgeRun run;
    ookd_rx_edge_run(rx, &run);
    if (run.serial == 0) return 0.0f;
    const BurstSpectraCtx *best = nullptr;
    for (EdgePassId id : {kEdgePassBurstSpectra, kEdgePassCleanBurstSpectra}) {
        const BurstSpectraCtx *c = static_cast<const BurstSpectraCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), id).get());
        if (c && c->serial == run.serial && (!best || c->asked > best->asked)) best = c;
    }
    return best ? best->kernel_ms : 0.0f;
}

int ookd_suggest_burst_carriers(const ookd_burst_spectrum *s, uint64_t num_bursts, double min_share, uint32_t min_spacing_bins,
                                ookd_burst_carrier *out, uint32_t capacity, uint32_t *count, int32_t *carrier_of_burst) {
    clear_error();
    if ((!s && num_bursts) || !count || (!out && capacity)) {
        set_error("ookd_suggest_burst_carriers: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (!(min_share >= 0.0)) {
        set_error("ookd_suggest_burst_carriers: min_share must be 0 (the default) or positive");
        return OOKD_ERR_ARG;
    }
    constexpr uint32_t N = OOKD_SPECTRUM_BINS;
    for (uint64_t b = 0; b < num_bursts; ++b) {
        if (s[b].peak_bin >= N) {
            set_error("ookd_suggest_burst_carriers: burst %llu has peak_bin %u", (unsigned long long)b, s[b].peak_bin);
            return OOKD_ERR_ARG;
        }
    }
    if (min_share == 0.0) min_share = OOKD_BURST_MIN_SHARE;
    if (min_spacing_bins == 0) min_spacing_bins = OOKD_CARRIER_MIN_SPACING;
    *count = 0;
    std::vector<char> qualifies((size_t)num_bursts, 0);
    std::vector<double> weight(N, 0.0);
    for (uint64_t b = 0; b < num_bursts; ++b) {
        if (carrier_of_burst) carrier_of_burst[b] = -1;
        const double rest = s[b].total_power - s[b].dc_power;
        if (s[b].frames >= 1 && rest > 0.0 && s[b].peak_power >= min_share * rest) {
            qualifies[b] = 1;
            weight[s[b].peak_bin] += s[b].peak_power;
        }
    }
    std::vector<char> live(N, 1);
    std::vector<int32_t> owner(N, -1);          // the carrier a bin went to
    while (*count < capacity) {
        int best = -1;
        for (uint32_t k = 0; k < N; ++k)
            if (live[k] && (best < 0 || weight[k] > weight[best])) best = (int)k;
        if (best < 0 || !(weight[best] > 0.0)) break;
        ookd_burst_carrier &c = out[*count];
        memset(&c, 0, sizeof c);
        c.bin = best < (int)(N / 2) ? best : best - (int)N;
        c.nu = ookd_spectrum_bin_nu((uint32_t)best);
        if (min_spacing_bins >= N / 2) {        // every bin is within reach
            for (uint32_t k = 0; k < N; ++k)
                if (live[k]) {
                    owner[k] = (int32_t)*count;
                    live[k] = 0;
                }
        } else {
            for (uint32_t d = 0; d <= min_spacing_bins; ++d) {
                for (uint32_t k : {((uint32_t)best + d) % N, ((uint32_t)best + N - d) % N}) {
                    if (live[k]) {
                        owner[k] = (int32_t)*count;
                        live[k] = 0;
                    }
                }
            }
        }
        ++*count;
    }
    for (uint64_t b = 0; b < num_bursts; ++b) {
        if (!qualifies[b]) continue;
        const int32_t o = owner[s[b].peak_bin];
        if (o < 0) continue;
        if (carrier_of_burst) carrier_of_burst[b] = o;
        out[o].bursts += 1;
        out[o].frames += s[b].frames;
        out[o].power += s[b].peak_power;
    }
    return OOKD_OK;
}

}  // extern "C"
