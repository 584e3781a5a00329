// run_levels.cpp -- pulse levels: the C ABI around run_levels.hip's sparse pass, and the host-only half -- the level
// of a message from the peaks of its pulses (include/ookiedokie_amd.h states both as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "clean.hpp"
#include "front_plan.hpp"
#include "run_levels.hpp"

using namespace ookd;

namespace ookd {

struct RunLevelCtx : EdgePass {
    // the filter as the pass's kernel reads it, made by the first call that launches (constant for the context)
    bool built = false;
    SurveyParams sv{};
    size_t lds_bytes = 0;
    float *d_taps = nullptr, *d_ctaps = nullptr;
    uint32_t ctap_floats = 0;
    // the results of run `serial`: [captures][kRunLevelWords], then the peaks as uint32 patterns
    std::vector<uint64_t> host;
    uint32_t captures = 0;
    uint64_t n_out = 0, peak_slots = 0;

    ~RunLevelCtx() override {
        if (d_taps) (void)hipFree(d_taps);
        if (d_ctaps) (void)hipFree(d_ctaps);
    }
    const uint32_t *peak_words() const { return reinterpret_cast<const uint32_t *>(host.data() + (size_t)captures * kRunLevelWords); }
};

}  // namespace ookd

namespace {

// The context's filter in the survey's layout (unpadded taps, stage after stage); a tuned or carrier context: every
// carrier's complex taps, carrier after carrier.
int build_filter(const char *who, RunLevelCtx &ctx, const EdgeRun &run, const RunLevelSource &src) {
    const FrontPlan &plan = *src.plan;
    const FrontParams &fp = plan.fp;
    SurveyParams p{};
    p.sample_fmt = fp.sample_fmt;
    p.num_stages = fp.num_stages;
    std::vector<float> taps;
    for (uint32_t s = 0; s < fp.num_stages && s < (uint32_t)kMaxStages; ++s) {
        FirStageDev d{};
        d.decim = fp.stage[s].decim;
        d.ntaps = d.ntaps_pad = fp.stage[s].ntaps;
        d.tap_off = (uint32_t)taps.size();
        taps.insert(taps.end(), plan.taps.begin() + fp.stage[s].tap_off, plan.taps.begin() + fp.stage[s].tap_off + fp.stage[s].ntaps);
        p.stage[s] = d;
    }
    const bool tuned = !plan.carriers.empty() && fp.num_stages != 0;
    std::vector<float> ctaps;
    if (tuned) {
        for (const CarrierPlan &c : plan.carriers) {
            for (uint32_t s = 0; s < fp.num_stages; ++s) {
                const float *from = plan.ctaps.data() + c.tap_off + 2 * (size_t)fp.stage[s].tap_off;
                ctaps.insert(ctaps.end(), from, from + 2 * (size_t)fp.stage[s].ntaps);
            }
        }
    }
    if (!survey_tile(p, &ctx.lds_bytes, tuned ? 2u : 1u)) {
        set_error("%s: the filter's history does not fit the kernel's LDS window", who);
        return OOKD_ERR_ARG;
    }
    if (hipSetDevice(run.dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    if ((!taps.empty() &&
         (hipMalloc(reinterpret_cast<void **>(&ctx.d_taps), taps.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(ctx.d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) ||
        (!ctaps.empty() &&
         (hipMalloc(reinterpret_cast<void **>(&ctx.d_ctaps), ctaps.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(ctx.d_ctaps, ctaps.data(), ctaps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        if (ctx.d_taps) (void)hipFree(ctx.d_taps);
        if (ctx.d_ctaps) (void)hipFree(ctx.d_ctaps);
        ctx.d_taps = ctx.d_ctaps = nullptr;
        return OOKD_ERR_NOMEM;
    }
    p.taps = ctx.d_taps;
    ctx.ctap_floats = plan.carrier_context() ? 2u * p.num_taps : 0u;
    ctx.sv = p;
    ctx.built = true;
    return OOKD_OK;
}

// The pass behind every entry point: `ctx` has answered the context's last run when this returns OOKD_OK.
// clean = false: the run's own edge list (pass kEdgePassLevels); true: the cleaned list (kEdgePassCleanLevels).
int levels_pass(const char *who, bool clean, ookd_rx *rx, uint32_t capture, RunLevelCtx *&ctx) {
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    if (clean && !clean_run_view(rx, run)) {
        set_error("%s: no cleaned list of the last run (ookd_rx_clean_edges first)", who);
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, clean ? kEdgePassCleanLevels : kEdgePassLevels);
    if (!slot) slot.reset(new (std::nothrow) RunLevelCtx());
    ctx = static_cast<RunLevelCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial == run.serial) return OOKD_OK;
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    if (!ctx->built) {                  // (before anything of the last answer goes: a refused filter changes nothing)
        if (const int rc = build_filter(who, *ctx, run, src); rc != OOKD_OK) return rc;
    }
    ctx->serial = 0;
    ctx->captures = run.captures;
    ctx->n_out = run.n_out;
    ctx->peak_slots = run_peak_slots(run.num_edges, run.captures);
    const size_t words = (size_t)run.captures * kRunLevelWords + (size_t)((ctx->peak_slots + 1u) / 2u);
    ctx->host.assign(words, 0);
    if (run.n_out == 0) {               // no buffer was processed: nothing was written for the kernel to read
        ctx->serial = run.serial;
        ctx->kernel_ms = 0.0f;
        return OOKD_OK;
    }
    RunLevelParams p{};
    p.list = edge_list_view(run);
    p.sv = ctx->sv;
    p.sv.iq = src.iq;
    p.sv.cap_stride = src.stride;
    p.sv.n_out = run.n_out;
    p.sv.num_tiles = (run.n_out + p.sv.tile - 1) / p.sv.tile;
    p.n_valid = src.n_valid;
    p.one_source = src.plan->carrier_context() ? 1u : 0u;
    p.ctap_floats = ctx->ctap_floats;
    p.ctaps = ctx->d_ctaps;
    p.peak_slots = ctx->peak_slots;
    const size_t lds_bytes = ctx->lds_bytes;
    const size_t peak_word = (size_t)run.captures * kRunLevelWords;
    return ctx->run(who, run, words, ctx->host.data(), [&](unsigned long long *d) {
        p.result = d;
        p.peaks = reinterpret_cast<uint32_t *>(d + peak_word);
        return launch_run_levels(p, lds_bytes, run.stream);
    });
}

// capture's E, and its peaks inside ctx->host (null when it has none)
const uint32_t *peaks_of(const RunLevelCtx &ctx, uint32_t capture, uint64_t &runs) {
    const uint64_t *r = ctx.host.data() + (size_t)capture * kRunLevelWords + kRunLevelMetaWord;
    runs = (r[0] + 1u) / 2u;
    const uint64_t base = run_peak_base(r[2], capture);
    if (base + runs > ctx.peak_slots) runs = base < ctx.peak_slots ? ctx.peak_slots - base : 0;
    return ctx.peak_words() + base;
}

int run_levels(const char *who, bool clean, ookd_rx *rx, uint32_t capture, ookd_run_levels *out) {
    clear_error();
    if (!rx || !out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    RunLevelCtx *ctx = nullptr;
    if (const int rc = levels_pass(who, clean, rx, capture, ctx); rc != OOKD_OK) return rc;
    memset(out, 0, sizeof *out);
    const uint64_t *r = ctx->host.data() + (size_t)capture * kRunLevelWords;
    uint64_t runs = 0;
    (void)peaks_of(*ctx, capture, runs);
    out->num_runs = runs;
    out->tile_outputs = ctx->sv.tile;
    out->tiles_total = (ctx->n_out + ctx->sv.tile - 1) / ctx->sv.tile;
    out->tiles_filtered = r[kRunLevelMetaWord + 1];
    out->hist.samples = runs;
    memcpy(out->hist.bins, r, sizeof out->hist.bins);
    return OOKD_OK;
}

int run_peaks(const char *who, bool clean, ookd_rx *rx, uint32_t capture, float *peaks, uint64_t capacity, uint64_t *num_runs) {
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    RunLevelCtx *ctx = nullptr;
    if (const int rc = levels_pass(who, clean, rx, capture, ctx); rc != OOKD_OK) return rc;
    uint64_t runs = 0;
    const uint32_t *from = peaks_of(*ctx, capture, runs);
    if (num_runs) *num_runs = runs;
    const uint64_t take = std::min<uint64_t>(runs, capacity);
    if (peaks && take) memcpy(peaks, from, take * sizeof(float));
    return OOKD_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ookd_run_levels) == 32 + sizeof(ookd_level_hist), "ookd_run_levels layout");
static_assert(sizeof(((ookd_level_hist *)nullptr)->bins) == kLevelBins * sizeof(uint64_t), "histogram words");

int ookd_rx_run_levels(ookd_rx *rx, uint32_t capture, ookd_run_levels *out) {
    return run_levels("ookd_rx_run_levels", false, rx, capture, out);
}

int ookd_rx_run_levels_clean(ookd_rx *rx, uint32_t capture, ookd_run_levels *out) {
    return run_levels("ookd_rx_run_levels_clean", true, rx, capture, out);
}

int ookd_rx_get_run_peaks(ookd_rx *rx, uint32_t capture, float *peaks, uint64_t capacity, uint64_t *num_runs) {
    return run_peaks("ookd_rx_get_run_peaks", false, rx, capture, peaks, capacity, num_runs);
}

int ookd_rx_get_run_peaks_clean(ookd_rx *rx, uint32_t capture, float *peaks, uint64_t capacity, uint64_t *num_runs) {
    return run_peaks("ookd_rx_get_run_peaks_clean", true, rx, capture, peaks, capacity, num_runs);
}

float ookd_rx_levels_kernel_ms(const ookd_rx *rx) { return edge_pass_kernel_ms(rx, kEdgePassLevels); }

int ookd_message_levels(const uint64_t *edges, uint64_t E, const float *peaks, uint64_t R, const uint64_t *msg_samples,
                        uint64_t M, uint32_t pulses, float *levels) {
    clear_error();
    if ((E && !edges) || (R && !peaks) || (M && (!msg_samples || !levels))) {
        set_error("ookd_message_levels: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (R != (E + 1u) / 2u) {
        set_error("ookd_message_levels: %llu peaks for %llu edges (ceil(E / 2) on-runs)", (unsigned long long)R, (unsigned long long)E);
        return OOKD_ERR_ARG;
    }
    if (pulses == 0) {
        set_error("ookd_message_levels: pulses must be at least 1");
        return OOKD_ERR_ARG;
    }
    for (uint64_t m = 1; m < M; ++m) {
        if (msg_samples[m] < msg_samples[m - 1]) {
            set_error("ookd_message_levels: msg_samples must ascend (message %llu)", (unsigned long long)m);
            return OOKD_ERR_ARG;
        }
    }
    std::vector<float> sel;
    uint64_t r = 0;                     // the first on-run no earlier message took
    for (uint64_t m = 0; m < M; ++m) {
        uint64_t end = r;               // on-runs [r, end) rise at or below msg_samples[m]
        while (end < R && edges[2 * end] <= msg_samples[m]) ++end;
        const uint64_t count = std::min<uint64_t>(end - r, pulses);
        levels[m] = 0.0f;
        if (count) {
            sel.assign(peaks + (end - count), peaks + end);
            std::nth_element(sel.begin(), sel.begin() + (count - 1) / 2, sel.end());
            levels[m] = sel[(count - 1) / 2];
        }
        r = end;
    }
    return OOKD_OK;
}

}  // extern "C"
