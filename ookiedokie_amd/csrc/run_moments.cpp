// run_moments.cpp -- pulse moments: the C ABI around run_moments.hip's sparse pass, the contract on the host given the
// filter's output (ookd_run_moments_of), and the host-only half -- mean power, carrier and coherence of a message from
// the sums of its pulses (include/ookiedokie_amd.h states all three as a contract).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "clean.hpp"
#include "front_plan.hpp"
#include "run_moments.hpp"

#pragma clang fp contract(off)

using namespace ookd;

namespace ookd {

struct RunMomentCtx : EdgePass {
    // the filter as the pass's kernel reads it, made by the first call that launches (constant for the context)
    bool built = false;
    SurveyParams sv{};
    size_t lds_bytes = 0;
    float *d_taps = nullptr, *d_ctaps = nullptr;
    uint32_t ctap_floats = 0, table_segs = kRunMomentTableSegs, decimation = 1;
    // the results of run `serial`: [captures][kRunMomentWords], then three sums per slot
    std::vector<uint64_t> host;
    uint32_t captures = 0;
    uint64_t n_out = 0, slots = 0;

    ~RunMomentCtx() override {
        if (d_taps) (void)hipFree(d_taps);
        if (d_ctaps) (void)hipFree(d_ctaps);
    }
};

}  // namespace ookd

namespace {

// The context's filter in the survey's layout, as run_levels.cpp builds it, with the LDS geometry of survey_tile_lag.
int build_filter(const char *who, RunMomentCtx &ctx, const EdgeRun &run, const RunLevelSource &src) {
    const FrontPlan &plan = *src.plan;
    const FrontParams &fp = plan.fp;
    SurveyParams p{};
    p.sample_fmt = fp.sample_fmt;
    p.num_stages = fp.num_stages;
    std::vector<float> taps;
    uint64_t decim = 1;
    for (uint32_t s = 0; s < fp.num_stages && s < (uint32_t)kMaxStages; ++s) {
        FirStageDev d{};
        d.decim = fp.stage[s].decim;
        d.ntaps = d.ntaps_pad = fp.stage[s].ntaps;
        d.tap_off = (uint32_t)taps.size();
        taps.insert(taps.end(), plan.taps.begin() + fp.stage[s].tap_off, plan.taps.begin() + fp.stage[s].tap_off + fp.stage[s].ntaps);
        p.stage[s] = d;
        decim *= d.decim;
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
    const size_t table_bytes = (size_t)kRunMomentTableSegs * kRunMomentSums * sizeof(uint64_t);
    if (!survey_tile_lag(p, &ctx.lds_bytes, tuned ? 2u : 1u, table_bytes)) {
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
    ctx.decimation = (uint32_t)decim;
    // (developers: how many of a tile's segments are summed in LDS, 0 = every wave adds to global memory)
    if (const char *t = dev_getenv("OOKD_MOMENTS_TABLE")) ctx.table_segs = (uint32_t)std::min<long>(kRunMomentTableSegs, std::max<long>(0, atol(t)));
    ctx.sv = p;
    ctx.built = true;
    return OOKD_OK;
}

// The pass behind every entry point: `ctx` has answered the context's last run when this returns OOKD_OK.
// clean = false: the run's own edge list (pass kEdgePassMoments); true: the cleaned list (kEdgePassCleanMoments).
int moments_pass(const char *who, bool clean, ookd_rx *rx, uint32_t capture, RunMomentCtx *&ctx) {
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    if (clean && !clean_run_view(rx, run)) {
        set_error("%s: no cleaned list of the last run (ookd_rx_clean_edges first)", who);
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, clean ? kEdgePassCleanMoments : kEdgePassMoments);
    if (!slot) slot.reset(new (std::nothrow) RunMomentCtx());
    ctx = static_cast<RunMomentCtx *>(slot.get());
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
    ctx->slots = run_peak_slots(run.num_edges, run.captures);
    const size_t sum_word = (size_t)run.captures * kRunMomentWords;
    const size_t words = sum_word + (size_t)ctx->slots * kRunMomentSums;
    ctx->host.assign(words, 0);
    if (run.n_out == 0) {               // no buffer was processed: nothing was written for the kernel to read
        ctx->serial = run.serial;
        ctx->kernel_ms = 0.0f;
        return OOKD_OK;
    }
    RunMomentParams p{};
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
    p.slots = ctx->slots;
    p.table_segs = ctx->table_segs;
    const size_t lds_bytes = ctx->lds_bytes;
    return ctx->run(who, run, words, ctx->host.data(), [&](unsigned long long *d) {
        p.result = d;
        p.moments = d + sum_word;
        return launch_run_moments(p, lds_bytes, run.stream);
    });
}

// capture's R, and its sums inside ctx->host
const uint64_t *sums_of(const RunMomentCtx &ctx, uint32_t capture, uint64_t &runs) {
    const uint64_t *r = ctx.host.data() + (size_t)capture * kRunMomentWords;
    runs = (r[0] + 1u) / 2u;
    const uint64_t base = run_peak_base(r[2], capture);
    if (base + runs > ctx.slots) runs = base < ctx.slots ? ctx.slots - base : 0;
    return ctx.host.data() + (size_t)ctx.captures * kRunMomentWords + (size_t)std::min(base, ctx.slots) * kRunMomentSums;
}

int run_moments(const char *who, bool clean, ookd_rx *rx, uint32_t capture, ookd_run_moments *out) {
    clear_error();
    if (!rx || !out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    RunMomentCtx *ctx = nullptr;
    if (const int rc = moments_pass(who, clean, rx, capture, ctx); rc != OOKD_OK) return rc;
    memset(out, 0, sizeof *out);
    uint64_t runs = 0;
    (void)sums_of(*ctx, capture, runs);
    out->num_runs = runs;
    out->tile_outputs = ctx->sv.tile;
    out->decimation = ctx->decimation;
    out->tiles_total = (ctx->n_out + ctx->sv.tile - 1) / ctx->sv.tile;
    out->tiles_filtered = ctx->host[(size_t)capture * kRunMomentWords + 1u];
    return OOKD_OK;
}

int get_moments(const char *who, bool clean, ookd_rx *rx, uint32_t capture, ookd_run_moment *m, uint64_t capacity, uint64_t *num_runs) {
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    RunMomentCtx *ctx = nullptr;
    if (const int rc = moments_pass(who, clean, rx, capture, ctx); rc != OOKD_OK) return rc;
    uint64_t runs = 0;
    const uint64_t *from = sums_of(*ctx, capture, runs);
    if (num_runs) *num_runs = runs;
    const uint64_t take = std::min<uint64_t>(runs, capacity);
    if (m && take) memcpy(m, from, take * sizeof(ookd_run_moment));
    return OOKD_OK;
}

// the arguments ookd_message_levels refuses, under another name
int check_lists(const char *who, const uint64_t *edges, uint64_t E, const void *per_run, uint64_t R) {
    if ((E && !edges) || (R && !per_run)) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (R != (E + 1u) / 2u) {
        set_error("%s: %llu on-runs for %llu edges (ceil(E / 2) on-runs)", who, (unsigned long long)R, (unsigned long long)E);
        return OOKD_ERR_ARG;
    }
    return OOKD_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(ookd_run_moment) == kRunMomentSums * sizeof(uint64_t), "ookd_run_moment is the kernel's three sums");
static_assert(sizeof(ookd_run_moments) == 32, "ookd_run_moments layout");
static_assert(sizeof(ookd_message_carrier) == 32, "ookd_message_carrier layout");

int ookd_rx_run_moments(ookd_rx *rx, uint32_t capture, ookd_run_moments *out) {
    return run_moments("ookd_rx_run_moments", false, rx, capture, out);
}

int ookd_rx_run_moments_clean(ookd_rx *rx, uint32_t capture, ookd_run_moments *out) {
    return run_moments("ookd_rx_run_moments_clean", true, rx, capture, out);
}

int ookd_rx_get_run_moments(ookd_rx *rx, uint32_t capture, ookd_run_moment *moments, uint64_t capacity, uint64_t *num_runs) {
    return get_moments("ookd_rx_get_run_moments", false, rx, capture, moments, capacity, num_runs);
}

int ookd_rx_get_run_moments_clean(ookd_rx *rx, uint32_t capture, ookd_run_moment *moments, uint64_t capacity, uint64_t *num_runs) {
    return get_moments("ookd_rx_get_run_moments_clean", true, rx, capture, moments, capacity, num_runs);
}

float ookd_rx_moments_kernel_ms(const ookd_rx *rx) { return edge_pass_kernel_ms(rx, kEdgePassMoments); }

int ookd_run_moments_of(const float *y, uint64_t n_out, const uint64_t *edges, uint64_t E, ookd_run_moment *out, uint64_t R) {
    clear_error();
    if (const int rc = check_lists("ookd_run_moments_of", edges, E, out, R); rc != OOKD_OK) return rc;
    if (n_out && !y) {
        set_error("ookd_run_moments_of: NULL argument");
        return OOKD_ERR_ARG;
    }
    for (uint64_t k = 0; k < E; ++k) {
        if (edges[k] >= n_out || (k && edges[k] <= edges[k - 1])) {
            set_error("ookd_run_moments_of: edges must ascend strictly below n_out (edge %llu)", (unsigned long long)k);
            return OOKD_ERR_ARG;
        }
    }
    for (uint64_t r = 0; r < R; ++r) {
        const uint64_t a = edges[2 * r], f = 2 * r + 1 < E ? edges[2 * r + 1] : n_out;
        uint64_t power = 0, lag_re = 0, lag_im = 0;     // unsigned: the sums wrap modulo 2^64
        for (uint64_t j = a; j < f; ++j) {
            const float re = y[2 * j], im = y[2 * j + 1];
            const float rr = re * re;
            const float ii = im * im;
            power += moment_q(rr + ii);
            if (j > a) {
                const float pre = y[2 * j - 2], pim = y[2 * j - 1];
                const float t0 = re * pre;
                const float t1 = im * pim;
                const float t2 = im * pre;
                const float t3 = re * pim;
                lag_re += moment_q(t0 + t1);
                lag_im += moment_q(t2 - t3);
            }
        }
        out[r].power = (int64_t)power;
        out[r].lag_re = (int64_t)lag_re;
        out[r].lag_im = (int64_t)lag_im;
    }
    return OOKD_OK;
}

int ookd_message_carriers(const uint64_t *edges, uint64_t E, uint64_t n_out, const ookd_run_moment *moments, uint64_t R,
                          const uint64_t *msg_samples, uint64_t M, uint32_t pulses, uint32_t decimation, double nu,
                          ookd_message_carrier *out) {
    clear_error();
    if (const int rc = check_lists("ookd_message_carriers", edges, E, moments, R); rc != OOKD_OK) return rc;
    if (M && (!msg_samples || !out)) {
        set_error("ookd_message_carriers: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (pulses == 0) {
        set_error("ookd_message_carriers: pulses must be at least 1");
        return OOKD_ERR_ARG;
    }
    if (decimation == 0) {
        set_error("ookd_message_carriers: decimation must be at least 1");
        return OOKD_ERR_ARG;
    }
    if ((E & 1u) && edges[E - 1] >= n_out) {
        set_error("ookd_message_carriers: the open last run begins at or beyond n_out");
        return OOKD_ERR_ARG;
    }
    for (uint64_t m = 1; m < M; ++m) {
        if (msg_samples[m] < msg_samples[m - 1]) {
            set_error("ookd_message_carriers: msg_samples must ascend (message %llu)", (unsigned long long)m);
            return OOKD_ERR_ARG;
        }
    }
    const double D = (double)decimation;
    const double two_pi = 6.283185307179586476925286766559;
    uint64_t r = 0;                     // the first on-run no earlier message took
    for (uint64_t m = 0; m < M; ++m) {
        uint64_t end = r;               // on-runs [r, end) rise at or below msg_samples[m]
        while (end < R && edges[2 * end] <= msg_samples[m]) ++end;
        const uint64_t count = std::min<uint64_t>(end - r, pulses);
        double P = 0.0, Zr = 0.0, Zi = 0.0, len = 0.0;
        for (uint64_t i = end - count; i < end; ++i) {
            P += (double)moments[i].power;
            Zr += (double)moments[i].lag_re;
            Zi += (double)moments[i].lag_im;
            len += (double)((2 * i + 1 < E ? edges[2 * i + 1] : n_out) - edges[2 * i]);
        }
        ookd_message_carrier &o = out[m];
        o.outputs = (uint64_t)len;
        o.mean_power = len > 0.0 ? P / 1073741824.0 / len : 0.0;
        o.coherence = P != 0.0 ? std::hypot(Zr, Zi) / P : 0.0;
        o.carrier = nu;
        if (Zr != 0.0 || Zi != 0.0) {
            const double x = std::atan2(Zi, Zr) / two_pi - nu * D;
            o.carrier = nu + (x - std::floor(x + 0.5)) / D;
        } else {
            o.coherence = 0.0;
        }
        r = end;
    }
    return OOKD_OK;
}

}  // extern "C"
