// pulses.cpp -- pulse survey: the C ABI around pulses.hip's histogram kernel, and the host-only half -- the bin rule
// and the timing classes (include/ookiedokie_amd.h states both as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "pulses.hpp"

using namespace ookd;

static_assert(OOKD_PULSE_BINS == kPulseBins, "OOKD_PULSE_BINS");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram word");

namespace ookd {

struct PulseCtx {
    unsigned long long *d_result = nullptr;     // [captures][kPulseWords]
    uint32_t capacity = 0;                      // captures d_result holds
    hipEvent_t t0 = nullptr, t1 = nullptr;
    uint64_t serial = 0;                        // the run `host` belongs to (PulseRun::serial), 0 = none
    float kernel_ms = 0.0f;
    std::vector<uint64_t> host;                 // its results
};

void pulse_ctx_free(PulseCtx *p) {
    if (!p) return;
    if (p->d_result) (void)hipFree(p->d_result);
    if (p->t0) (void)hipEventDestroy(p->t0);
    if (p->t1) (void)hipEventDestroy(p->t1);
    delete p;
}

}  // namespace ookd

namespace {

// one launch for all captures of the run; the results stay in c.host until the next run
int compute(PulseCtx &c, const PulseRun &run) {
    c.serial = 0;
    c.kernel_ms = 0.0f;
    c.host.assign((size_t)run.captures * kPulseWords, 0);
    if (run.n_out == 0) {               // no buffer was processed: nothing was written for the kernel to read
        c.serial = run.serial;
        return OOKD_OK;
    }
    if (hipSetDevice(run.dev) != hipSuccess) {
        set_error("ookd_rx_pulse_hist: hipSetDevice failed");
        return OOKD_ERR_HIP;
    }
    if (c.capacity < run.captures) {
        if (c.d_result) (void)hipFree(c.d_result);
        c.d_result = nullptr;
        c.capacity = 0;
        if (hipMalloc(reinterpret_cast<void **>(&c.d_result), (size_t)run.captures * kPulseWords * 8) != hipSuccess) {
            set_error("ookd_rx_pulse_hist: device allocation failed: %s", hipGetErrorString(hipGetLastError()));
            return OOKD_ERR_NOMEM;
        }
        c.capacity = run.captures;
    }
    if (!c.t0 && (hipEventCreate(&c.t0) != hipSuccess || hipEventCreate(&c.t1) != hipSuccess)) {
        set_error("ookd_rx_pulse_hist: hipEventCreate failed");
        return OOKD_ERR_HIP;
    }
    PulseParams p{};
    p.edges = run.d_edges;
    p.edge_capacity = run.edge_capacity;
    p.blk_offset = run.d_blk_offset;
    p.blocks_per_cap = run.blocks_per_cap;
    p.num_captures = run.captures;
    p.result = c.d_result;
    const size_t bytes = c.host.size() * 8;
    bool ok = hipEventRecord(c.t0, run.stream) == hipSuccess;
    ok = ok && hipMemsetAsync(c.d_result, 0, bytes, run.stream) == hipSuccess;
    ok = ok && launch_pulse_hist(p, run.num_edges, run.stream) == hipSuccess;
    ok = ok && hipEventRecord(c.t1, run.stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(c.host.data(), c.d_result, bytes, hipMemcpyDeviceToHost, run.stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(run.stream) == hipSuccess;
    if (!ok) {
        set_error("ookd_rx_pulse_hist: HIP failure: %s", hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    if (hipEventElapsedTime(&c.kernel_ms, c.t0, c.t1) != hipSuccess) {
        set_error("ookd_rx_pulse_hist: hipEventElapsedTime failed: %s", hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    c.serial = run.serial;
    return OOKD_OK;
}

struct ClassAcc {
    uint32_t first = 0, last = 0;
    uint64_t runs = 0;
    unsigned __int128 sum = 0;
};

double to_us(double x, double rate) { return rate > 0.0 ? x / rate * 1e6 : 0.0; }

}  // namespace

extern "C" {

uint32_t ookd_pulse_bin(uint64_t length) { return pulse_bin_of(length); }

uint64_t ookd_pulse_bin_lower(uint32_t bin) {
    if (bin < 32u) return bin;
    const uint64_t m = 16u + (bin - 32u) % 16u;         // five significant bits
    const uint32_t sh = 1u + (bin - 32u) / 16u;
    return sh > 59u ? UINT64_MAX : m << sh;
}

int ookd_rx_pulse_hist(ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out) {
    clear_error();
    if (!rx || !out) {
        set_error("ookd_rx_pulse_hist: NULL argument");
        return OOKD_ERR_ARG;
    }
    PulseRun run;
    ookd_rx_pulse_run(rx, &run);
    if (run.serial == 0 || run.in_flight || !run.valid) {
        set_error("ookd_rx_pulse_hist: no finished run to look at%s",
                  run.in_flight ? " (ookd_rx_wait first)" : run.serial ? " (the last run failed before its edges were counted)" : "");
        return OOKD_ERR_ARG;
    }
    if (run.shard) {
        set_error("ookd_rx_pulse_hist: the last run was a shard run: the level in front of a shard is not known here");
        return OOKD_ERR_ARG;
    }
    if (run.pipelined) {
        set_error("ookd_rx_pulse_hist: the last run was pipelined in chunks: its edge lists are chunk-local "
                  "(OOKD_RX_NO_PIPELINE, or pipeline_chunk_samples = 0)");
        return OOKD_ERR_ARG;
    }
    if (capture >= run.captures) {
        set_error("ookd_rx_pulse_hist: capture %u of %u", capture, run.captures);
        return OOKD_ERR_ARG;
    }
    if (run.overflow) {
        set_error("ookd_rx_pulse_hist: the run's edge list overflowed (%llu level changes, capacity %llu): raise "
                  "ookd_rx_config.edge_capacity", (unsigned long long)run.num_edges, (unsigned long long)run.edge_capacity);
        return OOKD_ERR_CAPACITY;
    }
    PulseCtx *&ctx = *ookd_rx_pulse_ctx(rx);
    if (!ctx) ctx = new (std::nothrow) PulseCtx();
    if (!ctx) {
        set_error("ookd_rx_pulse_hist: out of memory");
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial != run.serial) {
        const int rc = compute(*ctx, run);
        if (rc != OOKD_OK) return rc;
    }
    const uint64_t *r = ctx->host.data() + (size_t)capture * kPulseWords;
    memset(out, 0, sizeof *out);
    for (uint32_t lv = 0; lv < 2; ++lv) {
        for (uint32_t b = 0; b < (uint32_t)kPulseBins; ++b) {
            out->count[lv][b] = r[2u * (lv * kPulseBins + b)];
            out->sum[lv][b] = r[2u * (lv * kPulseBins + b) + 1u];
            out->runs[lv] += out->count[lv][b];
        }
    }
    const uint64_t E = r[kPulseMetaWord];
    out->num_edges = E;
    out->samples = run.n_out;
    out->open_head = E ? r[kPulseMetaWord + 1] : run.n_out;
    out->open_tail = E ? run.n_out - r[kPulseMetaWord + 2] : 0;
    out->tail_level = (uint32_t)(E & 1u);
    return OOKD_OK;
}

float ookd_rx_pulse_kernel_ms(const ookd_rx *rx) {
    if (!rx) return 0.0f;
    PulseRun run;
    ookd_rx_pulse_run(rx, &run);
    const PulseCtx *ctx = *ookd_rx_pulse_ctx(const_cast<ookd_rx *>(rx));
    return ctx && run.serial != 0 && ctx->serial == run.serial ? ctx->kernel_ms : 0.0f;
}

int ookd_suggest_pulses(const ookd_pulse_hist *h, double sample_rate, ookd_pulse_suggestion *out) {
    clear_error();
    if (!h || !out) {
        set_error("ookd_suggest_pulses: NULL argument");
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    bool both = true;
    for (uint32_t lv = 0; lv < 2; ++lv) {
        std::vector<ClassAcc> cls;                      // ascending in length
        for (uint32_t b = 0; b < (uint32_t)kPulseBins; ++b) {
            if (!h->count[lv][b]) continue;
            if (cls.empty() || b - cls.back().last >= (uint32_t)OOKD_PULSE_CLASS_GAP) {
                cls.emplace_back();
                cls.back().first = b;
            }
            ClassAcc &c = cls.back();
            c.last = b;
            c.runs += h->count[lv][b];
            c.sum += h->sum[lv][b];
        }
        std::vector<uint32_t> keep(cls.size());
        for (uint32_t i = 0; i < keep.size(); ++i) keep[i] = i;
        if (keep.size() > (size_t)OOKD_PULSE_MAX_CLASSES) {
            // most runs first, the shorter class on a tie; then back into ascending order
            std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return cls[a].runs > cls[b].runs; });
            for (size_t i = OOKD_PULSE_MAX_CLASSES; i < keep.size(); ++i) out->dropped_runs[lv] += cls[keep[i]].runs;
            keep.resize(OOKD_PULSE_MAX_CLASSES);
            std::sort(keep.begin(), keep.end());
        }
        bool two = false;
        for (uint32_t i = 0; i < keep.size(); ++i) {
            const ClassAcc &c = cls[keep[i]];
            ookd_pulse_class &o = out->classes[lv][i];
            o.first_bin = c.first;
            o.last_bin = c.last;
            o.runs = c.runs;
            o.mean = (double)c.sum / (double)c.runs;
            o.lower = ookd_pulse_bin_lower(c.first);
            o.upper = ookd_pulse_bin_lower(c.last + 1u) - 1u;
            o.mean_us = to_us(o.mean, sample_rate);
            o.lower_us = to_us((double)o.lower, sample_rate);
            o.upper_us = to_us((double)o.upper, sample_rate);
            two = two || c.runs >= 2;
        }
        out->num_classes[lv] = (uint32_t)keep.size();
        both = both && two;
    }
    out->found = both ? 1 : 0;
    return OOKD_OK;
}

}  // extern "C"
