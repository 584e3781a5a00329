// edge_pass.cpp -- the host skeleton shared by the edge-list readers (edge_pass.hpp).
#include "edge_pass.hpp"

namespace ookd {

EdgePass::~EdgePass() {
    if (d_result) (void)hipFree(d_result);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
}

int EdgePass::run(const char *who, const EdgeRun &run, size_t words, uint64_t *host,
                  const std::function<hipError_t(unsigned long long *)> &queue) {
    serial = 0;
    kernel_ms = 0.0f;
    if (const int rc = reserve_result(who, run.dev, words); rc != OOKD_OK) return rc;
    if (!t0 && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess)) {
        set_error("%s: hipEventCreate failed", who);
        return OOKD_ERR_HIP;
    }
    const size_t bytes = words * 8;
    bool ok = hipEventRecord(t0, run.stream) == hipSuccess;
    ok = ok && hipMemsetAsync(d_result, 0, bytes, run.stream) == hipSuccess;
    ok = ok && queue(d_result) == hipSuccess;
    ok = ok && hipEventRecord(t1, run.stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(host, d_result, bytes, hipMemcpyDeviceToHost, run.stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(run.stream) == hipSuccess;
    if (!ok) {
        set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    if (hipEventElapsedTime(&kernel_ms, t0, t1) != hipSuccess) {
        set_error("%s: hipEventElapsedTime failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    serial = run.serial;
    return OOKD_OK;
}

int EdgePass::reserve_result(const char *who, int dev, size_t words) {
    if (hipSetDevice(dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    if (capacity < words) {
        if (d_result) (void)hipFree(d_result);
        d_result = nullptr;
        capacity = 0;
        if (hipMalloc(reinterpret_cast<void **>(&d_result), words * 8) != hipSuccess) {
            d_result = nullptr;
            set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
            return OOKD_ERR_NOMEM;
        }
        capacity = words;
    }
    return OOKD_OK;
}

int edge_run_check(const char *who, const ookd_rx *rx, uint32_t capture, EdgeRun &run) {
    ookd_rx_edge_run(rx, &run);
    if (run.serial == 0 || run.in_flight || !run.valid) {
        set_error("%s: no finished run to look at%s", who,
                  run.in_flight ? " (ookd_rx_wait first)" : run.serial ? " (the last run failed before its edges were counted)" : "");
        return OOKD_ERR_ARG;
    }
    if (run.shard) {
        set_error("%s: the last run was a shard run: the level in front of a shard is not known here", who);
        return OOKD_ERR_ARG;
    }
    if (run.pipelined) {
        set_error("%s: the last run was pipelined in chunks: its edge lists are chunk-local "
                  "(OOKD_RX_NO_PIPELINE, or pipeline_chunk_samples = 0)", who);
        return OOKD_ERR_ARG;
    }
    if (capture >= run.captures) {
        set_error("%s: capture %u of %u", who, capture, run.captures);
        return OOKD_ERR_ARG;
    }
    if (run.overflow) {
        set_error("%s: the run's edge list overflowed (%llu level changes, capacity %llu): raise "
                  "ookd_rx_config.edge_capacity", who, (unsigned long long)run.num_edges, (unsigned long long)run.edge_capacity);
        return OOKD_ERR_CAPACITY;
    }
    return OOKD_OK;
}

float edge_pass_kernel_ms(const ookd_rx *rx, EdgePassId id) {
    if (!rx) return 0.0f;
    EdgeRun run;
    ookd_rx_edge_run(rx, &run);
    const EdgePass *p = ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), id).get();
    return p && run.serial != 0 && p->serial == run.serial ? p->kernel_ms : 0.0f;
}

}  // namespace ookd
