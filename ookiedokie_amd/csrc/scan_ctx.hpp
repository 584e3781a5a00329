// scan_ctx.hpp -- what the capture-scanning contexts (ookd_survey, survey.cpp; ookd_spectrum, spectrum.cpp) have in
// common on the host: the device, a borrowed or owned stream, the sample format, the capture limit, the event pair
// that times the kernel, and the checks and the staging copy of their *_create, *_device and *_host entry points.
// `who` names the entry point in the messages.  (HIP types: kept out of common.hpp, which has none.)
#pragma once

#include "common.hpp"
#include "kernels.hpp"

namespace ookd {

struct ScanCtx {
    int dev = -1;                   // < 0: scan_ctx_open has not got as far as the device
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t fmt = kFmtSc16;        // kFmt*
    uint32_t max_captures = 1;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    float kernel_ms = 0.0f;         // of the last run

    ScanCtx() = default;
    ScanCtx(const ScanCtx &) = delete;
    ScanCtx &operator=(const ScanCtx &) = delete;
    // (a context derived from this one frees what it owns in its own destructor, which runs first)
    ~ScanCtx();
};

// The arguments of a *_create that need no device: sample_flags (0 or one of OOKD_RX_SAMPLES_*) and max_captures.
// false + error.
bool scan_ctx_check_create(const char *who, uint32_t sample_flags, uint32_t max_captures);
// The device check ("no CPU fallback"), then the context's fields, its stream (`stream`, or one of its own when
// null) and its events.  false + error; whatever was created goes with the context.
bool scan_ctx_open(ScanCtx &c, const char *who, int32_t hip_device, uint32_t sample_flags, uint32_t max_captures,
                   void *stream);
// The arguments of a *_device run: OOKD_OK, or OOKD_ERR_ARG + error.  strict_layout: also refuse a capture stride of
// 2^48 samples and more and a capture that is not aligned to its samples (the spectrum does, the survey does not).
int scan_ctx_check_run(const ScanCtx *c, const char *who, const void *d_iq, uint32_t num_captures,
                       uint64_t samples_per_capture, uint64_t capture_stride_samples, bool strict_layout);
// A *_host run's capture -> device memory: *buf, a buffer of *capacity bytes that is grown (never shrunk) to hold
// it.  Whether the buffer outlives the run is the caller's policy.  OOKD_OK or an error code + error.
int scan_ctx_stage(const ScanCtx *c, const char *who, const void *iq, uint64_t num_samples, void **buf,
                   size_t *capacity);

}  // namespace ookd
