// scan_ctx.cpp -- the host skeleton shared by the survey and spectrum contexts (scan_ctx.hpp).
#include "scan_ctx.hpp"

namespace ookd {

ScanCtx::~ScanCtx() {
    if (dev < 0) return;
    (void)hipSetDevice(dev);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

bool scan_ctx_check_create(const char *who, uint32_t sample_flags, uint32_t max_captures) {
    const uint32_t both = OOKD_RX_SAMPLES_CS8 | OOKD_RX_SAMPLES_CU8;
    if ((sample_flags & ~both) || (sample_flags & both) == both) {
        set_error("%s: sample_flags must be 0, OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8", who);
        return false;
    }
    if (max_captures == 0 || max_captures > 65535u) {
        set_error("%s: max_captures must be 1 .. 65535", who);
        return false;
    }
    return true;
}

bool scan_ctx_open(ScanCtx &c, const char *who, int32_t hip_device, uint32_t sample_flags, uint32_t max_captures,
                   void *stream) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || hip_device < 0 || hip_device >= ndev) {
        set_error("no HIP device %d available: libookiedokie_amd has no CPU fallback", hip_device);
        return false;
    }
    c.dev = hip_device;
    c.max_captures = max_captures;
    c.fmt = (sample_flags & OOKD_RX_SAMPLES_CS8) ? kFmtCs8 : (sample_flags & OOKD_RX_SAMPLES_CU8) ? kFmtCu8 : kFmtSc16;
    (void)hipSetDevice(hip_device);
    if (stream) {
        c.stream = static_cast<hipStream_t>(stream);
    } else {
        if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("%s: hipStreamCreate failed: %s", who, hipGetErrorString(hipGetLastError()));
            return false;
        }
        c.own_stream = true;
    }
    if (hipEventCreate(&c.t0) != hipSuccess || hipEventCreate(&c.t1) != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return false;
    }
    return true;
}

int scan_ctx_check_run(const ScanCtx *c, const char *who, const void *d_iq, uint32_t num_captures,
                       uint64_t samples_per_capture, uint64_t capture_stride_samples, bool strict_layout) {
    if (!c || num_captures == 0 || num_captures > c->max_captures || (!d_iq && samples_per_capture) ||
        (num_captures > 1 && capture_stride_samples < samples_per_capture)) {
        set_error("%s: bad argument (captures %u of at most %u, %llu samples, stride %llu)", who, num_captures,
                  c ? c->max_captures : 0, (unsigned long long)samples_per_capture,
                  (unsigned long long)capture_stride_samples);
        return OOKD_ERR_ARG;
    }
    if ((samples_per_capture >> 48) || (strict_layout && (capture_stride_samples >> 48))) {
        set_error("%s: captures of 2^48 samples and more are not supported", who);
        return OOKD_ERR_ARG;
    }
    const uint32_t sb = sample_bytes(c->fmt);
    if (strict_layout && (uintptr_t)d_iq % sb) {
        set_error("%s: the capture is not aligned to its %u-byte samples", who, sb);
        return OOKD_ERR_ARG;
    }
    return OOKD_OK;
}

int scan_ctx_stage(const ScanCtx *c, const char *who, const void *iq, uint64_t num_samples, void **buf,
                   size_t *capacity) {
    if (!c || (!iq && num_samples)) {
        set_error("%s: bad argument", who);
        return OOKD_ERR_ARG;
    }
    (void)hipSetDevice(c->dev);
    const size_t bytes = (size_t)num_samples * sample_bytes(c->fmt);
    if (bytes > *capacity) {
        if (*buf) (void)hipFree(*buf);
        *buf = nullptr;
        *capacity = 0;
        if (hipMalloc(buf, bytes) != hipSuccess) {
            *buf = nullptr;
            set_error("%s: cannot allocate %zu bytes of device memory", who, bytes);
            return OOKD_ERR_NOMEM;
        }
        *capacity = bytes;
    }
    if (bytes && hipMemcpy(*buf, iq, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_HIP;
    }
    return OOKD_OK;
}

}  // namespace ookd
