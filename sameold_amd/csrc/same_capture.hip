// same_capture.hip -- alert audio out of a launch's input (same_batch_set_audio_capture): the transport kernel
// (same_transport.hip) has listed, per channel, the rows of this launch that belong to an open message and reserved their room
// in the launch's pool (same_capture_dev.h); this kernel copies them there.  It runs behind the transport kernel on the launch's
// stream, while the input is still the caller's to read (include/same_rx.h, "Stream contract"), and ahead of the launch's
// done event, which every later reuse of that input waits for.
//
// The plain strided copy: a workgroup per span (grid-strided over the list, whose length it reads on the device), its lanes on
// consecutive rows of the span -- reads n_channels * 4 bytes apart, writes coalesced.
#include <hip/hip_runtime.h>

#include "same_launch.h"

namespace same {

namespace {

constexpr uint32_t kCaptureBlocks = 1024, kCaptureThreads = 256;

template <typename T>
__global__ __launch_bounds__(kCaptureThreads) void capture_kernel(const cap::Span *__restrict__ spans, const cap::Cursors *__restrict__ cur,
                                                                  uint32_t span_cap, float *__restrict__ pool, uint64_t pool_cap,
                                                                  const T *__restrict__ x, uint32_t n_channels, uint32_t n_rows)
{
    const uint32_t n_spans = min(cur->n_spans, span_cap);
    for (uint32_t s = blockIdx.x; s < n_spans; s += gridDim.x) {
        const cap::Span sp = spans[s];
        // (the transport kernel keeps every span inside the launch and the pool; checked once more before a byte moves)
        if (sp.n == 0 || sp.channel >= n_channels || sp.row0 > n_rows || sp.n > n_rows - sp.row0 || sp.off > pool_cap ||
            sp.n > pool_cap - sp.off)
            continue;
        const T *src = x + (size_t)sp.row0 * n_channels + sp.channel;
        float *dst = pool + sp.off;
        for (uint32_t i = threadIdx.x; i < sp.n; i += kCaptureThreads) dst[i] = (float)src[(size_t)i * n_channels];
    }
}

// the launch's cursors to the host (host-mapped memory), then zero for the slot's next launch
__global__ void capture_epilogue_kernel(cap::Cursors *cur, volatile cap::Cursors *host)
{
    if (threadIdx.x == 0) {
        const cap::Cursors c = *cur;
        host->n_spans = c.n_spans; host->overflow = c.overflow; host->pool_used = c.pool_used;
        cur->n_spans = 0; cur->overflow = 0; cur->pool_used = 0;
    }
}

template <typename T>
hipError_t launch_capture_t(const cap::Span *spans, cap::Cursors *cur, uint32_t span_cap, float *pool, uint64_t pool_cap, const T *x,
                            uint32_t n_channels, uint32_t n_rows, cap::Cursors *host, hipStream_t stream)
{
    hipLaunchKernelGGL(capture_kernel<T>, dim3(kCaptureBlocks), dim3(kCaptureThreads), 0, stream, spans, cur, span_cap, pool, pool_cap, x,
                       n_channels, n_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(capture_epilogue_kernel, dim3(1), dim3(64), 0, stream, cur, host);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_capture(const cap::Span *spans, cap::Cursors *cur, uint32_t span_cap, float *pool, uint64_t pool_cap,
                          const float *x, uint32_t n_channels, uint32_t n_rows, cap::Cursors *host, hipStream_t stream)
{
    return launch_capture_t(spans, cur, span_cap, pool, pool_cap, x, n_channels, n_rows, host, stream);
}
hipError_t launch_capture(const cap::Span *spans, cap::Cursors *cur, uint32_t span_cap, float *pool, uint64_t pool_cap,
                          const int16_t *x, uint32_t n_channels, uint32_t n_rows, cap::Cursors *host, hipStream_t stream)
{
    return launch_capture_t(spans, cur, span_cap, pool, pool_cap, x, n_channels, n_rows, host, stream);
}

}  // namespace same
