// same_tone_delivery.hip -- the kernels of tone-alert audio in delivery form (include/same_tone_delivery.h).
// The arithmetic is same_tone_delivery_dev.h's (one text for g++ and the device).  same_tones.hip queues these behind the
// capture work of same_tone_audio.hip, whose float pool is then a staging buffer that never leaves the device.
//   tone_delivery_place_kernel     one workgroup, as tone_audio_place_kernel: every placed chunk's outputs (td::out_of), then an
//                                  exclusive prefix sum over the channels' delivered counts, 1024 channels per round with the
//                                  total carried along, hands out the delivery pool in chunk order.  Chunks are packed: no
//                                  padding, no atomics.  The total is the pool's use, the third word of the call's header.
//   tone_delivery_decimate_kernel  the hot path.  A workgroup of 256 lanes belongs to a group of 64 channels and exits at once
//                                  when the group's flag is clear.  Otherwise it walks the group's chunks and takes every
//                                  gridDim.y-th tile of 256 outputs, rotated by the channel so that the short chunks of many
//                                  channels spread over the workgroups.  A tile's input window -- up to 255 * 6 + 1 + 96 source
//                                  samples, from the staging pool and, in front of a chunk that continues a capture, the
//                                  channel's history -- is staged in LDS with the lanes along source time; then the lanes lie
//                                  along output time: lane i sums T taps of phase (p0 + i M) mod L over the window downwards
//                                  from floor((p0 + i M) / L), quantises, and stores one int16, 128 contiguous bytes per
//                                  wavefront.  The taps come from the [j][p] table in global memory (T L floats, up to 29 KB
//                                  at 22 050 -> 8 000: it stays in the caches, and does not fit LDS at the ratios' limit).
//   tone_delivery_history_kernel   lane = channel, behind the decimator in stream order: td::history_step on the call's input.
#include <hip/hip_runtime.h>

#include "../../include/same_rx.h"
#include "same_tone_delivery_kernels.h"

namespace same {
namespace {

constexpr uint32_t kPlaceThreads = 1024;
constexpr uint32_t kGroup = 64;
constexpr uint32_t kMaxGridY = 64;

__global__ __launch_bounds__(kPlaceThreads) void tone_delivery_place_kernel(ToneAudioCall k, ToneDeliveryCall dk)
{
    __shared__ uint64_t wave_sum[kPlaceThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t *n_spans = (const uint32_t *)(k.out + kCapHeaderBytes);
    const tn::Span *spans = (const tn::Span *)(k.out + cap_spans_offset(k.n_channels));
    td::Out *outs = (td::Out *)(k.out + dk.outs_offset);
    uint64_t carry = 0;                               // delivered samples of the channels before this round, the same in every thread
    for (uint32_t c0 = 0; c0 < k.n_channels; c0 += kPlaceThreads) {
        const uint32_t c = c0 + threadIdx.x;
        const bool valid = c < k.n_channels;
        const uint32_t n = valid ? n_spans[c] : 0, at = valid ? k.span_off[c] : 0;
        uint64_t v = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const td::Out o = td::out_of(spans[at + i], dk.a_next[c], dk.params, v);
            outs[at + i] = o;
            v += o.n_out;
        }
        uint64_t incl = v;
        for (uint32_t m = 1; m < 64; m <<= 1) {
            const uint64_t o = __shfl_up((unsigned long long)incl, m, 64);
            if (lane >= m) incl += o;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, round = 0;
        for (uint32_t w = 0; w < kPlaceThreads / 64; ++w) {
            const uint64_t s = wave_sum[w];
            if (w < wave) before += s;
            round += s;
        }
        const uint64_t base = carry + before + (incl - v);
        for (uint32_t i = 0; i < n; ++i) outs[at + i].off += base;
        carry += round;
        __syncthreads();                              // (wave_sum is written again by the next round)
    }
    if (threadIdx.x == 0) ((uint64_t *)k.out)[2] = carry;
}

__global__ __launch_bounds__(td::kTileOutputs) void tone_delivery_decimate_kernel(ToneAudioCall k, ToneDeliveryCall dk)
{
    __shared__ float w[td::kWindowMax];
    if (!k.flags[blockIdx.x]) return;
    const uint32_t C = k.n_channels, tid = threadIdx.x;
    const uint32_t *n_spans = (const uint32_t *)(k.out + kCapHeaderBytes);
    const tn::Span *spans = (const tn::Span *)(k.out + cap_spans_offset(C));
    const td::Out *outs = (const td::Out *)(k.out + dk.outs_offset);
    const td::Params p = dk.params;
    // (every bound below is read from the call's records and is the same in every lane: the barriers are met by all)
    for (uint32_t ch = 0; ch < kGroup; ++ch) {
        const uint32_t c = blockIdx.x * kGroup + ch;
        if (c >= C) break;
        const uint32_t n = n_spans[c], at = k.span_off[c];
        const float *hist = dk.hist + (size_t)c * (p.T - 1);
        const uint32_t t0 = (blockIdx.y + gridDim.y - ch % gridDim.y) % gridDim.y;
        for (uint32_t i = 0; i < n; ++i) {
            const tn::Span s = spans[at + i];
            const td::Out o = outs[at + i];
            const uint64_t tiles = (o.n_out + td::kTileOutputs - 1) / td::kTileOutputs;
            for (uint64_t t = t0; t < tiles; t += gridDim.y) {
                const td::Tile tl = td::tile_of(o, (uint32_t)t, p);
                __syncthreads();                      // (the window before this one has been read)
                for (uint32_t q = tid; q < tl.W; q += td::kTileOutputs) w[q] = td::window_at(s, o, tl, q, p.T, k.pool, hist);
                __syncthreads();
                if (tid < tl.n) dk.dpool[o.off + t * td::kTileOutputs + tid] = td::tile_output(w, dk.taps_t, p, tl, tid);
            }
        }
    }
}

template <typename SampleT>
__global__ __launch_bounds__(256) void tone_delivery_history_kernel(ToneAudioCall k, ToneDeliveryCall dk, const SampleT *__restrict__ x, uint32_t n_rows,
                                                                    int time_major)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k.n_channels) return;
    const tn::Desc d = k.desc[c];
    const tn::Cap cap = k.cap[c];
    const SampleT *xc = time_major ? x + c : x + (size_t)c * n_rows;
    td::history_step(d, cap, k.N, dk.params.T, xc, time_major ? (size_t)k.n_channels : (size_t)1, dk.hist + (size_t)c * (dk.params.T - 1), 1,
                     dk.a_next + c);
}

template <typename SampleT>
hipError_t launch_history(const ToneAudioCall &k, const ToneDeliveryCall &dk, const SampleT *x, size_t n_rows, int layout, hipStream_t stream)
{
    hipLaunchKernelGGL(tone_delivery_history_kernel<SampleT>, dim3((k.n_channels + 255) / 256), dim3(256), 0, stream, k, dk, x, (uint32_t)n_rows,
                       layout == SAME_LAYOUT_TIME_MAJOR ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

hipError_t tone_delivery_launch(const ToneAudioCall &k, const ToneDeliveryCall &dk, hipStream_t stream)
{
    hipLaunchKernelGGL(tone_delivery_place_kernel, dim3(1), dim3(kPlaceThreads), 0, stream, k, dk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t groups = (k.n_channels + kGroup - 1) / kGroup;
    const uint32_t gy = dk.max_tiles < kMaxGridY ? (dk.max_tiles ? dk.max_tiles : 1) : kMaxGridY;
    hipLaunchKernelGGL(tone_delivery_decimate_kernel, dim3(groups, gy), dim3(td::kTileOutputs), 0, stream, k, dk);
    return hipGetLastError();
}

hipError_t tone_delivery_launch_history(const ToneAudioCall &k, const ToneDeliveryCall &dk, const float *x, size_t n_rows, int layout, hipStream_t stream)
{
    return launch_history(k, dk, x, n_rows, layout, stream);
}

hipError_t tone_delivery_launch_history(const ToneAudioCall &k, const ToneDeliveryCall &dk, const int16_t *x, size_t n_rows, int layout, hipStream_t stream)
{
    return launch_history(k, dk, x, n_rows, layout, stream);
}

}  // namespace same
