// same_tone_audio.hip -- the kernels of tone-alert audio (include/same_tone_audio.h).  The decisions are
// same_tone_audio_dev.h's (one text for g++ and the device); same_tones.hip queues these behind its block kernel, in place of
// tones_sm_kernel, when a handle's capture is on.
//   tone_audio_sm_kernel     lane = channel: both tone state machines and the capture state over the call's qualify bits.  It
//                            writes the channel's events, its chunk records (spans of captured rows, offsets still counted
//                            inside the channel), its captured-row count, and per wavefront -- 64 adjacent channels -- whether
//                            anyone captures.
//   tone_audio_place_kernel  one workgroup: an exclusive prefix sum over the channels' counts, 1024 channels per round with the
//                            total carried along (any C), then every channel's spans get their room in the pool
//                            (tn::span_place: channel order, then stream order, cut where the pool ends).  No atomics.
//   tone_audio_copy_tm_kernel  time-major.  A group whose flag is clear exits at once.  Otherwise a wavefront takes tiles of
//                            64 channels x 64 rows: no two spans of a channel lie closer than a block (>= 320 rows), so a
//                            tile meets at most one span per channel; tiles no lane has rows in are skipped.  Loaded with the
//                            lanes along channels (one 256-byte row segment per instruction, 128 for int16, lanes outside
//                            their span masked: rows at or beyond counts[c] are never loaded), staged through LDS in rows
//                            padded to 65 words, stored with the lanes along time: each channel's chunk is written in
//                            contiguous segments of up to 256 bytes.  A tile in which at most kSparse channels have rows
//                            skips LDS: a row-per-lane gather per channel (a row load would fetch one sample each).
//   tone_audio_copy_cm_kernel  channel-major: lanes along time on both sides, no LDS; a workgroup takes one slice of the rows of
//                            one group's channels.
#include <hip/hip_runtime.h>

#include "../../include/same_rx.h"
#include "same_tone_audio_kernels.h"

namespace same {
namespace {

constexpr uint32_t kTile = 64, kTilePitch = kTile + 1;
constexpr uint32_t kPlaceThreads = 1024;
constexpr uint32_t kCmThreads = 256;
constexpr uint32_t kTmMaxGridY = 128;       // time-major: workgroups per group of channels, each takes every 128th tile
constexpr uint32_t kCmMaxSlices = 1024;
constexpr uint32_t kSparse = 8;             // time-major: up to this many capturing channels in a tile are gathered one by one

__global__ __launch_bounds__(256) void tone_audio_sm_kernel(ToneAudioCall k)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const bool valid = c < k.n_channels;
    uint64_t total = 0;
    if (valid) {
        const tn::Desc d = k.desc[c];
        tn::Sm s[2] = {k.sm[2 * (size_t)c], k.sm[2 * (size_t)c + 1]};
        tn::Cap cap = k.cap[c];
        uint32_t n_ev = 0, n_spans = 0;
        tn::Span *spans = (tn::Span *)(k.out + cap_spans_offset(k.n_channels)) + k.span_off[c];
        total = tn::run_capture(d, k.N, c, k.n_channels, k.qual, s, cap, k.params, k.ev, &n_ev, spans, &n_spans);
        k.sm[2 * (size_t)c] = s[0];
        k.sm[2 * (size_t)c + 1] = s[1];
        k.cap[c] = cap;
        k.ev_counts[c] = n_ev;
        ((uint32_t *)(k.out + kCapHeaderBytes))[c] = n_spans;
        k.counts[c] = total;
    }
    // (a wavefront is 64 adjacent channels: blocks of 256 start at multiples of 64)
    const unsigned long long any = __ballot(valid && total != 0);
    if ((threadIdx.x & 63u) == 0 && valid) k.flags[c >> 6] = any != 0 ? 1u : 0u;
}

__global__ __launch_bounds__(kPlaceThreads) void tone_audio_place_kernel(ToneAudioCall k)
{
    __shared__ uint64_t wave_sum[kPlaceThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t *n_spans = (const uint32_t *)(k.out + kCapHeaderBytes);
    tn::Span *spans = (tn::Span *)(k.out + cap_spans_offset(k.n_channels));
    uint64_t carry = 0;                               // captured rows of the channels before this round, the same in every thread
    for (uint32_t c0 = 0; c0 < k.n_channels; c0 += kPlaceThreads) {
        const uint32_t c = c0 + threadIdx.x;
        const bool valid = c < k.n_channels;          // (c0 + 1023 < 2^32: the library's batches end far below)
        const uint64_t v = valid ? k.counts[c] : 0;
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
        if (valid) {
            const uint64_t base = carry + before + (incl - v);
            const uint32_t n = n_spans[c];
            for (uint32_t i = 0; i < n; ++i) tn::span_place(spans[k.span_off[c] + i], base, k.pool_cap);
        }
        carry += round;
        __syncthreads();                              // (wave_sum is written again by the next round)
    }
    if (threadIdx.x == 0) {
        uint64_t *header = (uint64_t *)k.out;
        header[0] = carry;
        header[1] = carry < k.pool_cap ? carry : k.pool_cap;
    }
}

template <typename SampleT>
__global__ __launch_bounds__(64) void tone_audio_copy_tm_kernel(ToneAudioCall k, const SampleT *__restrict__ x, uint32_t n_rows)
{
    __shared__ float tile[kTile * kTilePitch];
    if (!k.flags[blockIdx.x]) return;
    const uint32_t lane = threadIdx.x, C = k.n_channels;
    const uint32_t c = blockIdx.x * kTile + lane;
    const bool valid = c < C;
    const uint32_t n_spans = valid ? ((const uint32_t *)(k.out + kCapHeaderBytes))[c] : 0;
    const tn::Span *spans = (const tn::Span *)(k.out + cap_spans_offset(C)) + (valid ? k.span_off[c] : 0);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_rows + kTile - 1) / kTile);
    for (uint32_t ti = blockIdx.y; ti < n_tiles; ti += gridDim.y) {
        const uint64_t t0 = (uint64_t)ti * kTile, t1 = t0 + kTile;
        // the rows [lo, hi) of this tile that the channel's span has room for, and where row lo goes
        uint32_t lo = 0, hi = 0;
        uint64_t dst = 0;
        for (uint32_t i = 0; i < n_spans; ++i) {
            const uint64_t a = spans[i].row0, b = a + spans[i].n;
            const uint64_t o_lo = a > t0 ? a : t0, o_hi = b < t1 ? b : t1;
            if (o_lo < o_hi) { lo = (uint32_t)o_lo; hi = (uint32_t)o_hi; dst = spans[i].off + (o_lo - a); }
        }
        unsigned long long active = __ballot(lo < hi);
        if (!active) continue;                        // (one wavefront per workgroup: the same in every thread)
        if (__popcll(active) <= (int)kSparse) {
            // few channels of the group capture here: a row-per-lane gather of each, one load and one store per channel, in
            // place of 64 row loads that would fetch one sample each
            const uint32_t g_lo = (uint32_t)dst, g_hi = (uint32_t)(dst >> 32);
            while (active) {
                const int ch = __builtin_ctzll(active);
                active &= active - 1;
                const uint32_t c_lo = (uint32_t)__builtin_amdgcn_readlane((int)lo, ch), c_hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, ch);
                const uint64_t c_dst = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g_lo, ch) |
                                       ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g_hi, ch) << 32);
                const uint64_t t = t0 + lane;
                if (t >= c_lo && t < c_hi) k.pool[c_dst + (t - c_lo)] = (float)x[(size_t)t * C + (blockIdx.x * kTile + (uint32_t)ch)];
            }
            continue;
        }
        __syncthreads();                              // (the tile before this one has been stored)
#pragma unroll 16
        for (uint32_t r = 0; r < kTile; ++r) {
            const uint64_t t = t0 + r;
            float v = 0.0f;
            if (t >= lo && t < hi) v = (float)x[(size_t)t * C + c];
            tile[r * kTilePitch + lane] = v;
        }
        __syncthreads();
        const uint32_t dst_lo = (uint32_t)dst, dst_hi = (uint32_t)(dst >> 32);
        for (uint32_t ch = 0; ch < kTile; ++ch) {
            const uint32_t c_lo = (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)ch), c_hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)ch);
            if (c_lo >= c_hi) continue;
            const uint64_t c_dst = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)dst_lo, (int)ch) |
                                   ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)dst_hi, (int)ch) << 32);
            const uint64_t t = t0 + lane;
            if (t >= c_lo && t < c_hi) k.pool[c_dst + (t - c_lo)] = tile[lane * kTilePitch + ch];
        }
    }
}

template <typename SampleT>
__global__ __launch_bounds__(kCmThreads) void tone_audio_copy_cm_kernel(ToneAudioCall k, const SampleT *__restrict__ x, uint32_t n_rows, uint32_t slice)
{
    if (!k.flags[blockIdx.x]) return;
    const uint32_t C = k.n_channels;
    const uint32_t *n_spans = (const uint32_t *)(k.out + kCapHeaderBytes);
    const tn::Span *spans = (const tn::Span *)(k.out + cap_spans_offset(C));
    const uint64_t t0 = (uint64_t)blockIdx.y * slice, t1 = t0 + slice;
    for (uint32_t ch = 0; ch < kTile; ++ch) {
        const uint32_t c = blockIdx.x * kTile + ch;
        if (c >= C) break;
        const uint32_t n = n_spans[c];
        const tn::Span *mine = spans + k.span_off[c];
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t a = mine[i].row0, b = a + mine[i].n, off = mine[i].off;
            const uint64_t lo = a > t0 ? a : t0, hi = b < t1 ? b : t1;
            const SampleT *src = x + (size_t)c * n_rows;
            for (uint64_t t = lo + threadIdx.x; t < hi; t += kCmThreads) k.pool[off + (t - a)] = (float)src[t];
        }
    }
}

template <typename SampleT>
hipError_t launch_copy(const ToneAudioCall &k, const SampleT *x, size_t n_rows, int layout, hipStream_t stream)
{
    const uint32_t groups = (k.n_channels + kTile - 1) / kTile;
    if (layout == SAME_LAYOUT_TIME_MAJOR) {
        const uint64_t tiles = ((uint64_t)n_rows + kTile - 1) / kTile;
        hipLaunchKernelGGL(tone_audio_copy_tm_kernel<SampleT>, dim3(groups, (uint32_t)(tiles < kTmMaxGridY ? tiles : kTmMaxGridY)), dim3(64), 0, stream,
                           k, x, (uint32_t)n_rows);
    } else {
        // slices of at least 2048 rows, a multiple of the workgroup, at most kCmMaxSlices of them
        uint64_t slice = ((uint64_t)n_rows + kCmMaxSlices - 1) / kCmMaxSlices;
        if (slice < 2048) slice = 2048;
        slice = (slice + kCmThreads - 1) / kCmThreads * kCmThreads;
        const uint64_t gy = ((uint64_t)n_rows + slice - 1) / slice;
        hipLaunchKernelGGL(tone_audio_copy_cm_kernel<SampleT>, dim3(groups, (uint32_t)gy), dim3(kCmThreads), 0, stream, k, x, (uint32_t)n_rows,
                           (uint32_t)slice);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t tone_audio_launch_sm(const ToneAudioCall &k, hipStream_t stream)
{
    hipLaunchKernelGGL(tone_audio_sm_kernel, dim3((k.n_channels + 255) / 256), dim3(256), 0, stream, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tone_audio_place_kernel, dim3(1), dim3(kPlaceThreads), 0, stream, k);
    return hipGetLastError();
}

hipError_t tone_audio_launch_copy(const ToneAudioCall &k, const float *x, size_t n_rows, int layout, hipStream_t stream)
{
    return launch_copy(k, x, n_rows, layout, stream);
}

hipError_t tone_audio_launch_copy(const ToneAudioCall &k, const int16_t *x, size_t n_rows, int layout, hipStream_t stream)
{
    return launch_copy(k, x, n_rows, layout, stream);
}

}  // namespace same
