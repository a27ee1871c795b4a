// same_resample.hip -- the mixed-rate resampler of include/same_resample.h: its kernels and its C ABI.  The arithmetic is
// same_resample_dev.h's (one text for g++ and the device), the clocks and tap tables same_resample_plan.h's (host only).
//
// resample_kernel: lane = channel.  A wavefront takes 64 adjacent channels through kRowsPerWave output rows, so its reads of
// x[row * C + c] and its writes of y[n * C + c] are rows of consecutive floats wherever neighbouring lanes share a rate (lanes
// of different rates walk the source at different paces: DESIGN.md 4.11 has the traffic).  No LDS, no barrier, no atomics, no
// word passed between wavefronts or workgroups: a FIR has nothing to hand over, so nothing can wait.
// history_kernel, behind it on the same stream: each channel's last T - 1 source samples into its column of the history, for
// the taps of the next call that reach back before that call's first row.
// clear_kernel, in front of both when a channel was reset: zeroes the reset channels' columns.
// source_resample_kernel and source_history_kernel, further down, are the per-source calls' (every channel from a buffer of its
// own): the same arithmetic, clocks and history with a wavefront on one channel and its lanes along the output rows.
//
// A call's per-channel descriptors (rs::Desc: counts and clocks before the call, 32 bytes a channel) are written into one of
// kSlots pinned host buffers and copied to the device on the call's stream in front of its kernels; a slot is reused only once
// the event recorded behind the call's kernels has passed.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "../../include/same_resample.h"
#include "same_hipmem.h"
#include "same_resample_plan.h"

namespace same {
namespace {

constexpr uint32_t kRowsPerWave = 64, kWavesPerBlock = 4, kRowsPerBlock = kRowsPerWave * kWavesPerBlock;
constexpr uint32_t kMaxGridY = 65535;
constexpr int kSlots = 3;

template <typename SampleT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void resample_kernel(const rs::Desc *__restrict__ desc, const rs::Ratio *__restrict__ ratios,
                                                                       const float *__restrict__ taps, const SampleT *__restrict__ x,
                                                                       const float *__restrict__ hist, float *__restrict__ y,
                                                                       uint32_t n_channels, uint32_t n_row_blocks)
{
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_channels) return;
    const rs::Desc d = desc[c];
    const rs::Ratio r = ratios[d.ratio];
    for (uint32_t rb = blockIdx.y; rb < n_row_blocks; rb += gridDim.y) {
        const uint32_t row0 = rb * kRowsPerBlock + threadIdx.y * kRowsPerWave;
        if (row0 >= d.out_count) return;          // this and every later block of the lane lies behind its outputs
        const uint32_t left = d.out_count - row0;
        rs::lane_rows(d, r, taps, x + c, n_channels, hist + c, n_channels, y + c, n_channels, row0,
                      row0 + (left < kRowsPerWave ? left : kRowsPerWave));
    }
}

template <typename SampleT>
__global__ __launch_bounds__(256) void history_kernel(const rs::Desc *__restrict__ desc, const rs::Ratio *__restrict__ ratios,
                                                      const SampleT *__restrict__ x, float *__restrict__ hist, uint32_t n_channels)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_channels) return;
    const rs::Desc d = desc[c];
    const uint32_t T = ratios[d.ratio].T;
    if (d.in_count == 0 || T == 1) return;
    rs::update_history(hist + c, n_channels, T, x + c, n_channels, d.in_count);
}

__global__ __launch_bounds__(256) void clear_kernel(const rs::Desc *__restrict__ desc, float *__restrict__ hist, uint32_t n_channels)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_channels || !desc[c].clear) return;
    for (uint32_t i = 0; i < rs::kHistRows; ++i) hist[(size_t)i * n_channels + c] = 0.0f;
}

// ---- per-source calls (same_resampler_process_device_sources): channel c's samples are src[c][0 .. in_count).
//
// source_resample_kernel: a workgroup of kSrcWaves wavefronts owns a tile of kTileCh adjacent channels x kTileRows output rows.
// First each wavefront takes kTileCh / kSrcWaves of the tile's channels in turn with lane = output row: the lanes read one
// contiguous stretch of the channel's buffer, and the descriptor, ratio and source pointer are wave-uniform.  The results go
// to an LDS tile [row][channel], padded to kTilePitch so that neither the column writes nor the row reads meet on a bank.
// Behind one barrier each wavefront writes kTileRows / kSrcWaves rows of the tile with lane = channel: 256-byte rows of y,
// each lane masked by its own out_count.  Whether a tile is run at all is decided by tile_out alone, the largest out_count of
// the tile's channels, which every wavefront computes from the same 64 descriptors: it is the same in every thread of the
// workgroup, so every wavefront meets the same barriers whatever its own channels' counts are.  No wavefront leaves in front
// of a barrier; there is no other synchronisation.
// Lanes differ in phase, so the taps of one tap step are 64 scattered words of the [j][p] table.  A tile whose 64 channels share
// one ratio (a producer that groups equal rates) first copies that table into LDS, up to kMaxLdsTaps floats, and reads it there.
constexpr uint32_t kTileCh = 64, kTileRows = 64, kTilePitch = kTileCh + 1, kSrcWaves = 4;
constexpr uint32_t kMaxLdsTaps = 441 * 24;        // 41 KB: 32 kHz -> 22.05 kHz, the largest table of the common rates (96 kHz: 147 * 70)

template <typename SampleT>
__global__ __launch_bounds__(64 * kSrcWaves) void source_resample_kernel(const rs::Desc *__restrict__ desc, const rs::Ratio *__restrict__ ratios,
                                                                         const float *__restrict__ taps_t, const SampleT *const *__restrict__ src,
                                                                         const float *__restrict__ hist, float *__restrict__ y,
                                                                         uint32_t n_channels, uint32_t n_row_tiles, uint32_t lds_taps)
{
    __shared__ float tile[kTileRows * kTilePitch];
    extern __shared__ float table[];                                           // lds_taps floats
    const uint32_t lane = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const uint32_t c0 = blockIdx.x * kTileCh;
    const uint32_t my_c = c0 + lane;                                           // the write-out's lane = channel
    const uint32_t my_out = my_c < n_channels ? desc[my_c].out_count : 0;
    const uint32_t my_ratio = desc[my_c < n_channels ? my_c : c0].ratio;       // (c0 < n_channels: the grid has no empty tile)
    uint32_t tile_out = my_out, ratio_lo = my_ratio, ratio_hi = my_ratio;
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)tile_out, m, 64);
        const uint32_t lo = (uint32_t)__shfl_xor((int)ratio_lo, m, 64), hi = (uint32_t)__shfl_xor((int)ratio_hi, m, 64);
        tile_out = o > tile_out ? o : tile_out;
        ratio_lo = lo < ratio_lo ? lo : ratio_lo;
        ratio_hi = hi > ratio_hi ? hi : ratio_hi;
    }
    // A tile whose channels share one ratio reads its [j][p] table from LDS when the launch gave it room.  Like tile_out the
    // decision comes from the tile's 64 descriptors alone, so it is the same in every thread of the workgroup.
    rs::Ratio one = ratios[ratio_lo];
    const bool staged = ratio_lo == ratio_hi && one.T > 1 && one.T * one.L <= lds_taps && blockIdx.y * kTileRows < tile_out;
    if (staged) {
        for (uint32_t e = threadIdx.y * 64 + lane; e < one.T * one.L; e += 64 * kSrcWaves) table[e] = taps_t[one.tap_off + e];
        one.tap_off = 0;
        __syncthreads();
    }
    for (uint32_t rt = blockIdx.y; rt < n_row_tiles; rt += gridDim.y) {
        const uint32_t row0 = rt * kTileRows;
        if (row0 >= tile_out) break;              // workgroup-uniform: this and every later tile lies behind all 64 channels' outputs
        for (uint32_t q = 0; q < kTileCh / kSrcWaves; ++q) {
            const uint32_t ch = wave * (kTileCh / kSrcWaves) + q, c = c0 + ch;
            if (c >= n_channels) break;
            const rs::Desc d = desc[c];
            if (row0 >= d.out_count) continue;
            const uint32_t left = d.out_count - row0, row1 = row0 + (left < kTileRows ? left : kTileRows);
            if (staged) rs::source_rows(d, one, table, src[c], hist + c, n_channels, tile + ch, kTilePitch, row0, row1, lane, 64u);
            else rs::source_rows(d, ratios[d.ratio], taps_t, src[c], hist + c, n_channels, tile + ch, kTilePitch, row0, row1, lane, 64u);
        }
        __syncthreads();
        for (uint32_t q = 0; q < kTileRows / kSrcWaves; ++q) {
            const uint32_t r = wave * (kTileRows / kSrcWaves) + q;
            if (row0 + r < my_out) y[(size_t)(row0 + r) * n_channels + my_c] = tile[r * kTilePitch + lane];
        }
        __syncthreads();                          // (the next tile of this workgroup overwrites the LDS tile)
    }
}

template <typename SampleT>
__global__ __launch_bounds__(256) void source_history_kernel(const rs::Desc *__restrict__ desc, const rs::Ratio *__restrict__ ratios,
                                                             const SampleT *const *__restrict__ src, float *__restrict__ hist, uint32_t n_channels)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_channels) return;
    const rs::Desc d = desc[c];
    rs::update_history_source(hist + c, n_channels, ratios[d.ratio].T, src[c], d.in_count);
}

thread_local std::string g_resampler_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_resampler_error = buf;
    return code;
}

#define RS_HIP_TRY(expr)                                                                                            \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) return fail(SAME_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

}  // namespace
}  // namespace same

struct same_resampler {
    same::ResamplePlan plan;
    int device = 0;
    same::DevBuf<same::rs::Ratio> d_ratios;      // rs::kMaxRatios entries, appended to
    same::DevBuf<float> d_taps;
    same::DevBuf<float> d_taps_t;                // the tables stored [j][p], for per-source calls
    uint32_t ratios_on_device = 0;
    same::DevBuf<same::rs::Desc> d_desc;         // the descriptors of the call the stream is at
    same::DevBuf<float> d_hist;                  // [rs::kHistRows x C]: channel c's last T - 1 source samples, oldest first
    same::DevBuf<const void *> d_src;            // the source pointers of the per-source call the stream is at
    struct Slot { same::PinnedBuf<same::rs::Desc> desc; same::PinnedBuf<const void *> src; same::Event done; bool in_flight = false; };
    Slot slot[same::kSlots];
    int next_slot = 0;
    std::vector<uint32_t> out_tmp;
};

namespace same {
namespace {

int wait_slot(same_resampler::Slot &s)
{
    if (s.in_flight) { RS_HIP_TRY(hipEventSynchronize(s.done)); s.in_flight = false; }
    return SAME_OK;
}

// the tap tables and ratios the plan has and the device has not.  Kernels in flight read the old tables: they are waited for
// before a table moves (a handle sees at most rs::kMaxRatios new ratios in its life).
int upload_tables(same_resampler *h)
{
    if (h->ratios_on_device == h->plan.ratios.size()) return SAME_OK;
    for (same_resampler::Slot &s : h->slot) { const int rc = wait_slot(s); if (rc) return rc; }
    RS_HIP_TRY(h->d_ratios.ensure(rs::kMaxRatios));
    RS_HIP_TRY(h->d_taps.ensure(h->plan.taps.size()));
    RS_HIP_TRY(h->d_taps_t.ensure(h->plan.taps_t.size()));
    RS_HIP_TRY(hipMemcpy(h->d_ratios.get(), h->plan.ratios.data(), h->plan.ratios.size() * sizeof(rs::Ratio), hipMemcpyHostToDevice));
    RS_HIP_TRY(hipMemcpy(h->d_taps.get(), h->plan.taps.data(), h->plan.taps.size() * sizeof(float), hipMemcpyHostToDevice));
    RS_HIP_TRY(hipMemcpy(h->d_taps_t.get(), h->plan.taps_t.data(), h->plan.taps_t.size() * sizeof(float), hipMemcpyHostToDevice));
    h->ratios_on_device = (uint32_t)h->plan.ratios.size();
    return SAME_OK;
}

template <typename SampleT>
int process(same_resampler *h, const SampleT *d_x, size_t n_rows, const uint32_t *in_counts, float *d_y, size_t out_rows,
            uint32_t *out_counts, void *hip_stream)
{
    if (!h || !in_counts || !out_counts) return fail(SAME_EINVAL, "null argument");
    const uint32_t C = h->plan.n_channels();
    uint32_t max_out = 0, max_in = 0;
    for (uint32_t c = 0; c < C; ++c) {
        if (in_counts[c] > n_rows)
            return fail(SAME_EINVAL, "in_counts[%u] = %u exceeds n_rows = %zu; nothing was consumed", c, in_counts[c], n_rows);
        if (in_counts[c] > max_in) max_in = in_counts[c];
    }
    if (h->plan.out_counts(in_counts, n_rows, h->out_tmp.data(), &max_out))
        return fail(SAME_EINVAL, "a channel's output count exceeds 2^32 - 1; nothing was consumed");
    if (max_out > out_rows)
        return fail(SAME_EINVAL, "out_rows = %zu, the call makes up to %u rows; nothing was consumed", out_rows, max_out);
    if (max_in == 0) {
        for (uint32_t c = 0; c < C; ++c) out_counts[c] = 0;
        return SAME_OK;
    }
    if (!d_x || (!d_y && max_out)) return fail(SAME_EINVAL, "null argument");
    RS_HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    same_resampler::Slot &s = h->slot[h->next_slot];
    int rc = wait_slot(s);
    if (rc) return rc;
    const bool any_clear = h->plan.describe(in_counts, h->out_tmp.data(), s.desc.get());
    RS_HIP_TRY(hipMemcpyAsync(h->d_desc.get(), s.desc.get(), (size_t)C * sizeof(rs::Desc), hipMemcpyHostToDevice, stream));
    const uint32_t lane_blocks = (C + 255) / 256;
    if (any_clear) {
        hipLaunchKernelGGL(clear_kernel, dim3(lane_blocks), dim3(256), 0, stream, h->d_desc.get(), h->d_hist.get(), C);
        RS_HIP_TRY(hipGetLastError());
    }
    if (max_out) {
        const uint32_t n_row_blocks = (uint32_t)(((uint64_t)max_out + kRowsPerBlock - 1) / kRowsPerBlock);
        hipLaunchKernelGGL(resample_kernel<SampleT>, dim3((C + 63) / 64, n_row_blocks < kMaxGridY ? n_row_blocks : kMaxGridY),
                           dim3(64, kWavesPerBlock), 0, stream, h->d_desc.get(), h->d_ratios.get(), h->d_taps.get(), d_x, h->d_hist.get(),
                           d_y, C, n_row_blocks);
        RS_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(history_kernel<SampleT>, dim3(lane_blocks), dim3(256), 0, stream, h->d_desc.get(), h->d_ratios.get(), d_x,
                       h->d_hist.get(), C);
    RS_HIP_TRY(hipGetLastError());
    RS_HIP_TRY(hipEventRecord(s.done, stream));
    s.in_flight = true;
    h->next_slot = (h->next_slot + 1) % kSlots;
    h->plan.commit(in_counts, h->out_tmp.data());
    for (uint32_t c = 0; c < C; ++c) out_counts[c] = h->out_tmp[c];
    return SAME_OK;
}

// A per-source call: the time-major call's slots, descriptors, clear and commit; the source pointers travel in the slot beside
// the descriptors and the kernels read their device copy.
template <typename SampleT>
int process_sources(same_resampler *h, const SampleT *const *d_src, const uint32_t *in_counts, float *d_y, size_t out_rows,
                    uint32_t *out_counts, void *hip_stream)
{
    if (!h || !d_src || !in_counts || !out_counts) return fail(SAME_EINVAL, "null argument");
    const uint32_t C = h->plan.n_channels();
    uint32_t max_out = 0, max_in = 0;
    for (uint32_t c = 0; c < C; ++c) {
        if (in_counts[c] == 0) continue;
        if (!d_src[c]) return fail(SAME_EINVAL, "d_src[%u] is null with in_counts[%u] = %u; nothing was consumed", c, c, in_counts[c]);
        if ((uintptr_t)d_src[c] % sizeof(SampleT))
            return fail(SAME_EINVAL, "d_src[%u] is not aligned to %zu bytes; nothing was consumed", c, sizeof(SampleT));
        if (in_counts[c] > max_in) max_in = in_counts[c];
    }
    if (h->plan.out_counts(in_counts, 0xffffffffu, h->out_tmp.data(), &max_out))
        return fail(SAME_EINVAL, "a channel's output count exceeds 2^32 - 1; nothing was consumed");
    if (max_out > out_rows)
        return fail(SAME_EINVAL, "out_rows = %zu, the call makes up to %u rows; nothing was consumed", out_rows, max_out);
    if (max_in == 0) {
        for (uint32_t c = 0; c < C; ++c) out_counts[c] = 0;
        return SAME_OK;
    }
    if (!d_y && max_out) return fail(SAME_EINVAL, "null argument");
    RS_HIP_TRY(hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    same_resampler::Slot &s = h->slot[h->next_slot];
    int rc = wait_slot(s);
    if (rc) return rc;
    const bool any_clear = h->plan.describe(in_counts, h->out_tmp.data(), s.desc.get());
    for (uint32_t c = 0; c < C; ++c) s.src[c] = in_counts[c] ? d_src[c] : nullptr;
    RS_HIP_TRY(hipMemcpyAsync(h->d_desc.get(), s.desc.get(), (size_t)C * sizeof(rs::Desc), hipMemcpyHostToDevice, stream));
    RS_HIP_TRY(hipMemcpyAsync(h->d_src.get(), s.src.get(), (size_t)C * sizeof(const void *), hipMemcpyHostToDevice, stream));
    const SampleT *const *src = (const SampleT *const *)h->d_src.get();
    const uint32_t lane_blocks = (C + 255) / 256;
    if (any_clear) {
        hipLaunchKernelGGL(clear_kernel, dim3(lane_blocks), dim3(256), 0, stream, h->d_desc.get(), h->d_hist.get(), C);
        RS_HIP_TRY(hipGetLastError());
    }
    if (max_out) {
        const uint32_t n_row_tiles = (uint32_t)(((uint64_t)max_out + kTileRows - 1) / kTileRows);
        // room in LDS for the largest table of a tile whose channels share one ratio (none: no room, and more workgroups per CU)
        uint32_t lds_taps = 0;
        for (uint32_t c0 = 0; c0 < C; c0 += kTileCh) {
            const uint32_t end = c0 + kTileCh < C ? c0 + kTileCh : C;
            uint32_t c = c0 + 1;
            while (c < end && h->plan.chan_ratio[c] == h->plan.chan_ratio[c0]) ++c;
            const rs::Ratio &r = h->plan.ratios[h->plan.chan_ratio[c0]];
            if (c == end && r.T > 1 && r.T * r.L <= kMaxLdsTaps && r.T * r.L > lds_taps) lds_taps = r.T * r.L;
        }
        hipLaunchKernelGGL(source_resample_kernel<SampleT>, dim3((C + kTileCh - 1) / kTileCh, n_row_tiles < kMaxGridY ? n_row_tiles : kMaxGridY),
                           dim3(64, kSrcWaves), lds_taps * sizeof(float), stream, h->d_desc.get(), h->d_ratios.get(), h->d_taps_t.get(), src,
                           h->d_hist.get(), d_y, C, n_row_tiles, lds_taps);
        RS_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(source_history_kernel<SampleT>, dim3(lane_blocks), dim3(256), 0, stream, h->d_desc.get(), h->d_ratios.get(), src,
                       h->d_hist.get(), C);
    RS_HIP_TRY(hipGetLastError());
    RS_HIP_TRY(hipEventRecord(s.done, stream));
    s.in_flight = true;
    h->next_slot = (h->next_slot + 1) % kSlots;
    h->plan.commit(in_counts, h->out_tmp.data());
    for (uint32_t c = 0; c < C; ++c) out_counts[c] = h->out_tmp[c];
    return SAME_OK;
}

}  // namespace
}  // namespace same

using namespace same;

extern "C" {

const char *same_resampler_last_error(void) { return g_resampler_error.c_str(); }

int same_resampler_new(uint32_t n_channels, const uint32_t *in_rates, uint32_t out_rate, int device, same_resampler **out)
{
    if (!in_rates || !out || n_channels == 0) return fail(SAME_EINVAL, "null in_rates/out or zero channels");
    *out = nullptr;
    same_resampler *h = new (std::nothrow) same_resampler;
    if (!h) return fail(SAME_ENOMEM, "out of memory");
    // (the plan first: a refused rate is refused with or without a device)
    int rc = h->plan.init(n_channels, in_rates, out_rate);
    if (rc) {
        delete h;
        return rc == SAME_ERATE ? fail(rc, "a source rate needs more than %u phases or %u taps per phase for %u Hz", rs::kMaxL, rs::kMaxT, out_rate)
                                : fail(rc, "a zero rate, or more than %u distinct ratios in one handle", rs::kMaxRatios);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { delete h; return fail(SAME_ENODEVICE, "no HIP device visible (this library has no CPU path)"); }
    if (device < 0 || device >= ndev) { delete h; return fail(SAME_ENODEVICE, "device %d out of range (%d visible)", device, ndev); }
    h->device = device;
    h->out_tmp.assign(n_channels, 0);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = h->d_desc.ensure(n_channels);
    if (e == hipSuccess) e = h->d_src.ensure(n_channels);
    if (e == hipSuccess) e = h->d_hist.ensure((size_t)rs::kHistRows * n_channels);     // (zeroed by the first call's clear_kernel)
    for (same_resampler::Slot &s : h->slot) {
        if (e == hipSuccess) e = s.desc.ensure(n_channels);
        if (e == hipSuccess) e = s.src.ensure(n_channels);
        if (e == hipSuccess) e = s.done.ensure();
    }
    if (e != hipSuccess) {
        delete h;
        return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the resampler failed: %s", hipGetErrorString(e));
    }
    rc = upload_tables(h);
    if (rc) { delete h; return rc; }
    *out = h;
    return SAME_OK;
}

void same_resampler_free(same_resampler *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    // (the kernels in flight read the handle's buffers)
    for (same_resampler::Slot &s : h->slot) (void)wait_slot(s);
    delete h;
}

uint32_t same_resampler_n_channels(const same_resampler *h) { return h ? h->plan.n_channels() : 0; }
uint32_t same_resampler_out_rate(const same_resampler *h) { return h ? h->plan.out_rate : 0; }

int same_resampler_plan(const same_resampler *h, uint32_t channel, uint32_t *L, uint32_t *M, uint32_t *T)
{
    if (!h || channel >= h->plan.n_channels()) return fail(SAME_EINVAL, "null handle or channel out of range");
    const rs::Ratio &r = h->plan.ratio(channel);
    if (L) *L = r.L;
    if (M) *M = r.M;
    if (T) *T = r.T;
    return SAME_OK;
}

int same_resampler_taps(const same_resampler *h, uint32_t channel, float *out, size_t cap, size_t *n)
{
    if (!h || !n || channel >= h->plan.n_channels()) return fail(SAME_EINVAL, "null argument or channel out of range");
    const rs::Ratio &r = h->plan.ratio(channel);
    *n = (size_t)r.T * r.L;
    if (!out || cap < *n) return fail(SAME_EINVAL, "the channel has %zu taps, room for %zu", *n, out ? cap : (size_t)0);
    for (size_t i = 0; i < *n; ++i) out[i] = h->plan.taps[r.tap_off + i];
    return SAME_OK;
}

double same_resampler_delay(const same_resampler *h, uint32_t channel)
{
    return h && channel < h->plan.n_channels() ? h->plan.delay(channel) : -1.0;
}

int same_resampler_out_counts(const same_resampler *h, const uint32_t *in_counts, uint32_t *out_counts, uint32_t *max_out)
{
    if (!h || !in_counts || !out_counts || !max_out) return fail(SAME_EINVAL, "null argument");
    if (h->plan.out_counts(in_counts, 0xffffffffu, out_counts, max_out))
        return fail(SAME_EINVAL, "a channel's output count exceeds 2^32 - 1");
    return SAME_OK;
}

int same_resampler_process_device(same_resampler *h, const float *d_x, size_t n_rows, const uint32_t *in_counts, float *d_y,
                                  size_t out_rows, uint32_t *out_counts, void *hip_stream)
{
    return process(h, d_x, n_rows, in_counts, d_y, out_rows, out_counts, hip_stream);
}

int same_resampler_process_device_i16(same_resampler *h, const int16_t *d_x, size_t n_rows, const uint32_t *in_counts, float *d_y,
                                      size_t out_rows, uint32_t *out_counts, void *hip_stream)
{
    return process(h, d_x, n_rows, in_counts, d_y, out_rows, out_counts, hip_stream);
}

int same_resampler_process_device_sources(same_resampler *h, const float *const *d_src, const uint32_t *in_counts, float *d_y,
                                          size_t out_rows, uint32_t *out_counts, void *hip_stream)
{
    return process_sources(h, d_src, in_counts, d_y, out_rows, out_counts, hip_stream);
}

int same_resampler_process_device_sources_i16(same_resampler *h, const int16_t *const *d_src, const uint32_t *in_counts, float *d_y,
                                              size_t out_rows, uint32_t *out_counts, void *hip_stream)
{
    return process_sources(h, d_src, in_counts, d_y, out_rows, out_counts, hip_stream);
}

int same_resampler_reset_channels(same_resampler *h, const uint32_t *channels, size_t n, const uint32_t *new_rates)
{
    if (!h || (!channels && n)) return fail(SAME_EINVAL, "null argument");
    const int rc = h->plan.reset(channels, n, new_rates);
    if (rc == SAME_ERATE)
        return fail(rc, "a new rate needs more than %u phases or %u taps per phase for %u Hz; nothing was reset", rs::kMaxL, rs::kMaxT, h->plan.out_rate);
    if (rc) return fail(rc, "a channel out of range, a zero rate, or more than %u distinct ratios in one handle; nothing was reset", rs::kMaxRatios);
    if (h->ratios_on_device == h->plan.ratios.size()) return SAME_OK;
    RS_HIP_TRY(hipSetDevice(h->device));
    return upload_tables(h);
}

uint64_t same_resampler_channel_input_counter(const same_resampler *h, uint32_t channel)
{
    return h && channel < h->plan.n_channels() ? h->plan.n_in[channel] : 0;
}
uint64_t same_resampler_channel_output_counter(const same_resampler *h, uint32_t channel)
{
    return h && channel < h->plan.n_channels() ? h->plan.n_out[channel] : 0;
}

}  // extern "C"
