// same_tones.hip -- the tone detector of include/same_tones.h: its kernels and its C ABI.  The arithmetic is
// same_tones_dev.h's (one text for g++ and the device), positions and the call's work plan same_tones_plan.h's (host only).
//
// Blocks are independent of each other: only a channel's open block carries state from call to call.  So the work is
// parallel over (group of 64 adjacent channels, block of the call): a lane is a channel, a work item runs one block's serial
// recurrence.  An item loads the saved Acc only when it continues the open block (the call's block 0 of a channel with
// fill > 0), and saves one only when its block stays open (the call's last block).  Those may be two items running at the
// same time, so the Acc lives in two banks: a call reads the bank the plan names and saves to the other.  An item whose block
// completes writes P_0..2 and Em (when asked) and the block's two qualify bits.
//   tones_tm_kernel  time-major: lane c reads x[r * C + c].  Lanes whose block phases agree read one row together.
//   tones_cm_kernel  channel-major: a wavefront stages tiles of 64 channels x 64 samples through LDS -- loaded with the lanes
//                    along time (256 or 128 contiguous bytes of one channel), consumed with the lanes along channels from rows
//                    padded to 65 words, so that the 32 lanes of a half read 32 different banks.  A tile's 64 loads are
//                    issued together into registers, one tile ahead of the arithmetic.  One wavefront per
//                    workgroup: the two barriers around a tile are that wavefront's own, and the trip counts they sit in
//                    are the same in every lane (the longest block of the 64 channels, by a butterfly of shuffles).
//   tones_sm_kernel  lane = channel: both state machines over the call's qualify bits, events into the channel's own slots.
// No atomics, no word passed between wavefronts.  Behind the kernels one copy of the call's counts and event slots into the
// pinned buffer of one of tq::kSlots slots, and an event record; a slot is reused only once its event has passed and its events
// have been taken into the host queue.  The host half behind that wait -- where a call's records lie, the event queue, the chunk
// logs -- is same_tone_queue.h's (host only); this file keeps the HIP resources, the slots' wait and collect, and the error text.
// Tone-alert audio (include/same_tone_audio.h): a handle whose capture is on queues, in place of
// tones_sm_kernel, the capture-aware state-machine kernel, the prefix kernel and the layout's copy kernel of same_tone_audio.hip,
// and copies the call's chunk records behind its event slots.  The samples stay in the slot's pool on the device until the
// call has passed and someone asks for them (fetch_pool): same_tone_audio_peek, or the call that takes the slot next.
// Delivery form (include/same_tone_delivery.h): a handle in delivery mode queues, behind that capture work, the
// output-offset kernel, the decimator and the history kernel of same_tone_delivery.hip.  The float pool is then a staging buffer
// that stays on the device; what fetch_pool copies is the used part of the slot's int16 delivery pool, into a pinned host
// block that returns to a free list when its last chunk has been dropped.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/same_tone_audio.h"
#include "../../include/same_tone_delivery.h"
#include "../../include/same_tones.h"
#include "same_hipmem.h"
#include "same_tone_audio_kernels.h"
#include "same_tone_audio_plan.h"
#include "same_tone_delivery_kernels.h"
#include "same_tone_delivery_plan.h"
#include "same_tone_queue.h"
#include "same_tones_plan.h"

namespace same {
namespace {

constexpr uint32_t kItemsPerBlock = 4;            // time-major: wavefronts of a workgroup, each on a block of its own
constexpr uint32_t kMaxGridY = 65535;
constexpr uint32_t kTile = 64, kTilePitch = kTile + 1;

template <typename SampleT>
__global__ __launch_bounds__(64 * kItemsPerBlock) void tones_tm_kernel(const tn::Desc *__restrict__ desc, tn::Coef cf, const SampleT *__restrict__ x,
                                                                       float *__restrict__ acc, float *__restrict__ blocks,
                                                                       uint8_t *__restrict__ qual, uint32_t n_channels, uint32_t n_items)
{
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_channels) return;
    const tn::Desc d = desc[c];
    const size_t bank_words = (size_t)tn::kAccWords * n_channels;
    const float *bank_in = acc + ((d.flags & tn::kDescBank) ? bank_words : 0);
    float *bank_out = acc + ((d.flags & tn::kDescBank) ? 0 : bank_words);
    for (uint32_t j = blockIdx.y * kItemsPerBlock + threadIdx.y; j < n_items; j += gridDim.y * kItemsPerBlock) {
        if (j >= d.n_touch) return;               // this and every later block lies behind the channel's samples
        uint32_t r0, r1;
        tn::block_rows(d, cf.N, j, r0, r1);
        tn::Acc a = tn::block_continues(d, j) ? tn::acc_load(bank_in, n_channels, c) : tn::acc_zero();
        tn::run_rows(a, cf, x + c, n_channels, r0, r1);
        tn::block_end(d, cf, j, a, c, n_channels, blocks, qual, bank_out);
    }
}

// One tile of the channel-major kernel into registers: v[ch] = the sample of channel c0 + ch at row r0(ch) + k0 + lane of the
// call, where r0(ch), r1(ch) are lane ch's block bounds.  A lane whose row lies at or beyond r1(ch) -- the block is shorter, or
// there is no such channel (r1 == 0) -- loads x[star_at + k0] instead, a sample the group's longest block owns, and nobody
// consumes what it loaded: rows at or beyond a channel's count are never loaded, and no load hangs on a branch.
template <typename SampleT>
__device__ __forceinline__ void cm_load_tile(SampleT (&v)[kTile], const SampleT *__restrict__ x, size_t n_rows, uint32_t c0, uint32_t lane,
                                             uint32_t r0, uint32_t r1, uint32_t k0, size_t star_at)
{
#pragma unroll
    for (uint32_t ch = 0; ch < kTile; ++ch) {
        const uint32_t cr0 = (uint32_t)__builtin_amdgcn_readlane((int)r0, (int)ch), cr1 = (uint32_t)__builtin_amdgcn_readlane((int)r1, (int)ch);
        const uint64_t t = (uint64_t)cr0 + k0 + lane;
        const size_t at = t < cr1 ? (size_t)(c0 + ch) * n_rows + (size_t)t : star_at + k0;
        v[ch] = x[at];
    }
}

template <typename SampleT>
__global__ __launch_bounds__(64) void tones_cm_kernel(const tn::Desc *__restrict__ desc, tn::Coef cf, const SampleT *__restrict__ x, size_t n_rows,
                                                      float *__restrict__ acc, float *__restrict__ blocks, uint8_t *__restrict__ qual,
                                                      uint32_t n_channels, uint32_t n_items)
{
    __shared__ float tile[kTile * kTilePitch];
    const uint32_t lane = threadIdx.x;
    const uint32_t c0 = blockIdx.x * kTile, c = c0 + lane;
    const bool valid = c < n_channels;
    tn::Desc d{};                                  // (n_touch == 0: a lane without a channel owns no block)
    if (valid) d = desc[c];
    const size_t bank_words = (size_t)tn::kAccWords * n_channels;
    const float *bank_in = acc + ((d.flags & tn::kDescBank) ? bank_words : 0);
    float *bank_out = acc + ((d.flags & tn::kDescBank) ? 0 : bank_words);
    for (uint32_t j = blockIdx.y; j < n_items; j += gridDim.y) {
        const bool mine = j < d.n_touch;
        uint32_t r0 = 0, r1 = 0;
        if (mine) tn::block_rows(d, cf.N, j, r0, r1);
        const uint32_t len = r1 - r0;              // (> 0 for a block the channel touches)
        uint32_t longest = len;
        for (int m = 32; m > 0; m >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)longest, m, 64);
            longest = o > longest ? o : longest;
        }
        if (longest == 0) break;                   // the same in every lane: no channel of the group reaches block j or a later one
        // the first lane whose block is the longest: row r0 + k of its channel is one the channel owns for every k < longest,
        // the address a lane loads from when its own position lies outside the block it loads for
        const uint32_t star = (uint32_t)__builtin_ctzll(__ballot(len == longest));
        const size_t star_at = (size_t)(c0 + star) * n_rows + (uint32_t)__builtin_amdgcn_readlane((int)r0, (int)star);
        tn::Acc a = mine && tn::block_continues(d, j) ? tn::acc_load(bank_in, n_channels, c) : tn::acc_zero();
        // A tile's 64 loads are issued together, unconditionally, into registers, one tile ahead of the arithmetic: while
        // the lanes consume tile k from LDS the loads of tile k + 1 are in flight.
        SampleT v[kTile];
        cm_load_tile(v, x, n_rows, c0, lane, r0, r1, 0, star_at);
        for (uint32_t k0 = 0; k0 < longest; k0 += kTile) {
            __syncthreads();                       // (the tile before this one has been consumed)
#pragma unroll
            for (uint32_t ch = 0; ch < kTile; ++ch) tile[ch * kTilePitch + lane] = (float)v[ch];
            __syncthreads();
            if (k0 + kTile < longest) cm_load_tile(v, x, n_rows, c0, lane, r0, r1, k0 + kTile, star_at);
            const uint32_t left = len > k0 ? len - k0 : 0, n = left < kTile ? left : kTile;
            for (uint32_t i = 0; i < n; ++i) tn::step(a, cf, tile[lane * kTilePitch + i]);
        }
        if (mine) tn::block_end(d, cf, j, a, c, n_channels, blocks, qual, bank_out);
    }
}

__global__ __launch_bounds__(256) void tones_sm_kernel(const tn::Desc *__restrict__ desc, uint32_t N, const uint8_t *__restrict__ qual,
                                                       tn::Sm *__restrict__ sm, uint32_t *__restrict__ ev_counts,
                                                       same_tone_event *__restrict__ ev, uint32_t n_channels)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_channels) return;
    const tn::Desc d = desc[c];
    tn::Sm s[2] = {sm[2 * (size_t)c], sm[2 * (size_t)c + 1]};
    ev_counts[c] = tn::run_state_machines(d, N, c, n_channels, qual, s, ev);
    sm[2 * (size_t)c] = s[0];
    sm[2 * (size_t)c + 1] = s[1];
}

thread_local std::string g_tones_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_tones_error = buf;
    return code;
}

#define TN_HIP_TRY(expr)                                                                                            \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) return fail(SAME_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

}  // namespace
}  // namespace same

struct same_tones {
    same::TonesPlan plan;
    int device = 0;
    same::DevBuf<same::tn::Desc> d_desc;         // the descriptors of the call the stream is at; behind them its chunk-slot offsets
    same::DevBuf<float> d_acc;                   // two banks of [tn::kAccWords x C]: the channels' open blocks
    same::DevBuf<same::tn::Sm> d_sm;             // [C x 2]: attention, wat
    same::DevBuf<uint8_t> d_qual;                // [blocks completed x C]: the qualify bits of the call the stream is at
    same::DevBuf<uint8_t> d_out;                 // its counts and event slots
    struct Slot {
        same::PinnedBuf<same::tn::Desc> desc;
        same::PinnedBuf<uint8_t> out;
        same::Event done;
        bool in_flight = false;
        same::tq::Layout layout;                 // where the records of the call in this slot lie in out and cap_out
        // tone-alert audio: the call's chunk records and its sample pool (the mode's log knows which block waits for its samples)
        same::PinnedBuf<uint8_t> cap_out;
        same::DevBuf<float> pool;
        same::DevBuf<int16_t> dpool;             // delivery mode: the call's delivery pool (pool is then the staging buffer)
    };
    Slot slot[same::tq::kSlots];
    int next_slot = 0;                           // (the slots are used in turn: the oldest call in flight is in next_slot)
    same::tq::EventQueue events;                 // events of the calls that have passed
    bool fed = false;                            // a call has consumed samples

    // tone-alert audio
    same::ToneAudioPlan audio;
    same::DevBuf<same::tn::Cap> d_cap;           // [C]
    same::DevBuf<uint64_t> d_cap_counts;         // [C]: captured rows of the call the stream is at
    same::DevBuf<uint32_t> d_cap_flags;          // [ceil(C / 64)]
    same::DevBuf<uint8_t> d_cap_out;             // its chunk records
    hipStream_t copy_stream = nullptr;           // the lazy copies of the pools' used parts
    // the float capture's chunks, their samples in plain host blocks that are freed behind their last drop
    same::tq::ChunkLog<same_tone_audio_chunk, float, std::vector<float>> audio_log{0};

    // delivery form: the ratio and taps, the channels' histories and capture-local clocks, and the queue in its own record:
    // pinned host blocks, of which at most kSlots + 1 wait on the log's free list (a handle has one mode: the other log is empty)
    same::ToneDeliveryPlan delivery;
    same::DevBuf<float> d_taps_t;                // [T][L]
    same::DevBuf<float> d_hist;                  // [C][T - 1]
    same::DevBuf<uint64_t> d_anext;              // [C]
    same::tq::ChunkLog<same_tone_delivery_chunk, int16_t, same::PinnedBuf<int16_t>> delivery_log{same::tq::kSlots + 1};
};

namespace same {
namespace {

// the records of a call that has passed, into the event queue and the mode's chunk log
void harvest(same_tones *h, same_tones::Slot &s)
{
    const uint32_t C = h->plan.n_channels();
    const tq::Records r{C, s.desc.get(), (const uint32_t *)(s.desc.get() + C), s.out.get(), s.cap_out.get(), h->delivery.params.rate};
    h->events.harvest(s.layout, r);
    s.in_flight = false;
    if (!s.layout.captures()) return;
    if (h->delivery.on()) h->delivery_log.harvest(s.layout, r, (int)(&s - h->slot));
    else h->audio_log.harvest(s.layout, r, (int)(&s - h->slot));
}

// What the chunk logs fetch with: the used part of a passed call's pool into its host block -- plain memory for the float
// capture, pinned and sized in steps of 64 Ki samples for the delivery form.  Waits for that copy, never for a call in flight.
template <typename Block>
int fetch_pool(same_tones *h, int slot, uint64_t used, Block &mem)
{
    const void *pool;
    if constexpr (std::is_same<Block, std::vector<float>>::value) {
        try { mem.resize((size_t)used); } catch (...) { return fail(SAME_ENOMEM, "%llu captured samples on the host", (unsigned long long)used); }
        pool = h->slot[slot].pool.get();
    } else {
        const hipError_t e = mem.ensure(((size_t)used + 0xffff) & ~(size_t)0xffff);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "%llu delivered samples on the host: %s", (unsigned long long)used, hipGetErrorString(e));
        pool = h->slot[slot].dpool.get();
    }
    TN_HIP_TRY(hipMemcpyAsync(tq::block_data(mem), pool, (size_t)used * sizeof(*tq::block_data(mem)), hipMemcpyDeviceToHost, h->copy_stream));
    TN_HIP_TRY(hipStreamSynchronize(h->copy_stream));
    return SAME_OK;
}

// before a call writes slot's pools: the block that still waits for their samples takes them
int fetch_slot(same_tones *h, int slot)
{
    const auto fetch = [h](int i, uint64_t used, auto &mem) { return fetch_pool(h, i, used, mem); };
    return h->delivery.on() ? h->delivery_log.fetch_slot(slot, fetch) : h->audio_log.fetch_slot(slot, fetch);
}

int wait_slot(same_tones *h, same_tones::Slot &s)
{
    if (!s.in_flight) return SAME_OK;
    TN_HIP_TRY(hipEventSynchronize(s.done));
    harvest(h, s);
    return SAME_OK;
}

// the slots whose calls have passed, oldest first, up to the first that has not
int collect(same_tones *h, bool wait)
{
    for (int i = 0; i < tq::kSlots; ++i) {
        same_tones::Slot &s = h->slot[(h->next_slot + i) % tq::kSlots];
        if (!s.in_flight) continue;
        if (wait) { const int rc = wait_slot(h, s); if (rc) return rc; continue; }
        const hipError_t e = hipEventQuery(s.done);
        if (e == hipErrorNotReady) break;
        if (e != hipSuccess) return fail(SAME_EHIP, "hipEventQuery failed: %s", hipGetErrorString(e));
        harvest(h, s);
    }
    return SAME_OK;
}

// same_tone_audio_peek / same_tone_delivery_peek on the record's log (the log of the mode the handle is not in holds nothing)
template <typename Log, typename Chunk>
int peek(same_tones *h, Log same_tones::*log, const Chunk **chunks, size_t *n, const char *what)
{
    if (!h || !chunks || !n) return fail(SAME_EINVAL, "null argument");
    *chunks = nullptr;
    *n = 0;
    TN_HIP_TRY(hipSetDevice(h->device));
    int rc = collect(h, false), fetched = SAME_OK;
    if (rc) return rc;
    rc = (h->*log).publish([&](int slot, uint64_t used, auto &mem) { return fetched = fetch_pool(h, slot, used, mem); }, chunks, n);
    return rc && !fetched ? fail(rc, "%s view", what) : rc;      // (a fetch that failed has said why)
}

template <typename Log>
int drop(same_tones *h, Log same_tones::*log, size_t n)
{
    if (!h) return fail(SAME_EINVAL, "null argument");
    return (h->*log).drop(n) ? fail(SAME_EINVAL, "more chunks than the view holds") : SAME_OK;
}

template <typename SampleT>
int process(same_tones *h, const SampleT *d_x, size_t n_rows, const uint32_t *counts, int layout, float *d_blocks, size_t block_rows,
            void *hip_stream)
{
    if (!h) return fail(SAME_EINVAL, "null handle");
    if (layout != SAME_LAYOUT_TIME_MAJOR && layout != SAME_LAYOUT_CHANNEL_MAJOR)
        return fail(SAME_EINVAL, "layout %d is neither time-major nor channel-major; nothing was consumed", layout);
    const uint32_t C = h->plan.n_channels();
    uint32_t max_blocks = 0;
    if (h->plan.block_counts(counts, n_rows, nullptr, &max_blocks))
        return fail(SAME_EINVAL, "a count exceeds n_rows = %zu, or n_rows exceeds 2^32 - 1; nothing was consumed", n_rows);
    if (d_blocks && max_blocks > block_rows)
        return fail(SAME_EINVAL, "block_rows = %zu, the call completes up to %u blocks; nothing was consumed", block_rows, max_blocks);
    TN_HIP_TRY(hipSetDevice(h->device));
    same_tones::Slot &s = h->slot[h->next_slot];
    int rc = wait_slot(h, s);
    if (rc) return rc;
    const TonesPlan::Shape shape = h->plan.describe(counts, n_rows, s.desc.get());
    if (!shape.any_samples) return SAME_OK;       // nothing to read: a no-op (a pending reset stays pending)
    if (!d_x) return fail(SAME_EINVAL, "null d_x with samples to read; nothing was consumed");
    tq::Layout at;                                // where the call's records lie, here and for its harvest
    if (at.set_events(C, shape.event_slots)) return fail(SAME_ENOMEM, "the call needs %llu bytes of event slots; nothing was consumed", (unsigned long long)at.out_bytes);
    // (a buffer that grows is freed first, which waits for the device: nothing in flight loses it)
    hipError_t e = h->d_qual.ensure((size_t)(shape.max_complete ? shape.max_complete : 1) * C);
    if (e == hipSuccess) e = h->d_out.ensure((size_t)at.out_bytes);
    if (e == hipSuccess) e = s.out.ensure((size_t)at.out_bytes);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the call's buffers failed: %s; nothing was consumed", hipGetErrorString(e));
    // capture on: the chunk slots behind the descriptors, room for the chunk records, and the slot's pool free to be written
    const bool capture = h->audio.on();
    if (capture) {
        if ((rc = fetch_slot(h, h->next_slot))) return rc;
        const uint64_t slots = ToneAudioPlan::describe(s.desc.get(), C, (uint32_t *)(s.desc.get() + C));
        if (at.set_capture(C, slots, h->delivery.on()))
            return fail(SAME_ENOMEM, "the call needs %llu bytes of chunk slots; nothing was consumed", (unsigned long long)at.cap_bytes);
        e = h->d_cap_out.ensure((size_t)at.cap_bytes);
        if (e == hipSuccess) e = s.cap_out.ensure((size_t)at.cap_bytes);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the call's chunk records failed: %s; nothing was consumed", hipGetErrorString(e));
    }

    hipStream_t stream = (hipStream_t)hip_stream;
    TN_HIP_TRY(hipMemcpyAsync(h->d_desc.get(), s.desc.get(), (size_t)C * (sizeof(tn::Desc) + (capture ? sizeof(uint32_t) : 0)), hipMemcpyHostToDevice, stream));
    const uint32_t groups = (C + 63) / 64;
    if (layout == SAME_LAYOUT_TIME_MAJOR) {
        const uint32_t gy = (shape.max_touch + kItemsPerBlock - 1) / kItemsPerBlock;
        hipLaunchKernelGGL(tones_tm_kernel<SampleT>, dim3(groups, gy < kMaxGridY ? gy : kMaxGridY), dim3(64, kItemsPerBlock), 0, stream,
                           h->d_desc.get(), h->plan.coef, d_x, h->d_acc.get(), d_blocks, h->d_qual.get(), C, shape.max_touch);
    } else {
        hipLaunchKernelGGL(tones_cm_kernel<SampleT>, dim3(groups, shape.max_touch < kMaxGridY ? shape.max_touch : kMaxGridY), dim3(64), 0,
                           stream, h->d_desc.get(), h->plan.coef, d_x, n_rows, h->d_acc.get(), d_blocks, h->d_qual.get(), C, shape.max_touch);
    }
    TN_HIP_TRY(hipGetLastError());
    if (capture) {
        const ToneAudioCall k{h->d_desc.get(), (const uint32_t *)(h->d_desc.get() + C), h->d_qual.get(), h->d_sm.get(), h->d_cap.get(),
                              h->audio.params, (uint32_t *)h->d_out.get(), (same_tone_event *)(h->d_out.get() + at.events_at),
                              h->d_cap_out.get(), h->d_cap_counts.get(), h->d_cap_flags.get(), s.pool.get(), h->audio.pool_cap,
                              h->plan.coef.N, C};
        TN_HIP_TRY(tone_audio_launch_sm(k, stream));
        TN_HIP_TRY(tone_audio_launch_copy(k, d_x, n_rows, layout, stream));
        if (h->delivery.on()) {
            const td::Params &p = h->delivery.params;
            // a chunk has at most n_rows placed rows: its outputs, in tiles of 256
            const uint64_t most = rs::outputs_after(n_rows, p.L, p.M) + 1;
            const ToneDeliveryCall dk{p, h->d_taps_t.get(), h->d_hist.get(), h->d_anext.get(), s.dpool.get(), at.outs_at,
                                      (uint32_t)((most + td::kTileOutputs - 1) / td::kTileOutputs)};
            TN_HIP_TRY(tone_delivery_launch(k, dk, stream));
            TN_HIP_TRY(tone_delivery_launch_history(k, dk, d_x, n_rows, layout, stream));
        }
        TN_HIP_TRY(hipMemcpyAsync(s.cap_out.get(), h->d_cap_out.get(), (size_t)at.cap_bytes, hipMemcpyDeviceToHost, stream));
    } else {
        hipLaunchKernelGGL(tones_sm_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, h->d_desc.get(), h->plan.coef.N, h->d_qual.get(),
                           h->d_sm.get(), (uint32_t *)h->d_out.get(), (same_tone_event *)(h->d_out.get() + at.events_at), C);
        TN_HIP_TRY(hipGetLastError());
    }
    TN_HIP_TRY(hipMemcpyAsync(s.out.get(), h->d_out.get(), (size_t)at.out_bytes, hipMemcpyDeviceToHost, stream));
    TN_HIP_TRY(hipEventRecord(s.done, stream));
    s.in_flight = true;
    s.layout = at;
    h->fed = true;
    h->next_slot = (h->next_slot + 1) % tq::kSlots;
    h->plan.commit(s.desc.get());
    return SAME_OK;
}

}  // namespace
}  // namespace same

using namespace same;

extern "C" {

const char *same_tones_last_error(void) { return g_tones_error.c_str(); }

int same_tones_new(uint32_t n_channels, uint32_t rate, int device, same_tones **out)
{
    if (!out) return fail(SAME_EINVAL, "null out");
    *out = nullptr;
    same_tones *h = new (std::nothrow) same_tones;
    if (!h) return fail(SAME_ENOMEM, "out of memory");
    // (the plan first: a refused rate is refused with or without a device)
    const int rc = h->plan.init(n_channels, rate);
    if (rc) {
        delete h;
        return rc == SAME_ERATE ? fail(rc, "rate %u Hz is outside %u .. %u Hz", rate, SAME_TONES_MIN_RATE, SAME_TONES_MAX_RATE)
                                : fail(rc, "zero channels");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { delete h; return fail(SAME_ENODEVICE, "no HIP device visible (this library has no CPU path)"); }
    if (device < 0 || device >= ndev) { delete h; return fail(SAME_ENODEVICE, "device %d out of range (%d visible)", device, ndev); }
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = h->d_desc.ensure(n_channels);
    if (e == hipSuccess) e = h->d_acc.ensure((size_t)2 * tn::kAccWords * n_channels);      // (read only where a call saved before)
    if (e == hipSuccess) e = h->d_sm.ensure((size_t)2 * n_channels);                        // (made idle by the first call that runs)
    for (same_tones::Slot &s : h->slot) {
        if (e == hipSuccess) e = s.desc.ensure(n_channels);
        if (e == hipSuccess) e = s.done.ensure();
    }
    if (e != hipSuccess) {
        delete h;
        return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the tone detector failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return SAME_OK;
}

void same_tones_free(same_tones *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    // (the kernels in flight read the handle's buffers)
    for (same_tones::Slot &s : h->slot)
        if (s.in_flight) (void)hipEventSynchronize(s.done);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    delete h;
}

int same_tone_audio_set(same_tones *h, uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, size_t samples_per_call)
{
    if (!h) return fail(SAME_EINVAL, "null handle");
    if (h->fed) return fail(SAME_EINVAL, "capture is set before the handle's first sample");
    ToneAudioPlan plan;
    if (plan.set(kinds, tail_blocks, max_blocks, samples_per_call))
        return fail(SAME_EINVAL, "kinds = %u is not a non-zero mask of SAME_TONE_ATTENTION | SAME_TONE_WAT, or max_blocks = %u is zero", kinds, max_blocks);
    TN_HIP_TRY(hipSetDevice(h->device));
    h->audio = ToneAudioPlan();                   // (off until everything is there)
    h->delivery = ToneDeliveryPlan();             // (the float mode, or none: not the delivery form)
    hipError_t e = hipSuccess;
    for (same_tones::Slot &s : h->slot)
        if (e == hipSuccess) e = s.dpool.reset();
    if (!plan.on()) {
        for (same_tones::Slot &s : h->slot)
            if (e == hipSuccess) e = s.pool.reset();
        if (e != hipSuccess) return fail(SAME_EHIP, "freeing the pools failed: %s", hipGetErrorString(e));
        return SAME_OK;
    }
    const uint32_t C = h->plan.n_channels();
    const size_t desc_room = (size_t)C + ((size_t)C * sizeof(uint32_t) + sizeof(tn::Desc) - 1) / sizeof(tn::Desc);   // descriptors, then C chunk-slot offsets
    if (!h->copy_stream) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->d_desc.ensure(desc_room);
    if (e == hipSuccess) e = h->d_cap.ensure(C);                                  // (made zero by the first call that runs)
    if (e == hipSuccess) e = h->d_cap_counts.ensure(C);
    if (e == hipSuccess) e = h->d_cap_flags.ensure((C + 63) / 64);
    for (same_tones::Slot &s : h->slot) {
        if (e == hipSuccess) e = s.desc.ensure(desc_room);
        if (e == hipSuccess) e = s.pool.reset();
        if (e == hipSuccess) e = s.pool.ensure(samples_per_call);
    }
    if (e != hipSuccess) {
        for (same_tones::Slot &s : h->slot) (void)s.pool.reset();
        return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the capture's pools (3 x %zu samples) failed: %s; capture is off", samples_per_call,
                    hipGetErrorString(e));
    }
    h->audio = plan;
    return SAME_OK;
}

int same_tone_audio_peek(same_tones *h, const same_tone_audio_chunk **chunks, size_t *n) { return peek(h, &same_tones::audio_log, chunks, n, "audio"); }
int same_tone_audio_drop(same_tones *h, size_t n) { return drop(h, &same_tones::audio_log, n); }

int same_tone_delivery_set(same_tones *h, uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, size_t samples_per_call, uint32_t out_rate,
                           float gain)
{
    if (!h) return fail(SAME_EINVAL, "null handle");
    if (h->fed) return fail(SAME_EINVAL, "delivery is set before the handle's first sample");
    ToneDeliveryPlan plan;
    const int prc = plan.set(kinds, tail_blocks, max_blocks, samples_per_call, h->plan.rate, out_rate, gain);
    if (prc == SAME_ERATE) return fail(prc, "%u -> %u Hz needs more than %u phases or %u taps", h->plan.rate, out_rate, rs::kMaxL, rs::kMaxT);
    if (prc)
        return fail(prc, "kinds = %u is not a non-zero mask of SAME_TONE_ATTENTION | SAME_TONE_WAT, max_blocks = %u is zero, gain = %g is not finite and "
                         "positive, or out_rate = %u is zero or above the handle's %u Hz", kinds, max_blocks, (double)gain, out_rate, h->plan.rate);
    // the float path's memory first: the staging pools and the capture state (this also leaves the delivery form off)
    const int rc = same_tone_audio_set(h, kinds, tail_blocks, max_blocks, samples_per_call);
    if (rc || !plan.on()) return rc;
    h->audio = ToneAudioPlan();                   // (off until everything is there)
    const uint32_t C = h->plan.n_channels();
    const td::Params &p = plan.params;
    hipError_t e = h->d_taps_t.ensure(plan.taps_t.size());
    if (e == hipSuccess) e = h->d_hist.ensure((size_t)C * (p.T - 1) + 1);
    if (e == hipSuccess) e = h->d_anext.ensure(C);
    // L <= M: a call delivers no more samples than it placed rows, so samples_per_call int16 cannot overflow
    for (same_tones::Slot &s : h->slot)
        if (e == hipSuccess) e = s.dpool.ensure(samples_per_call);
    if (e == hipSuccess) e = hipMemcpy(h->d_taps_t.get(), plan.taps_t.data(), plan.taps_t.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->d_anext.get(), 0, (size_t)C * sizeof(uint64_t));
    if (e != hipSuccess) {
        for (same_tones::Slot &s : h->slot) { (void)s.pool.reset(); (void)s.dpool.reset(); }
        return fail(e == hipErrorOutOfMemory ? SAME_ENOMEM : SAME_EHIP, "allocating the delivery pools (3 x %zu samples) failed: %s; capture is off",
                    samples_per_call, hipGetErrorString(e));
    }
    h->audio = plan.audio;
    h->delivery = std::move(plan);
    return SAME_OK;
}

int same_tone_delivery_peek(same_tones *h, const same_tone_delivery_chunk **chunks, size_t *n) { return peek(h, &same_tones::delivery_log, chunks, n, "delivery"); }
int same_tone_delivery_drop(same_tones *h, size_t n) { return drop(h, &same_tones::delivery_log, n); }

uint32_t same_tone_audio_chunk_bound(uint32_t n_blocks) { return tn::chunk_bound(n_blocks); }

uint32_t same_tones_n_channels(const same_tones *h) { return h ? h->plan.n_channels() : 0; }
uint32_t same_tones_rate(const same_tones *h) { return h ? h->plan.rate : 0; }
uint32_t same_tones_block_length(const same_tones *h) { return h ? h->plan.coef.N : 0; }

int same_tones_coefficients(const same_tones *h, float out[3])
{
    if (!h || !out) return fail(SAME_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k) out[k] = h->plan.coef.c[k];
    return SAME_OK;
}

int same_tones_block_counts(const same_tones *h, const uint32_t *counts, size_t n_rows, uint32_t *block_counts, uint32_t *max_blocks)
{
    if (!h || !block_counts || !max_blocks) return fail(SAME_EINVAL, "null argument");
    if (h->plan.block_counts(counts, n_rows, block_counts, max_blocks))
        return fail(SAME_EINVAL, "a count exceeds n_rows = %zu, or n_rows exceeds 2^32 - 1", n_rows);
    return SAME_OK;
}

int same_tones_process_device(same_tones *h, const float *d_x, size_t n_rows, const uint32_t *counts, int layout, float *d_blocks,
                              size_t block_rows, void *hip_stream)
{
    return process(h, d_x, n_rows, counts, layout, d_blocks, block_rows, hip_stream);
}

int same_tones_process_device_i16(same_tones *h, const int16_t *d_x, size_t n_rows, const uint32_t *counts, int layout, float *d_blocks,
                                  size_t block_rows, void *hip_stream)
{
    return process(h, d_x, n_rows, counts, layout, d_blocks, block_rows, hip_stream);
}

int same_tones_sync(same_tones *h)
{
    if (!h) return fail(SAME_EINVAL, "null handle");
    TN_HIP_TRY(hipSetDevice(h->device));
    return collect(h, true);
}

int same_tones_poll(same_tones *h, same_tone_event *out, size_t cap, size_t *n_out, size_t *n_left)
{
    if (!h || (!out && cap) || !n_out) return fail(SAME_EINVAL, "null argument");
    *n_out = 0;
    TN_HIP_TRY(hipSetDevice(h->device));
    const int rc = collect(h, false);
    if (rc) return rc;
    *n_out = h->events.take(out, cap, n_left);
    return SAME_OK;
}

int same_tones_reset_channels(same_tones *h, const uint32_t *channels, size_t n)
{
    if (!h || (!channels && n)) return fail(SAME_EINVAL, "null argument");
    if (h->plan.reset(channels, n)) return fail(SAME_EINVAL, "a channel out of range; nothing was reset");
    return SAME_OK;
}

uint64_t same_tones_channel_sample_counter(const same_tones *h, uint32_t channel)
{
    return h && channel < h->plan.n_channels() ? h->plan.pos[channel] : 0;
}

}  // extern "C"
