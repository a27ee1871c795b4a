// same_tone_queue.h -- the host half of the tone family's harvest (include/same_tones.h, same_tone_audio.h,
// same_tone_delivery.h): where one call's records lie (Layout), the queue of tone events (EventQueue), and the log of audio
// chunks whose samples come to the host lazily (ChunkLog: one text for the float capture and for the delivery form).
// same_tones.hip waits for a call, and calls in here with plain pointers to the slot's pinned copies; the pinned blocks and the
// copy of a pool's used part reach the log as its storage type and as a callable.  The unit returns codes: the error text is
// same_tones.hip's.
// Host-only (no HIP): tests/helpers/tone_queue_main.cpp drives it under ASan + UBSan without a device, on plain memory
// (tests/test_tone_queue_cpu.py), and so do tone_audio_main.cpp and tone_delivery_main.cpp behind their device cores.
//
// The rules of a ChunkLog.  A block (the samples of one call) is freed, or recycled, only when its last chunk has been dropped.
// The published view and its `samples` pointers stay valid until the next publish or drop.  A slot's pool is copied out before
// the call that takes the slot next writes to it (fetch_slot).  A fetch that fails leaves its block waiting and the blocks before
// it published.  Recycled blocks wait on a free list of at most keep_free entries.
#ifndef SAME_TONE_QUEUE_H
#define SAME_TONE_QUEUE_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "../../include/same_rx.h"
#include "../../include/same_tone_delivery.h"
#include "same_tone_delivery_dev.h"

namespace same {
namespace tq {

constexpr int kSlots = 3;                         // calls of a handle that can be in flight
constexpr uint64_t kMaxCallBytes = 1ull << 31;    // each of a call's two record buffers

template <typename T>
inline T load(const uint8_t *p, size_t i = 0)
{
    T v;
    std::memcpy(&v, p + i * sizeof(T), sizeof(T));
    return v;
}

// The byte layout of one call's records, the same on the device and in a slot's pinned copies.  The event buffer: the
// channels' event counts (tn::events_offset), then the event slots.  The capture buffer, for a call with capture on: the header
// and the channels' chunk counts (cap_spans_offset, same_tone_audio_dev.h), the chunk slots, and in delivery mode one td::Out
// per chunk slot behind them.
struct Layout {
    size_t events_at = 0, spans_at = 0, outs_at = 0;
    uint64_t out_bytes = 0, cap_bytes = 0;        // cap_bytes == 0: the call ran with capture off
    uint32_t used_word = 0;                       // the header word that holds the use of the pool whose samples go to the host

    bool captures() const { return cap_bytes != 0; }
    // both: SAME_ENOMEM when the buffer would exceed kMaxCallBytes (out_bytes / cap_bytes then hold what it would take)
    int set_events(uint32_t n_channels, uint64_t event_slots)
    {
        events_at = tn::events_offset(n_channels);
        out_bytes = events_at + event_slots * sizeof(same_tone_event);
        return out_bytes > kMaxCallBytes ? SAME_ENOMEM : SAME_OK;
    }
    int set_capture(uint32_t n_channels, uint64_t chunk_slots, bool delivery)
    {
        spans_at = cap_spans_offset(n_channels);
        outs_at = spans_at + (size_t)chunk_slots * sizeof(tn::Span);      // (a multiple of 16: the output records are aligned)
        cap_bytes = outs_at + (delivery ? chunk_slots * sizeof(td::Out) : 0);
        used_word = delivery ? kCapWordDelivered : kCapWordUsed;
        return cap_bytes > kMaxCallBytes ? SAME_ENOMEM : SAME_OK;
    }
};

// the host copies of a call that has passed
struct Records {
    uint32_t n_channels;
    const tn::Desc *desc;                         // [C]: ev_off
    const uint32_t *span_off;                     // [C]: each channel's first chunk slot (capture on)
    const uint8_t *out, *cap_out;                 // the event buffer; the capture buffer (capture on)
    uint32_t out_rate;                            // delivery mode
};

// the events of the calls that have passed, from head on
struct EventQueue {
    std::vector<same_tone_event> queue;
    size_t head = 0;

    // a call's events, by channel and inside a channel in the order its lane wrote them
    void harvest(const Layout &L, const Records &r)
    {
        if (head == queue.size()) { queue.clear(); head = 0; }
        for (uint32_t c = 0; c < r.n_channels; ++c)
            for (uint32_t i = 0, n = load<uint32_t>(r.out, c); i < n; ++i)
                queue.push_back(load<same_tone_event>(r.out + L.events_at, (size_t)r.desc[c].ev_off + i));
    }
    // up to cap events leave the queue, oldest first; returns how many, *n_left (if given): how many stay
    size_t take(same_tone_event *out, size_t cap, size_t *n_left)
    {
        const size_t have = queue.size() - head, n = have < cap ? have : cap;
        if (n) std::memcpy(out, queue.data() + head, n * sizeof(same_tone_event));
        head += n;
        if (n_left) *n_left = have - n;
        return n;
    }
};

// chunk slot `at` of a call as the public record, and where its samples begin in the call's pool
inline uint64_t chunk_of(const Layout &L, const Records &r, size_t at, same_tone_audio_chunk &ch)
{
    const tn::Span sp = load<tn::Span>(r.cap_out + L.spans_at, at);
    ch = same_tone_audio_chunk{sp.channel, sp.flags, sp.kind, 0, sp.sample_counter, sp.n, sp.tone_start, nullptr};
    return sp.off;
}
inline uint64_t chunk_of(const Layout &L, const Records &r, size_t at, same_tone_delivery_chunk &ch)
{
    const tn::Span sp = load<tn::Span>(r.cap_out + L.spans_at, at);
    const td::Out o = load<td::Out>(r.cap_out + L.outs_at, at);
    ch = same_tone_delivery_chunk{sp.channel, sp.flags, sp.kind, r.out_rate, sp.sample_counter, o.out_index, o.n_out, sp.tone_start, nullptr};
    return o.off;
}

// a block's samples: a std::vector, or an owner with get() (same_hipmem.h)
template <typename T> inline T *block_data(std::vector<T> &v) { return v.data(); }
template <typename B> inline auto block_data(B &b) -> decltype(b.get()) { return b.get(); }

// The queued chunks of one record type.  Chunk: the public record; Sample: what its `samples` point at; Block: the host
// storage of one call's samples -- default-constructible, movable, with size() in samples and block_data().  A call's samples
// stay in its slot's pool until someone asks: `fetch`, wherever it appears, is int(int slot, uint64_t used, Block &mem), which
// gives mem room for `used` samples, copies the first `used` samples of that slot's pool there, and returns SAME_OK or an error.
template <typename Chunk, typename Sample, typename Block>
class ChunkLog {
public:
    // keep_free: how many blocks whose chunks have all been dropped are kept for later calls (0: a dropped block is freed)
    explicit ChunkLog(size_t keep_free_) : keep_free(keep_free_)
    {
        for (uint64_t &w : waiting) w = kNone;
    }

    // The chunks of the call in `slot` that has passed, by channel and inside a channel in stream order; their samples stay
    // in the slot's pool for now.
    void harvest(const Layout &L, const Records &r, int slot)
    {
        size_t n = 0;
        for (uint32_t c = 0; c < r.n_channels; ++c)
            for (uint32_t i = 0, k = load<uint32_t>(r.cap_out + kCapHeaderBytes, c); i < k; ++i, ++n) {
                Pending p;
                p.off = chunk_of(L, r, (size_t)r.span_off[c] + i, p.ch);
                pending.push_back(p);
            }
        if (!n) return;
        calls.emplace_back();
        Call &b = calls.back();
        b.chunks = n;
        b.used = load<uint64_t>(r.cap_out, L.used_word);
        if (b.used) { b.slot = slot; waiting[slot] = popped + calls.size() - 1; }
    }

    // The harvested calls' samples come to the host and their chunks into the view: *chunks points at the *n chunks that
    // have not been dropped.  On an error (fetch's, or SAME_ENOMEM) the view is reported empty; what was published stays so.
    template <typename Fetch>
    int publish(Fetch &&fetch, const Chunk **chunks, size_t *n)
    {
        *chunks = nullptr;
        *n = 0;
        if (head == ready.size()) { ready.clear(); head = 0; }
        size_t at = 0;
        int rc = SAME_OK;
        for (Call &b : calls) {
            if (b.published) continue;
            if ((rc = bring(b, fetch))) break;
            try { ready.reserve(ready.size() + b.chunks); } catch (...) { rc = SAME_ENOMEM; break; }
            const Sample *data = block_data(b.mem);
            for (size_t i = 0; i < b.chunks; ++i) {
                Chunk ch = pending[at + i].ch;
                ch.samples = ch.n_samples ? data + pending[at + i].off : nullptr;
                ready.push_back(ch);
            }
            at += b.chunks;
            b.published = true;
        }
        pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)at);
        if (rc) return rc;
        *n = ready.size() - head;
        *chunks = *n ? ready.data() + head : nullptr;
        return SAME_OK;
    }

    // the first n chunks of the view leave the queue; SAME_EINVAL, and nothing changes, when the view holds fewer
    int drop(size_t n)
    {
        if (n > ready.size() - head) return SAME_EINVAL;
        head += n;
        while (n) {                               // (the view's chunks are those of the oldest blocks)
            Call &b = calls.front();
            const size_t k = n < b.chunks ? n : b.chunks;
            b.chunks -= k;
            n -= k;
            if (b.chunks) continue;
            // pinning a block again for every call would cost more than the copy
            if (free_blocks.size() < keep_free && block_data(b.mem)) {
                try { free_blocks.push_back(std::move(b.mem)); } catch (...) { }
            }
            calls.pop_front();
            ++popped;
        }
        return SAME_OK;
    }

    // before slot's pool is written again: the block that still waits for it, if any, takes its samples
    template <typename Fetch>
    int fetch_slot(int slot, Fetch &&fetch)
    {
        return waiting[slot] == kNone ? SAME_OK : bring(calls[(size_t)(waiting[slot] - popped)], fetch);
    }

    size_t n_free() const { return free_blocks.size(); }

private:
    struct Pending { Chunk ch; uint64_t off; };   // off: the first sample's place in the call's pool
    struct Call {                                 // the samples of one call, on the host once fetched
        Block mem;
        size_t chunks = 0;                        // queued chunks of the call that have not been dropped
        uint64_t used = 0;                        // samples of the call's pool in use
        int slot = -1;                            // the slot whose pool holds them until they are fetched; -1: fetched
        bool published = false;                   // its chunks are in the view
    };
    static constexpr uint64_t kNone = ~0ull;

    template <typename Fetch>
    int bring(Call &b, Fetch &fetch)
    {
        if (b.slot < 0) return SAME_OK;
        // a free block with room, else any free block (it grows), else a new one
        size_t pick = free_blocks.size();
        for (size_t i = 0; i < free_blocks.size(); ++i)
            if (free_blocks[i].size() >= b.used) { pick = i; break; }
        if (pick == free_blocks.size() && pick) pick -= 1;
        if (pick < free_blocks.size()) { b.mem = std::move(free_blocks[pick]); free_blocks.erase(free_blocks.begin() + (ptrdiff_t)pick); }
        const int rc = fetch(b.slot, b.used, b.mem);
        if (rc) return rc;
        waiting[b.slot] = kNone;
        b.slot = -1;
        return SAME_OK;
    }

    const size_t keep_free;
    std::deque<Call> calls;                       // the calls whose chunks are queued, oldest first; number popped + index
    uint64_t popped = 0;                          // calls that have left the front
    uint64_t waiting[kSlots];                     // per slot: the number of the call that waits for its pool's samples, or kNone
    std::vector<Pending> pending;                 // chunks of harvested calls that are not in the view yet
    std::vector<Chunk> ready;                     // from head on: the view
    size_t head = 0;
    std::vector<Block> free_blocks;
};

}  // namespace tq
}  // namespace same
#endif  // SAME_TONE_QUEUE_H
