// same_tone_audio_dev.h -- tone-alert audio (include/same_tone_audio.h) as __host__ __device__ code: no heap, no STL.  The
// capture state machine Cap beside the two Sm of same_tones_dev.h, the listing of a call's captured rows as spans, and how a
// span gets its room in the call's sample pool are one text for the device (same_tone_audio.hip) and for a plain C++ compiler,
// where tests/helpers/tone_audio_main.cpp holds them against the numpy reference (tests/helpers/tone_audio_reference.py)
// under ASan + UBSan.
//
// The contract.  Captures are made of whole blocks: block b of a channel is captured if and only if Cap.open
// is set at its first sample, that is behind the decision of block b - 1.  cap_step() takes the decision at the end of a
// completed block, behind both sm_step()s of that block.  A block that stays open at the end of a call is captured by the same
// rule: its rows of this call are copied in this call and the rest with the call that continues it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/same_tone_audio.h"
#include "same_tones_dev.h"

namespace same {
namespace tn {

struct CapParams { uint32_t kinds, tail_blocks, max_blocks; };

// the capture state of one channel
struct Cap { uint64_t first, tone_start; uint32_t open, kind, len, left; };
static_assert(sizeof(Cap) == 32, "two capture states per 64-byte line");

SAME_HD inline Cap cap_zero() { return Cap{0, 0, 0, 0, 0, 0}; }

// The decision at the end of completed block b.  started: the enabled kinds that emitted START in block b; act: some enabled
// kind is active behind block b; start_of[k]: the start of class k (0: attention, 1: wat).  Returns 0, or the END flag of the
// capture that block b closes (block b is then the capture's last block).
SAME_HD inline uint32_t cap_step(Cap &c, const CapParams &p, uint32_t started, bool act, uint64_t b, uint32_t N, const uint64_t start_of[2])
{
    uint32_t closed = 0;
    if (c.open) {
        c.len += 1;
        if (act) c.left = p.tail_blocks;
        else if (c.left == 0) { c.open = 0; closed = SAME_TONE_AUDIO_END_TAIL; }
        else c.left -= 1;
        if (c.open && c.len == p.max_blocks) { c.open = 0; closed = SAME_TONE_AUDIO_END_MAX; }
    } else if (started) {
        c.open = 1;
        c.kind = (started & SAME_TONE_ATTENTION) ? SAME_TONE_ATTENTION : SAME_TONE_WAT;
        c.tone_start = start_of[c.kind == SAME_TONE_ATTENTION ? 0 : 1];
        c.first = (b + 1) * N;
        c.len = 0;
        c.left = p.tail_blocks;
    }
    return closed;
}

// Chunks one channel can have in a call in which it completes n blocks: SAME_TONE_AUDIO_CHUNK_BOUND(n).
//
// Proof.  A call's chunks of a channel are the maximal runs of its captured rows.  open changes only in cap_step, so a run ends
// inside the call only where a capture closes, and it begins either with the call's first row (the capture was open on entry:
// at most one such run) or with the block behind one in which a capture opened.  So chunks <= 1 + opens, and <= opens when no
// capture was open on entry.  Number the call's completed blocks 0 .. n-1.  A capture opens only in the else branch: not in a
// block in which one closes, and only when a class emits START in that block.  Between two opens lies a close, so two opens lie
// at least 2 blocks apart, and the STARTs of one class lie at least 30 blocks apart (same_tones_dev.h).  Give every open to a
// class that started in its block.  Open on entry: the capture closes in block >= 0, the first open lies in block >= 1, the
// second in block >= 3: the class that has the first open has its i-th open in block >= 1 + 30 (i - 1), the other class in block
// >= 3 + 30 (i - 1); with blocks <= n - 1 that is floor((n + 28) / 30) + floor((n + 26) / 30) opens.  Not open on entry: blocks
// >= 0 and >= 2, floor((n + 29) / 30) + floor((n + 27) / 30) opens, and the two terms exceed the former two by one only for
// n = 1 and n = 3 mod 30 respectively, never both: no more chunks than 1 + the former.
// The bound is met with equality by a channel that enters the call with a capture open, max_blocks = 1, tail_blocks = 0, the
// attention class not active with run == 23 and the wat class not active with run == 21, where attention qualifies in blocks
// 0 and 1, wat in blocks 0 .. 3, and behind that each class sees in turn 5 blocks without and 25 blocks with: captures open in
// blocks 1, 3, 31, 33, ... (tests/helpers/tone_audio_main.cpp runs it).  Entry states are taken as they can be stored, not as
// a stream can produce them, so the bound is safe, and for some n a stream stays below it.
SAME_HD inline uint32_t chunk_bound(uint32_t n) { return SAME_TONE_AUDIO_CHUNK_BOUND(n); }

// a run of captured rows of one channel in one call
struct Span {
    uint32_t channel, flags, kind;
    uint32_t row0;            // the call's row of the run's first sample
    uint64_t sample_counter;  // the channel's counter of that sample
    uint64_t n;               // rows of the run; behind span_place: samples that got room in the pool (fewer: TRUNCATED)
    uint64_t tone_start;
    uint64_t off;             // offset among the channel's captured samples of the call; behind span_place: in the call's pool
};
static_assert(sizeof(Span) == 48, "span records are copied to the host as they are");

// Both state machines and the capture of one channel over one call: what run_state_machines() does, with cap_step() behind
// every completed block and the captured rows listed.  ev as in run_state_machines (*n_ev: events written); spans: the channel's
// own chunk_bound(d.n_complete) slots (*n_spans: spans written).  Returns the channel's captured rows of the call.
SAME_HD inline uint64_t run_capture(const Desc &d, uint32_t N, uint32_t c, size_t C, const uint8_t *qual, Sm *sm /* [2] */, Cap &cap,
                                    const CapParams &p, same_tone_event *ev, uint32_t *n_ev, Span *spans, uint32_t *n_spans)
{
    if (d.flags & kDescClear) { sm[0] = sm_zero(); sm[1] = sm_zero(); cap = cap_zero(); }
    const uint32_t ev_cap = events_bound(d.n_complete), span_cap = chunk_bound(d.n_complete);
    const uint64_t pos = d.block0 * N + d.fill;       // the channel's counter of the call's row 0
    uint32_t ne = 0, ns = 0;
    uint64_t total = 0;
    bool in_run = false;
    Span cur{};
    for (uint32_t j = 0; j < d.n_touch; ++j) {
        if (cap.open) {
            uint32_t r0, r1;
            block_rows(d, N, j, r0, r1);
            if (!in_run) {
                in_run = true;
                cur = Span{c, pos + r0 == cap.first ? (uint32_t)SAME_TONE_AUDIO_FIRST : 0u, cap.kind, r0, pos + r0, 0, cap.tone_start, total};
            }
            cur.n += r1 - r0;
            total += r1 - r0;
        }
        if (j >= d.n_complete) break;                 // (the call's last block stays open: no decision yet)
        const uint32_t q = qual[(size_t)j * C + c];
        uint32_t started = 0;
        same_tone_event e;
        if (sm_step(sm[0], (q & kQAttention) != 0, d.block0 + j, N, c, SAME_TONE_ATTENTION, &e)) {
            if (ne < ev_cap) ev[d.ev_off + ne++] = e;
            if (e.edge == SAME_TONE_START) started |= SAME_TONE_ATTENTION;
        }
        if (sm_step(sm[1], (q & kQWat) != 0, d.block0 + j, N, c, SAME_TONE_WAT, &e)) {
            if (ne < ev_cap) ev[d.ev_off + ne++] = e;
            if (e.edge == SAME_TONE_START) started |= SAME_TONE_WAT;
        }
        const bool act = ((p.kinds & SAME_TONE_ATTENTION) && sm[0].active) || ((p.kinds & SAME_TONE_WAT) && sm[1].active);
        const uint64_t start_of[2] = {sm[0].start, sm[1].start};
        const uint32_t closed = cap_step(cap, p, started & p.kinds, act, d.block0 + j, N, start_of);
        if (closed) {                                 // (a capture closes only when open: block j was captured, the run holds it)
            cur.flags |= closed;
            if (ns < span_cap) spans[ns++] = cur;
            in_run = false;
        }
    }
    if (in_run && ns < span_cap) spans[ns++] = cur;
    *n_ev = ne;
    *n_spans = ns;
    return total;
}

// A span's room in the call's pool of pool_cap samples, base: the captured rows of the channels before this one.  Room is
// handed out in channel order, then in stream order: the first span that does not fit is cut, every later one gets nothing,
// and all of them are marked TRUNCATED.
SAME_HD inline void span_place(Span &s, uint64_t base, uint64_t pool_cap)
{
    s.off += base;
    const uint64_t room = s.off < pool_cap ? pool_cap - s.off : 0;
    if (room < s.n) { s.n = room; s.flags |= SAME_TONE_AUDIO_TRUNCATED; }
}

}  // namespace tn

// where a call's chunk records lie, on the device and in the pinned copy: a header of uint64 words (captured samples of the
// call; samples of the float pool in use; in delivery mode the delivered samples, the delivery pool's use), the channels' chunk
// counts padded as the event counts are, the chunk slots
constexpr size_t kCapHeaderBytes = 32;
constexpr uint32_t kCapWordUsed = 1, kCapWordDelivered = 2;
SAME_HD inline size_t cap_spans_offset(uint32_t n_channels) { return kCapHeaderBytes + tn::events_offset(n_channels); }

}  // namespace same
