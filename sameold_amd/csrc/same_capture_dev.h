// same_capture_dev.h -- which samples of a launch belong to an open message (same_batch_set_audio_capture): heap-free
// __host__ __device__ code.  The transport lane of a channel (same_transport.hip) feeds it the channel's messages of the launch
// in order and it reserves room for the spans they delimit in the launch's pool; the capture kernel (same_capture.hip) then
// copies those rows of the launch's input.  The same text compiles with a plain C++ compiler, where
// tests/helpers/capture_spans_fuzz.cpp holds it, launch by launch, against the rule stated over a whole stream.
//
// The capture of a message (what samedec hands its child, crates/samedec/src/app.rs:200-232): the channel's samples
// x[som.sample_counter, next.sample_counter), `next` being its next message -- an EndOfMessage, a forced one, or a new
// StartOfMessage, which opens a capture of its own.  Counters are the batch's (DevMessage::sample_counter); a launch covers
// [start, start + n_rows), row r being counter start + r.  Rows from flush_row on were fed by same_batch_flush and are never
// captured: a capture open there ends at the flush position, and a StartOfMessage the flush yields gets an empty one.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef SAME_HD
#if defined(__HIPCC__)
#define SAME_HD __host__ __device__
#else
#define SAME_HD
#endif
#endif

namespace same {
namespace cap {

// chunk flags (SAME_AUDIO_* in include/same_rx.h)
constexpr uint32_t kFirst = 1u, kEndMessage = 2u, kEndFlush = 4u, kEndReset = 8u, kTruncated = 16u;
constexpr uint32_t kNoFlush = 0xffffffffu;          // Launch::flush_row: no flush sample in this launch
constexpr uint32_t kAudioOverflow = 16u;            // bit of the launch's overflow word: a span or its samples did not fit
constexpr uint32_t kMsgStart = 18u, kMsgEnd = 19u;  // SAME_TRANSPORT_MSG_START / _END

// a channel's capture between launches (an array of its own, beside the transport layer's records)
struct Rec {
    uint64_t from;          // first counter not yet delivered
    uint32_t open;          // a capture is open
    uint32_t first;         // ... and its first chunk has not been delivered yet
};
static_assert(sizeof(Rec) == 16, "capture record");

// one chunk of a launch: rows [row0, row0 + n) of channel `channel`, in the pool at [off, off + n)
struct Span {
    uint32_t channel, flags;
    uint64_t counter;       // batch counter of the chunk's first sample
    uint64_t off;           // where its samples are in the pool
    uint32_t row0, n;       // n: samples stored (fewer than the span has if it is marked kTruncated)
};
static_assert(sizeof(Span) == 32, "span record");

// a launch's cursors (device memory; the capture kernel's epilogue publishes them to the host and zeroes them for the slot's next launch)
struct Cursors {
    uint32_t n_spans, overflow;
    unsigned long long pool_used;
};
static_assert(sizeof(Cursors) == 16, "cursors");

struct Launch {
    uint64_t start;                   // batch counter of row 0
    uint32_t n_rows, flush_row;       // rows of the launch; first row fed by a flush (kNoFlush: none)
    Rec *rec;                         // [n_channels]; nullptr: capture is off
    Span *spans; uint32_t span_cap;
    uint32_t *n_spans;                // cursor of `spans` (may pass span_cap: those spans are lost, kAudioOverflow)
    unsigned long long *pool_used;    // cursor of the pool, in samples (may pass pool_cap)
    uint64_t pool_cap;
    uint32_t *overflow;
};

SAME_HD inline uint32_t add_u32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const uint32_t o = *p; *p = o + v; return o;
#endif
}
SAME_HD inline unsigned long long add_u64(unsigned long long *p, unsigned long long v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const unsigned long long o = *p; *p = o + v; return o;
#endif
}
SAME_HD inline void or_u32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// One channel's walk over its messages of one launch: on_message() for each (in order), then finish().
// RAGGED (a ragged launch, same_batch_process_*_ragged): the channel consumed only the launch's first `rows` rows, and its
// captures stop there; the other rows are not its samples.
template <bool RAGGED>
struct WalkerT {
    const Launch &L;
    uint32_t c;
    Rec r;
    uint32_t rows = 0;

    SAME_HD WalkerT(const Launch &l, uint32_t channel) : L(l), c(channel), r(l.rec ? l.rec[channel] : Rec{0, 0, 0}) {}
    SAME_HD WalkerT(const Launch &l, uint32_t channel, uint32_t own_rows) : L(l), c(channel), r(l.rec ? l.rec[channel] : Rec{0, 0, 0}), rows(own_rows) {}
    SAME_HD uint32_t n_rows() const { return RAGGED ? rows : L.n_rows; }
    SAME_HD bool has_flush() const { return L.flush_row != kNoFlush; }
    SAME_HD uint64_t real_end() const { return L.start + (has_flush() ? L.flush_row : n_rows()); }      // end of the rows that may be captured
    SAME_HD uint64_t clamp(uint64_t m) const { return m < L.start ? L.start : (m > L.start + n_rows() ? L.start + n_rows() : m); }
    SAME_HD uint64_t from() const { return r.from < L.start ? L.start : r.from; }

    // the chunk [a, b) (counters, inside [start, real_end()]) with `flags`
    SAME_HD void emit(uint64_t a, uint64_t b, uint32_t flags)
    {
        if (r.first) { flags |= kFirst; r.first = 0; }
        const uint64_t len = b > a ? b - a : 0;
        const uint32_t k = add_u32(L.n_spans, 1u);
        if (k >= L.span_cap) { or_u32(L.overflow, kAudioOverflow); return; }
        uint64_t off = 0, stored = 0;
        if (len) {
            off = add_u64(L.pool_used, len);
            stored = off >= L.pool_cap ? 0 : (len < L.pool_cap - off ? len : L.pool_cap - off);
            if (stored < len) { flags |= kTruncated; or_u32(L.overflow, kAudioOverflow); }
            if (!stored) off = 0;
        }
        Span &s = L.spans[k];
        s.channel = c; s.flags = flags; s.counter = a; s.off = off;
        s.row0 = (uint32_t)(a - L.start); s.n = (uint32_t)stored;
    }
    SAME_HD void on_message(uint32_t kind, uint64_t counter)
    {
        if (kind != kMsgStart && kind != kMsgEnd) return;
        const uint64_t m = clamp(counter);
        if (has_flush() && m > real_end()) {
            // yielded by the flush: whatever was open ended where the flush began
            if (r.open) { emit(from(), real_end(), kEndFlush); r.open = 0; }
            if (kind == kMsgStart) { r.first = 1; emit(m, m, kEndFlush); }
            return;
        }
        if (r.open) { emit(from(), m, kEndMessage); r.open = 0; }
        if (kind == kMsgStart) { r.open = 1; r.first = 1; r.from = m; }
    }
    // the rest of an open capture (a message that began in this launch always delivers its first chunk here, if empty)
    SAME_HD void finish()
    {
        if (r.open) {
            const uint64_t e = real_end();
            const uint64_t a = from();
            if (has_flush()) { emit(a, e, kEndFlush); r.open = 0; }
            else if (a < e || r.first) { emit(a, e, 0u); r.from = e; }
        }
        L.rec[c] = r;
    }
};
using Walker = WalkerT<false>;

}  // namespace cap
}  // namespace same
