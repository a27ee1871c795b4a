// same_transport_dev.h -- the transport layer of same_transport.h/.cpp restated as __host__ __device__ code: no heap, no STL,
// no function pointers.  One lane per channel runs it on the device (same_transport.hip) for SAME_BATCH_MESSAGES_ONLY batches;
// the same text compiles with a plain C++ compiler, where tests/helpers/device_transport_fuzz.cpp holds it against
// same::TransportRef event for event.
//
// Citations: file:line under crates/sameold/src/ ("rx/" = receiver/) unless a crate is named -- rx/assembler.rs:154-234,
// 294-346, 362-376 (Assembler), rx/combiner.rs:32-80, 154-273 (combine), receiver.rs:291-333 (process_transportlayer),
// crates/sameplace/src/message.rs:718-736, 813-828 (Message::try_from, the header check).
//
// What the host version does eight bytes at a time (combine's bit votes, parse_message's sums) is done here byte by byte:
// the results are the same (tests/test_host_sanitizers.py::test_combine_equals_the_byte_walk), and a lane's scalar loop
// over a burst is what the device does well.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/same_rx.h"

#if defined(__HIPCC__)
#define SAME_HD __host__ __device__
#else
#define SAME_HD
#endif

namespace same {
namespace dt {

constexpr uint32_t kTick = 8;                        // device transport wake-up (same::kDevTick)
constexpr uint32_t kMsgLen = 268;                    // MAX_MESSAGE_LENGTH rx/assembler.rs:70
constexpr uint64_t kMaxInterburstSymbols = 682;      // rx/assembler.rs:85 ((1.05 * 520.83 + 17 * 8) as u64 in f32)
constexpr uint64_t kMaxHistoryDuration = 5652;       // rx/assembler.rs:92-93 (2 * (682 + 8 * 268))
constexpr uint64_t kMaxMessageDurationSecs = 135;    // receiver.rs:496

// Result<Message, MessageDecodeErr> with its header text in place
struct Msg {
    uint32_t kind, err, len;                         // SAME_TRANSPORT_MSG_*; 1 NotAscii, 2 UnrecognizedPrefix, 3 Malformed; header length
    uint32_t offset_time, parity_errors, voting_bytes;
    uint8_t text[kMsgLen + 4];
};
struct Burst { uint32_t len; uint8_t data[kMsgLen]; };

// A channel's state: the HOT record (one cache line: everything a poll that changes nothing touches) and the COLD one
// (burst bytes and message texts, touched when a burst arrives or a message state begins or ends) -- the layout of
// same::TransportHot / TransportCold
struct alignas(64) Hot {
    uint32_t state_kind;
    uint8_t have_force_eom, dirty, have_polled, nhist, pending, have_prev, pad_[2];
    uint64_t force_eom_at;
    uint64_t last_polled_symbol;
    uint64_t hist_deadline[3];
    uint64_t pend_deadline;
};
static_assert(sizeof(Hot) == 64, "one cache line per channel");
struct Cold {
    uint64_t prev_deadline;
    Burst history[3];
    Msg pend, prev, state_msg;
};

// A transport event (receiver.rs:256-265): what on_link_event reports when the transport state changes
struct Event {
    uint32_t kind, len, aux, aux2;                   // aux: MSG_START voting bytes, MSG_ERR error code; aux2: MSG_START parity errors
    uint64_t sample_counter, symbol_count;
    const uint8_t *text;                             // MSG_START: the header (len bytes), valid until the next call on the channel
};

SAME_HD inline void copy_bytes(uint8_t *d, const uint8_t *s, uint32_t n) { for (uint32_t i = 0; i < n; ++i) d[i] = s[i]; }
SAME_HD inline void clear_msg(Msg &m) { m.kind = 0; m.err = 0; m.len = 0; m.offset_time = 0; m.parity_errors = 0; m.voting_bytes = 0; }
// (a copy moves the header fields and the live text bytes, not the whole buffer)
SAME_HD inline void copy_msg(Msg &d, const Msg &s)
{
    d.kind = s.kind; d.err = s.err; d.len = s.len; d.offset_time = s.offset_time; d.parity_errors = s.parity_errors; d.voting_bytes = s.voting_bytes;
    copy_bytes(d.text, s.text, s.len <= kMsgLen ? s.len : kMsgLen);
}
SAME_HD inline bool equal_msg(const Msg &a, const Msg &b)
{
    if (a.kind != b.kind || a.err != b.err || a.len != b.len || a.offset_time != b.offset_time ||
        a.parity_errors != b.parity_errors || a.voting_bytes != b.voting_bytes) return false;
    for (uint32_t i = 0; i < a.len; ++i) if (a.text[i] != b.text[i]) return false;
    return true;
}
// Message::as_str(): the header text, or "NNNN" for EndOfMessage (sameplace message.rs:105-110); duplicates are string-equal
SAME_HD inline bool same_text(const Msg &a, const Msg &b)
{
    const bool ea = a.kind == SAME_TRANSPORT_MSG_END, eb = b.kind == SAME_TRANSPORT_MSG_END;
    if (ea || eb) return ea && eb;                    // (a header is never "NNNN": it begins "ZCZC-")
    if (a.len != b.len) return false;
    for (uint32_t i = 0; i < a.len; ++i) if (a.text[i] != b.text[i]) return false;
    return true;
}

SAME_HD inline bool is_alpha(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
SAME_HD inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// rx/combiner.rs:105-137
SAME_HD inline bool is_allowed(uint8_t c)
{
    if (is_alpha(c) || is_digit(c)) return true;
    switch (c) {
    case '-': case '/': case '?': case '(': case ')': case '[': case ']': case '.': case '_': case ',': case '+': case ' ':
        return true;
    default:
        return false;
    }
}
SAME_HD inline uint32_t popcount8(uint8_t x) { uint32_t n = 0; for (; x; x &= (uint8_t)(x - 1u)) ++n; return n; }

// crates/sameplace/src/message.rs:813-828: ^ZCZC-[[:alpha:]]{3}-[[:alpha:]]{3}(-[0-9]{6})+(\+[0-9]{4}-[0-9]{7}-.{3,8}-)
// (the location group is greedy and the next group begins with '+': giving back a repetition never helps; .{3,8} is greedy)
SAME_HD inline bool check_header(const uint8_t *h, uint32_t n, uint32_t *offset_time, uint32_t *hdr_len)
{
    auto at = [&](uint32_t i, uint8_t c) { return i < n && h[i] == c; };
    auto alphas = [&](uint32_t i, uint32_t k) { for (uint32_t j = 0; j < k; ++j) if (i + j >= n || !is_alpha(h[i + j])) return false; return true; };
    auto digits = [&](uint32_t i, uint32_t k) { for (uint32_t j = 0; j < k; ++j) if (i + j >= n || !is_digit(h[i + j])) return false; return true; };
    if (n < 5 || h[0] != 'Z' || h[1] != 'C' || h[2] != 'Z' || h[3] != 'C' || h[4] != '-') return false;
    uint32_t p = 5;
    if (!alphas(p, 3) || !at(p + 3, '-') || !alphas(p + 4, 3)) return false;
    p += 7;
    uint32_t nloc = 0;
    while (at(p, '-') && digits(p + 1, 6)) { p += 7; ++nloc; }
    if (!nloc) return false;
    const uint32_t g2 = p;
    if (!at(p, '+') || !digits(p + 1, 4) || !at(p + 5, '-') || !digits(p + 6, 7) || !at(p + 13, '-')) return false;
    p += 14;
    for (uint32_t m = 8; m >= 3; --m) {
        if (!at(p + m, '-')) continue;
        bool ok = true;
        for (uint32_t k = 0; k < m; ++k) if (h[p + k] == '\n') { ok = false; break; }
        if (ok) { *offset_time = g2; *hdr_len = p + m + 1; return true; }
    }
    return false;
}

// Message::try_from((bytes, errs, counts)) crates/sameplace/src/message.rs:718-736, 184-230
SAME_HD inline void parse_message(const uint8_t *b, uint32_t n, const uint8_t *errs, const uint8_t *counts, Msg &out)
{
    clear_msg(out);
    for (uint32_t i = 0; i < n; ++i)
        if (b[i] & 0x80u) { out.kind = SAME_TRANSPORT_MSG_ERR; out.err = 1; return; }
    if (n >= 5 && b[0] == 'Z' && b[1] == 'C' && b[2] == 'Z' && b[3] == 'C' && b[4] == '-') {
        uint32_t off = 0, hl = 0;
        if (!check_header(b, n, &off, &hl)) { out.kind = SAME_TRANSPORT_MSG_ERR; out.err = 3; return; }
        out.kind = SAME_TRANSPORT_MSG_START;
        out.len = hl;
        copy_bytes(out.text, b, hl);
        out.offset_time = off;
        uint32_t pe = 0, vb = 0;
        for (uint32_t i = 0; i < hl; ++i) { pe += errs[i]; vb += counts[i] >= 3 ? 1u : 0u; }
        out.parity_errors = pe; out.voting_bytes = vb;
    } else if (n >= 2 && b[0] == 'N' && b[1] == 'N') {
        out.kind = SAME_TRANSPORT_MSG_END;
    } else {
        out.kind = SAME_TRANSPORT_MSG_ERR; out.err = 2;
    }
}

// combine() rx/combiner.rs:32-80 over up to three bursts, with estimate_message :154-203, the bit votes :216-249, the fast
// end-of-message :251-258 and truncate_bytes_with_reference :264-273; false = None
SAME_HD inline bool combine(const Burst *bursts, uint32_t nbursts, Msg &res)
{
    uint8_t msg[kMsgLen], cnt[kMsgLen], errs[kMsgLen];
    const uint32_t nb = nbursts < 3u ? nbursts : 3u;
    uint32_t n = 0;
    for (; n < kMsgLen; ++n) {
        uint8_t cur[3];
        uint32_t k = 0;
        bool msb = false;
        for (uint32_t i = 0; i < nb; ++i)
            if (n < bursts[i].len) { const uint8_t x = bursts[i].data[n]; msb |= (x & 0x80u) != 0; cur[k++] = (uint8_t)(x & 0x7fu); }
        if (k == 0) break;
        uint8_t est;
        uint32_t be = 0;
        if (k == 1) {
            est = cur[0];
        } else if (k == 2) {
            const uint8_t x = (uint8_t)(cur[0] ^ cur[1]);      // bit_vote_detect :216-222
            est = x ? 0 : cur[0];
            be = popcount8(x);
        } else {
            const uint8_t p0 = (uint8_t)~(cur[0] ^ cur[1]), p1 = (uint8_t)~(cur[1] ^ cur[2]), p2 = (uint8_t)~(cur[0] ^ cur[2]);
            est = (uint8_t)((cur[0] & p0) | (cur[2] & p1) | (cur[2] & p2));      // bit_vote_correct :234-249
            be = 8u - popcount8((uint8_t)(p0 & p1 & p2));
        }
        if (!is_allowed(est)) break;
        msg[n] = est; cnt[n] = (uint8_t)k; errs[n] = (uint8_t)(be + (msb ? 1u : 0u));
    }
    if (n == 0) return false;
    uint32_t good = 0;
    while (good < n && cnt[good] >= 2) ++good;
    parse_message(msg, good, errs, cnt, res);
    if (res.kind != SAME_TRANSPORT_MSG_ERR) return true;
    if (n >= 2 && msg[0] == 'N' && msg[1] == 'N') { clear_msg(res); res.kind = SAME_TRANSPORT_MSG_END; return true; }
    return good != 0;
}

// The Assembler (rx/assembler.rs:108-266) and the transport state of SameReceiver (receiver.rs:79, 85, 89, 291-333) of one
// channel; `msg` is the caller's scratch (a stack object on the host, a lane's private memory on the device)
struct Transport {
    Hot &h;
    Cold &c;

    SAME_HD void reset()
    {
        h.nhist = 0; h.pending = 0; h.have_prev = 0;
        h.state_kind = SAME_TRANSPORT_IDLE; clear_msg(c.state_msg);
        h.have_force_eom = 0; h.dirty = 1;
        h.have_polled = 0; h.last_polled_symbol = 0;
    }
    // force_eom_at_sample (receiver.rs:89), 0 = None
    SAME_HD uint64_t force_eom_at() const { return h.have_force_eom ? h.force_eom_at : 0; }
    SAME_HD bool force_eom_dirty() { const bool d = h.dirty != 0; h.dirty = 0; return d; }
    // a ragged launch left the channel `by` samples further behind the batch's counter: an armed instant (batch sample
    // coordinates) moves with it; true if there was one
    SAME_HD bool shift_force_eom(uint64_t by) { if (!h.have_force_eom || !by) return false; h.force_eom_at += by; return true; }

    // rx/assembler.rs:362-368: retain unexpired entries, then keep at most the two newest
    SAME_HD void prune_history(uint64_t now)
    {
        uint32_t w = 0;
        for (uint32_t i = 0; i < h.nhist; ++i)
            if (!(h.hist_deadline[i] <= now)) {
                if (w != i) { c.history[w].len = c.history[i].len; copy_bytes(c.history[w].data, c.history[i].data, c.history[i].len); h.hist_deadline[w] = h.hist_deadline[i]; }
                ++w;
            }
        h.nhist = (uint8_t)w;
        while (h.nhist > 2) {
            for (uint32_t i = 1; i < h.nhist; ++i) {
                c.history[i - 1].len = c.history[i].len; copy_bytes(c.history[i - 1].data, c.history[i].data, c.history[i].len);
                h.hist_deadline[i - 1] = h.hist_deadline[i];
            }
            --h.nhist;
        }
    }
    // PendingResult::accept rx/assembler.rs:294-328
    SAME_HD void accept(const Msg &m, uint64_t now)
    {
        const uint64_t deadline = (m.kind == SAME_TRANSPORT_MSG_END) ? now : now + kMaxInterburstSymbols;
        bool replace = true;
        if (h.pending) {
            if (c.pend.kind == SAME_TRANSPORT_MSG_ERR) replace = true;
            else if (c.pend.kind == SAME_TRANSPORT_MSG_END && m.kind == SAME_TRANSPORT_MSG_START) replace = true;
            else if (c.pend.kind == SAME_TRANSPORT_MSG_START && m.kind == SAME_TRANSPORT_MSG_START) replace = m.voting_bytes >= c.pend.voting_bytes;
            else replace = false;
        }
        if (replace) { h.pending = 1; copy_msg(c.pend, m); h.pend_deadline = deadline; }
    }
    // rx/assembler.rs:205-234 with PendingResult::poll :336-345; the TransportState kind, *msg filled for Message states
    SAME_HD uint32_t idle(uint64_t now, Msg &msg)
    {
        if (h.nhist > 2 || (h.nhist && h.hist_deadline[0] <= now)) prune_history(now);
        if (h.pending && h.pend_deadline <= now) {
            copy_msg(msg, c.pend);
            h.pending = 0;
            if (msg.kind != SAME_TRANSPORT_MSG_ERR) { h.have_prev = 1; copy_msg(c.prev, msg); c.prev_deadline = now + kMaxHistoryDuration; }
            return msg.kind;
        }
        return h.nhist == 0 ? SAME_TRANSPORT_IDLE : SAME_TRANSPORT_ASSEMBLING;
    }
    // rx/assembler.rs:154-184, the deduplication :245-265 and prune_previous :371-376
    SAME_HD uint32_t assemble(const uint8_t *burst, uint32_t n, uint64_t now, Msg &msg)
    {
        if (n == 0) return idle(now, msg);
        prune_history(now);
        if (h.have_prev && c.prev_deadline <= now) h.have_prev = 0;
        h.hist_deadline[h.nhist] = now + kMaxHistoryDuration;
        Burst &t = c.history[h.nhist++];                 // at most 2 survive the prune
        t.len = n < kMsgLen ? n : kMsgLen;
        copy_bytes(t.data, burst, t.len);
        if (combine(c.history, h.nhist, msg)) {
            const bool dup = msg.kind != SAME_TRANSPORT_MSG_ERR && h.have_prev && same_text(c.prev, msg);
            if (!dup) accept(msg, now);
        }
        return idle(now, msg);
    }

    // process_transportlayer receiver.rs:291-333 at one device event (link event or wake-up tick) of this channel, in order.
    // Returns true and fills *out when the transport state changed (receiver.rs:256-265).
    SAME_HD bool on_link_event(uint32_t kind, uint64_t sample_counter, uint64_t symbol_count, const uint8_t *bytes, uint32_t len,
                               uint32_t input_rate, Msg &msg, Event *out)
    {
        // the reference polls once per symbol: a wake-up on the symbol of the event just handled does not poll again
        if (kind == kTick && h.have_polled && symbol_count == h.last_polled_symbol) return false;
        if (kind == SAME_LINK_BURST || kind == SAME_LINK_NO_CARRIER || kind == kTick) { h.have_polled = 1; h.last_polled_symbol = symbol_count; }
        uint32_t st;
        if (kind == SAME_LINK_BURST) {
            st = assemble(bytes, len, symbol_count, msg);
        } else if (kind == SAME_LINK_NO_CARRIER || kind == kTick) {
            if (h.have_force_eom && sample_counter > h.force_eom_at) { st = SAME_TRANSPORT_MSG_END; clear_msg(msg); msg.kind = st; }
            else st = idle(symbol_count, msg);
        } else {
            return false;
        }
        if (st == SAME_TRANSPORT_MSG_START) {
            h.have_force_eom = 1; h.dirty = 1;
            h.force_eom_at = sample_counter + kMaxMessageDurationSecs * (uint64_t)input_rate;
        } else if (st == SAME_TRANSPORT_MSG_END) {
            if (h.have_force_eom) h.dirty = 1;
            h.have_force_eom = 0;
        }
        const bool is_msg = st >= SAME_TRANSPORT_MSG_START;
        if (st == h.state_kind && (!is_msg || equal_msg(msg, c.state_msg))) return false;
        const bool was_msg = h.state_kind >= SAME_TRANSPORT_MSG_START;
        h.state_kind = st;
        if (is_msg) copy_msg(c.state_msg, msg); else if (was_msg) clear_msg(c.state_msg);
        out->kind = st; out->len = 0; out->aux = 0; out->aux2 = 0; out->text = nullptr;
        out->sample_counter = sample_counter;
        out->symbol_count = symbol_count;
        if (st == SAME_TRANSPORT_MSG_START) {
            out->len = msg.len; out->aux = msg.voting_bytes; out->aux2 = msg.parity_errors; out->text = c.state_msg.text;
        } else if (st == SAME_TRANSPORT_MSG_ERR) {
            out->aux = msg.err;
        }
        return true;
    }
};

}  // namespace dt
}  // namespace same
