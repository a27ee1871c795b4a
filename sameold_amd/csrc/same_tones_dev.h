// same_tones_dev.h -- the arithmetic of the tone detector (include/same_tones.h) as __host__ __device__ code: no heap, no STL.
// The per-sample step, the end-of-block arithmetic and the state machine are one text for the device (same_tones.hip) and
// for a plain C++ compiler, where tests/helpers/tones_main.cpp holds them bit for bit against the numpy reference
// (tests/helpers/tones_reference.py) under ASan + UBSan.
//
// The contract.  A channel's stream is cut into blocks of N = rate / 25 samples; every block starts from a
// zero Acc and takes its samples through step() in order; finish() turns the Acc behind the block's last sample into P_0, P_1,
// P_2, Em and the two qualify bits; sm_step() runs one class's state machine over one block.  Only a channel's open block
// carries an Acc from call to call.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/same_tones.h"

#if defined(__HIPCC__)
#define SAME_HD __host__ __device__
#else
#define SAME_HD
#endif

namespace same {
namespace tn {

constexpr uint32_t kBlocksPerSecond = 25;
constexpr uint32_t kStartBlocks = SAME_TONES_START_BLOCKS, kEndBlocks = SAME_TONES_END_BLOCKS;
constexpr double kToneHz[3] = {853.0, 960.0, 1050.0};
constexpr float kWatShare = 0.5f, kAttnEachShare = 0.15f, kAttnSumShare = 0.5f;
constexpr float kLiveShare = 0.015625f;                   // 1/64: a block is live only when Em is at least this share of E
constexpr uint32_t kQAttention = 1u, kQWat = 2u;          // the qualify bits of a block

// what a rate fixes
struct Coef { float c[3]; float halfN, invN; uint32_t N; };

// the Goertzel state of three tones, the block's energy and its sum
struct Acc { float s1[3], s2[3], E, S; };
constexpr uint32_t kAccWords = 8;                          // an open block's Acc on the device: word w of channel c at [w * C + c]

SAME_HD inline Acc acc_zero()
{
    Acc a;
    for (int k = 0; k < 3; ++k) { a.s1[k] = 0.0f; a.s2[k] = 0.0f; }
    a.E = 0.0f; a.S = 0.0f;
    return a;
}

// one sample
SAME_HD inline void step(Acc &a, const Coef &cf, float x)
{
    for (int k = 0; k < 3; ++k) {
        const float t = cf.c[k] * a.s1[k];
        const float u = t - a.s2[k];
        const float s0 = x + u;
        a.s2[k] = a.s1[k];
        a.s1[k] = s0;
    }
    a.E = a.E + x * x;
    a.S = a.S + x;
}

struct BlockOut { float P[3], Em; uint32_t q; };

// behind the block's last sample
SAME_HD inline BlockOut finish(const Acc &acc, const Coef &cf)
{
    BlockOut o;
    for (int k = 0; k < 3; ++k) {
        const float a = acc.s1[k] * acc.s1[k];
        const float b = acc.s2[k] * acc.s2[k];
        const float d = cf.c[k] * acc.s1[k];
        const float e = d * acc.s2[k];
        o.P[k] = (a + b) - e;
    }
    o.Em = acc.E - (acc.S * acc.S) * cf.invN;
    const float ref = o.Em * cf.halfN;
    // (a constant leaks into P_0 and P_1 -- 34.12 and 38.4 cycles per block -- and on an idle channel Em is LSB noise or rounding
    // residue, far below E: without the second test a muted channel with a DC offset qualifies as ATTENTION in every block)
    const bool live = o.Em > 0.0f && o.Em >= acc.E * kLiveShare;
    const bool wat = live && o.P[2] >= kWatShare * ref;
    const bool attn = live && o.P[0] >= kAttnEachShare * ref && o.P[1] >= kAttnEachShare * ref && (o.P[0] + o.P[1]) >= kAttnSumShare * ref;
    o.q = (attn ? kQAttention : 0u) | (wat ? kQWat : 0u);
    return o;
}

// one class's state machine of one channel
struct Sm { uint64_t start, end; uint32_t active, run, miss, pad; };
static_assert(sizeof(Sm) == 32, "two state machines per 64-byte line");

SAME_HD inline Sm sm_zero() { return Sm{0, 0, 0, 0, 0, 0}; }

// Block b of the channel qualifies (q) or does not.  Returns 1 and fills *ev when the block emits an event, else 0.
SAME_HD inline uint32_t sm_step(Sm &s, bool q, uint64_t b, uint32_t N, uint32_t channel, uint32_t kind, same_tone_event *ev)
{
    if (!s.active) {
        if (!q) { s.run = 0; return 0; }
        if (s.run == 0) s.start = b * N;
        s.run++;
        if (s.run < kStartBlocks) return 0;
        s.active = 1; s.miss = 0;
        *ev = same_tone_event{channel, kind, SAME_TONE_START, 0, s.start, 0};
        return 1;
    }
    if (q) { s.miss = 0; return 0; }
    if (s.miss == 0) s.end = b * N;
    s.miss++;
    if (s.miss < kEndBlocks) return 0;
    s.active = 0; s.run = 0;
    *ev = same_tone_event{channel, kind, SAME_TONE_END, 0, s.end, s.end - s.start};
    return 1;
}

// Events one channel can emit while it completes n blocks, both classes together: SAME_TONES_EVENTS_BOUND(n).
//
// Proof, for one class.  An edge is emitted only by sm_step: START only when not active, and it sets active; END only when
// active, and it clears active: the edges of a class alternate.  After a START miss is 0, and an END needs miss == 5, one
// increment per block: an END comes at least 5 blocks behind the START before it.  After an END run is 0, and a START needs
// run == 25, one increment per block: a START comes at least 25 blocks behind the END before it.  Number a call's completed
// blocks 1 .. n.  Whatever the state at block 1, the call's first edge lies at block >= 1.  If it is a START, the i-th START of
// the call lies at block >= 1 + 30 (i - 1) and the i-th END at >= 6 + 30 (i - 1): at most floor((n + 29) / 30) STARTs and
// floor((n + 24) / 30) ENDs.  If it is an END, the i-th END lies at >= 1 + 30 (i - 1) and the i-th START at >= 26 + 30 (i - 1):
// floor((n + 29) / 30) + floor((n + 4) / 30), which is no more.  The first case is met with equality by a channel that enters
// the call not active with run == 24 and sees q = 1, then 5 times 0, then 25 times 1, and so on
// (tests/helpers/tones_main.cpp runs it).  The two classes are independent: twice that.
SAME_HD inline uint32_t events_bound(uint32_t n) { return SAME_TONES_EVENTS_BOUND(n); }

// a call's counts and event slots, on the device and in a slot's pinned copy: n_channels counts, padded to 32 bytes, then the events
SAME_HD inline size_t events_offset(uint32_t n_channels) { return (((size_t)n_channels * sizeof(uint32_t)) + 31) / 32 * 32; }

// a channel's part of one call (same_tones_plan.h fills it)
struct Desc {
    uint64_t block0;          // index of the first block the call touches, counted from the channel's start or last reset
    uint32_t fill;            // samples that block already holds: > 0 means the call's block 0 continues the saved open block
    uint32_t count;           // samples of the call that are the channel's
    uint32_t n_touch;         // blocks the call touches: ceil((fill + count) / N), 0 when count == 0
    uint32_t n_complete;      // blocks the call completes: (fill + count) / N; the blocks 0 .. n_complete-1 of the call
    uint32_t ev_off;          // the channel's first event slot of the call; it owns events_bound(n_complete) slots
    uint32_t flags;           // kDescClear | kDescBank
};
static_assert(sizeof(Desc) == 32, "two descriptors per 64-byte line");
constexpr uint32_t kDescClear = 1u;       // the channel was reset: its state machines are idle in front of this call
constexpr uint32_t kDescBank = 2u;        // which of the two Acc banks holds the channel's open block (the call saves to the other)

// the rows [r0, r1) of the call that belong to block j (< n_touch) of the channel
SAME_HD inline void block_rows(const Desc &d, uint32_t N, uint32_t j, uint32_t &r0, uint32_t &r1)
{
    // (j N - fill <= count < 2^32: no wrap)
    r0 = j == 0 ? 0u : j * N - d.fill;
    const uint64_t end = (uint64_t)(j + 1) * N - d.fill;
    r1 = end < d.count ? (uint32_t)end : d.count;
}
SAME_HD inline bool block_continues(const Desc &d, uint32_t j) { return j == 0 && d.fill != 0; }
SAME_HD inline bool block_completes(const Desc &d, uint32_t j) { return j < d.n_complete; }

SAME_HD inline Acc acc_load(const float *bank, size_t C, uint32_t c)
{
    Acc a;
    for (int k = 0; k < 3; ++k) { a.s1[k] = bank[(size_t)k * C + c]; a.s2[k] = bank[(size_t)(3 + k) * C + c]; }
    a.E = bank[(size_t)6 * C + c]; a.S = bank[(size_t)7 * C + c];
    return a;
}
SAME_HD inline void acc_store(float *bank, size_t C, uint32_t c, const Acc &a)
{
    for (int k = 0; k < 3; ++k) { bank[(size_t)k * C + c] = a.s1[k]; bank[(size_t)(3 + k) * C + c] = a.s2[k]; }
    bank[(size_t)6 * C + c] = a.E; bank[(size_t)7 * C + c] = a.S;
}

// The rows [r0, r1) of one channel, x[r * xs], through step().  Eight loads are issued ahead of the eight serial steps that
// consume them, so that a lane has several rows in flight; the order of the steps is the stream's.
template <typename SampleT>
SAME_HD inline void run_rows(Acc &a, const Coef &cf, const SampleT *x, size_t xs, uint32_t r0, uint32_t r1)
{
    uint32_t r = r0;
    for (; r + 8 <= r1; r += 8) {
        float v[8];
        for (int i = 0; i < 8; ++i) v[i] = (float)x[(size_t)(r + i) * xs];
        for (int i = 0; i < 8; ++i) step(a, cf, v[i]);
    }
    for (; r < r1; ++r) step(a, cf, (float)x[(size_t)r * xs]);
}

// What the end of block j of the channel leaves: the block's values and qualify bits when it completes, the Acc in the bank
// the call saves to when it stays open.  blocks may be null.
SAME_HD inline void block_end(const Desc &d, const Coef &cf, uint32_t j, const Acc &a, uint32_t c, size_t C, float *blocks, uint8_t *qual,
                              float *bank_out)
{
    if (block_completes(d, j)) {
        const BlockOut o = finish(a, cf);
        if (blocks) {
            float *p = blocks + ((size_t)j * C + c) * 4;
            p[0] = o.P[0]; p[1] = o.P[1]; p[2] = o.P[2]; p[3] = o.Em;
        }
        qual[(size_t)j * C + c] = (uint8_t)o.q;
    } else {
        acc_store(bank_out, C, c, a);
    }
}

// Both state machines of one channel over the blocks the call completed.  ev: the call's event slots; returns the events
// written, at most events_bound(d.n_complete), into ev[d.ev_off ...] -- by block, then by kind.
SAME_HD inline uint32_t run_state_machines(const Desc &d, uint32_t N, uint32_t c, size_t C, const uint8_t *qual, Sm *sm /* [2] */,
                                           same_tone_event *ev)
{
    if (d.flags & kDescClear) { sm[0] = sm_zero(); sm[1] = sm_zero(); }
    const uint32_t cap = events_bound(d.n_complete);
    uint32_t n = 0;
    for (uint32_t j = 0; j < d.n_complete; ++j) {
        const uint32_t q = qual[(size_t)j * C + c];
        same_tone_event e;
        if (sm_step(sm[0], (q & kQAttention) != 0, d.block0 + j, N, c, SAME_TONE_ATTENTION, &e) && n < cap) ev[d.ev_off + n++] = e;
        if (sm_step(sm[1], (q & kQWat) != 0, d.block0 + j, N, c, SAME_TONE_WAT, &e) && n < cap) ev[d.ev_off + n++] = e;
    }
    return n;
}

}  // namespace tn
}  // namespace same
