// same_tone_delivery_dev.h -- tone-alert audio in delivery form (include/same_tone_delivery.h) as __host__ __device__ code: no
// heap, no STL.  Which outputs a chunk delivers, how a tile of outputs is cut and what its input window holds, one output's sum
// and the quantiser, and the history a call leaves behind are one text for the device (same_tone_delivery.hip) and for a plain
// C++ compiler, where tests/helpers/tone_delivery_main.cpp holds them against the numpy reference
// (tests/helpers/tone_delivery_reference.py) under ASan + UBSan.
//
// The contract.  A capture's source stream is s[i] = the channel's sample first + i, zero for i < 0; output n of
// its delivered stream is the resampler's (same_resample_dev.h) on those clocks, then quantised.  A chunk whose placed rows are
// s[a .. a + n) delivers the outputs whose newest source sample k = floor(n M / L) lies in [a, a + n).  By the chunk proof of
// same_tone_audio_dev.h a chunk either begins at `first` (FIRST: a == 0, everything before it is zero) or at its channel's row 0
// of the call, with the capture open on entry: then a and the T - 1 source samples before it are what history_step() left
// behind the call before.  There is no third case.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "same_resample_dev.h"
#include "same_tone_audio_dev.h"

namespace same {
namespace td {

struct Params { uint32_t L, M, T, rate; float gain; };

constexpr uint32_t kTileOutputs = 256;        // outputs of one tile: the lanes of a workgroup
// source samples a tile's outputs read: the newest of output i lies floor((p0 + i M) / L) behind that of output 0, p0 < L and
// M / L <= 6 (T <= rs::kMaxT), so the last of 256 lies at most 255 * 6 + 1 further; T - 1 more in front
constexpr uint32_t kWindowMax = (kTileOutputs - 1) * 6 + 1 + rs::kMaxT;

// what a chunk delivers, beside its tn::Span in the call's records
struct Out {
    uint64_t a;               // capture-local index of the chunk's first placed row
    uint64_t out_index;       // its first output: ceil(a L / M)
    uint64_t n_out;           // ceil((a + n) L / M) - out_index
    uint64_t off;             // among the channel's delivered samples of the call; behind out_place: in the call's delivery pool
};
static_assert(sizeof(Out) == 32, "output records are copied to the host as they are");

// The quantiser: one f32 multiply, round to nearest even, NaN -> 0, clamp.
SAME_HD inline int16_t quantise(float acc, float gain)
{
    const float v = acc * gain;
    if (!(v == v)) return 0;
    const float r = __builtin_rintf(v);       // (the rounding mode is the default one on both sides: to nearest, ties to even)
    if (r < -32768.0f) return (int16_t)-32768;
    if (r > 32767.0f) return (int16_t)32767;
    return (int16_t)(int32_t)r;
}

// The outputs of the placed span s (behind tn::span_place: s.n is what got room).  a_entry: the capture-local index of the
// channel's row 0 of this call, left by history_step() of the call before; looked at only for a chunk that is not FIRST.
// `before`: the channel's delivered samples of the call in front of this chunk.
SAME_HD inline Out out_of(const tn::Span &s, uint64_t a_entry, const Params &p, uint64_t before)
{
    const uint64_t a = (s.flags & SAME_TONE_AUDIO_FIRST) ? 0 : a_entry;
    const uint64_t n0 = rs::outputs_after(a, p.L, p.M);
    return Out{a, n0, rs::outputs_after(a + s.n, p.L, p.M) - n0, before};
}

// Tile t of a chunk: its outputs out_index + t * 256 + [0, n), the phase of the first, and the window of source samples they
// read, s[k0 - (T - 1) .. k0 - (T - 1) + W), as indices of the capture's stream.
struct Tile { uint64_t k0; uint32_t p0, n, W; };
SAME_HD inline Tile tile_of(const Out &o, uint32_t t, const Params &p)
{
    const uint64_t done = (uint64_t)t * kTileOutputs, left = o.n_out - done;
    const rs::Phase ph = rs::phase_of(o.out_index + done, p.L, p.M);
    Tile tl;
    tl.k0 = ph.k;
    tl.p0 = ph.p;
    tl.n = left < kTileOutputs ? (uint32_t)left : kTileOutputs;
    // (p0 + 255 M < 1024 + 255 * 6144 < 2^21)
    tl.W = (tl.p0 + (tl.n - 1) * p.M) / p.L + p.T;
    return tl;
}

// Entry i of tile tl's window: s[k0 - (T - 1) + i].  Every output of the chunk has k in [a, a + n), so the window lies in
// [a - (T - 1), a + n): rows of the chunk come from the staging pool (s.off: the chunk's place in it), what lies before it from
// the channel's history (hist[q] = s[a - (T - 1) + q]), or is zero for a FIRST chunk.
SAME_HD inline float window_at(const tn::Span &s, const Out &o, const Tile &tl, uint32_t i, uint32_t T, const float *pool, const float *hist)
{
    const uint64_t at = tl.k0 + i;                 // s index + (T - 1)
    const uint64_t lo = o.a + (T - 1);
    if (at >= lo) return pool[s.off + (at - lo)];
    if (s.flags & SAME_TONE_AUDIO_FIRST) return 0.0f;
    return hist[at - o.a];                         // (at >= a: k0 >= a)
}

// Output i (< tl.n) of the tile from its window w: the resampler's sum in the resampler's order, with the [j][p] table.
SAME_HD inline int16_t tile_output(const float *w, const float *taps_t, const Params &p, const Tile &tl, uint32_t i)
{
    const uint32_t q = tl.p0 + i * p.M;
    const float *wk = w + (p.T - 1) + q / p.L;     // s[k]
    const float *h = taps_t + q % p.L;
    float acc = 0.0f;
    SAME_RS_UNROLL8
    for (uint32_t j = 0; j < p.T; ++j) acc = acc + h[(size_t)j * p.L] * wk[-(ptrdiff_t)j];
    return quantise(acc, p.gain);
}

// What a call leaves behind for the next one, per channel, behind the call's state-machine kernel (cap: the capture state
// behind the call): if a capture is open, *a_next = the capture-local index of the next call's row 0, and hist = the last T - 1
// source samples of the capture, oldest first, taken from the call's input x (x[r * xs]: the channel's row r) -- never from the
// pool.  A capture that was open on entry (first < pos) has run through the whole call: rs::update_history's shifting rule
// over all count rows.  One that opened in this call has the rows [first - pos, count): zeros first, then those.
template <typename SampleT>
SAME_HD inline void history_step(const tn::Desc &d, const tn::Cap &cap, uint32_t N, uint32_t T, const SampleT *x, size_t xs, float *hist,
                                 size_t hs, uint64_t *a_next)
{
    if (!cap.open || d.count == 0) return;
    const uint64_t pos = d.block0 * N + d.fill;
    *a_next = pos + d.count - cap.first;
    if (T == 1) return;
    if (cap.first < pos) { rs::update_history(hist, hs, T, x, xs, d.count); return; }
    const uint64_t r0 = cap.first - pos;           // (<= count: a capture begins behind a block the call completed)
    for (uint32_t i = 0; i + 1 < T; ++i) hist[(size_t)i * hs] = 0.0f;
    if (r0 < d.count) rs::update_history(hist, hs, T, x + (size_t)r0 * xs, xs, (uint32_t)(d.count - r0));
}

}  // namespace td
}  // namespace same
