// same_resample_dev.h -- the per-output arithmetic of the mixed-rate resampler (include/same_resample.h) as
// __host__ __device__ code: no heap, no STL.  One lane per channel runs it on the device (same_resample.hip), or, in a
// per-source call, one lane per output row of one channel; the same text compiles with a plain C++ compiler, where
// tests/helpers/resample_plan_main.cpp and resample_sources_main.cpp hold it bit for bit against the numpy reference
// (tests/helpers/resample_reference.py) under ASan + UBSan.
//
// The contract.  A channel converts r_in to r_out with L = r_out / g, M = r_in / g, g = gcd, through T taps per
// phase, stored [phase p][tap j].  Output n of the channel's stream reads the source from k = floor(n M / L) downwards with the
// taps of phase p = (n M) mod L:
//     acc = 0.0f;  for j = 0 .. T-1:  acc = acc + h[p][j] * x[k - j]
// one f32 multiply and one f32 add per tap (-ffp-contract=off), x[i] = 0 for i < 0.  L == M == 1 has T == 1 and hands x[k] over
// with its bits unchanged.  After N source samples exactly ceil(N L / M) outputs exist; a call that begins at clocks
// (n_in, n_out) therefore has k >= n_in for every output it makes and reads no further back than x[n_in - (T - 1)]: the
// channel's history, the last T - 1 source samples of the calls before, oldest first in its own column.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAME_HD __host__ __device__
#else
#define SAME_HD
#endif

#if defined(__HIPCC__)
#define SAME_RS_UNROLL8 _Pragma("unroll 8")
#else
#define SAME_RS_UNROLL8
#endif

namespace same {
namespace rs {

constexpr uint32_t kMaxL = 1024;              // phases: beyond it SAME_ERATE
constexpr uint32_t kMaxT = 96;                // taps per phase: beyond it SAME_ERATE
constexpr uint32_t kMaxRatios = 16;           // distinct (L, M) of one handle: beyond it SAME_EINVAL
constexpr uint32_t kHistRows = kMaxT - 1;     // rows of the history buffer (a channel uses its first T - 1)

// one distinct ratio; its taps are taps[tap_off + p * T + j]
struct Ratio { uint32_t L, M, T, tap_off; };

// a channel's part of one call: its clocks before the call and what the call gives and takes
struct Desc {
    uint64_t n_in, n_out;                     // source samples consumed / outputs made before this call
    uint32_t in_count, out_count;             // rows of x that are the channel's; outputs the call makes
    uint32_t ratio;                           // index of the channel's Ratio
    uint32_t clear;                           // 1: the channel was reset, its history is zeroed in front of this call
};
static_assert(sizeof(Desc) == 32, "two descriptors per 64-byte line");

// where output n reads: the newest source sample k and the phase p
struct Phase { uint64_t k; uint32_t p; };
// n M < 2^64: n <= N L / M + 1 with N the source samples, so n M <= N L + M, and N = 2^40 with L = 1024 is 2^50
SAME_HD inline Phase phase_of(uint64_t n, uint32_t L, uint32_t M)
{
    const uint64_t nm = n * (uint64_t)M;
    return Phase{nm / L, (uint32_t)(nm % L)};
}
// phase_of(n + 1) from phase_of(n)
SAME_HD inline void advance(Phase &ph, uint32_t L, uint32_t M)
{
    ph.k += M / L;
    ph.p += M % L;
    if (ph.p >= L) { ph.p -= L; ph.k += 1; }
}

// outputs that exist after n_in source samples: ceil(n_in L / M)
SAME_HD inline uint64_t outputs_after(uint64_t n_in, uint32_t L, uint32_t M) { return (n_in * (uint64_t)L + (M - 1)) / M; }

// One output.  `taps`: the T taps of its phase.  `rel` = k - n_in >= 0: the newest source sample it reads, as a row of this
// call's x (x[r * xs] is row r of the channel, hist[i * hs] the source sample n_in - (T - 1) + i).
template <typename SampleT>
SAME_HD inline float eval(const float *taps, uint32_t T, uint64_t rel, const SampleT *x, size_t xs, const float *hist, size_t hs)
{
    if (T == 1) return (float)x[rel * xs];
    if (rel + 1 >= (uint64_t)T) {
        // every tap reads this call's rows (all but a call's first outputs).  Unrolled so that a lane has several loads in
        // flight; the sum keeps its order.
        const SampleT *xk = x + rel * xs;
        float acc = 0.0f;
        SAME_RS_UNROLL8
        for (uint32_t j = 0; j < T; ++j) acc = acc + taps[j] * (float)xk[-(ptrdiff_t)((size_t)j * xs)];
        return acc;
    }
    const uint32_t jx = (uint32_t)(rel + 1);                                   // taps 0 .. jx-1 read this call's rows
    float acc = 0.0f;
    for (uint32_t j = 0; j < jx; ++j) acc = acc + taps[j] * (float)x[(rel - j) * xs];
    // tap j >= jx reads source sample n_in + rel - j = n_in - (T - 1) + (T - 1 + rel - j)
    for (uint32_t j = jx; j < T; ++j) acc = acc + taps[j] * hist[(size_t)(T - 1 + (uint32_t)rel - j) * hs];
    return acc;
}

// The outputs [row0, row1) of one channel's call, as far as the call makes them: y[row * ys] for row < d.out_count.
template <typename SampleT>
SAME_HD inline void lane_rows(const Desc &d, const Ratio &r, const float *taps, const SampleT *x, size_t xs, const float *hist, size_t hs,
                              float *y, size_t ys, uint32_t row0, uint32_t row1)
{
    if (row1 > d.out_count) row1 = d.out_count;
    if (row0 >= row1) return;
    Phase ph = phase_of(d.n_out + row0, r.L, r.M);
    const float *h = taps + r.tap_off;
    for (uint32_t row = row0; row < row1; ++row) {
        y[(size_t)row * ys] = eval(h + (size_t)ph.p * r.T, r.T, ph.k - d.n_in, x, xs, hist, hs);
        advance(ph, r.L, r.M);
    }
}

// The history behind a call of m = in_count rows: the channel's last T - 1 source samples, oldest first.  A short call shifts
// what is there -- upwards through the column, every row read before it is written -- and appends its rows.
template <typename SampleT>
SAME_HD inline void update_history(float *hist, size_t hs, uint32_t T, const SampleT *x, size_t xs, uint32_t m)
{
    const uint32_t H = T - 1;
    if (m >= H) {
        for (uint32_t i = 0; i < H; ++i) hist[(size_t)i * hs] = (float)x[(size_t)(m - H + i) * xs];
        return;
    }
    for (uint32_t i = 0; i + m < H; ++i) hist[(size_t)i * hs] = hist[(size_t)(i + m) * hs];
    for (uint32_t q = 0; q < m; ++q) hist[(size_t)(H - m + q) * hs] = (float)x[(size_t)q * xs];
}

// ---- Per-source calls: a channel's samples are its own unit-stride buffer, and the lanes of a wavefront are
// consecutive output rows of ONE channel.  Ratio, T and the tap table are then the same in every lane, and lanes differ in
// phase; the taps are read from a second copy of the table stored [tap j][phase p] (taps_t[j * L + p] == taps[p * T + j]), in
// which the phases of one tap step are neighbours.

// phase_of(n + i) from ph0 = phase_of(n), for 0 <= i < 64, in 32-bit arithmetic: (n + i) M = k0 L + p0 + i M, and
// p0 + i M < L + 63 M <= 1024 + 63 * 6144 < 2^19 (T <= kMaxT bounds M / L <= 6, so M <= 6 kMaxL).
SAME_HD inline Phase lane_phase(const Phase &ph0, uint32_t i, uint32_t L, uint32_t M)
{
    const uint32_t q = ph0.p + i * M;
    return Phase{ph0.k + q / L, q % L};
}

// eval for a unit-stride source and the [j][p] table: `taps_p` = taps_t + p, tap j at taps_p[j * L].  The same sums in the same
// order; x[0 .. rel] are the only samples of the source it loads.
template <typename SampleT>
SAME_HD inline float eval_source(const float *taps_p, uint32_t L, uint32_t T, uint64_t rel, const SampleT *x, const float *hist, size_t hs)
{
    if (T == 1) return (float)x[rel];
    if (rel + 1 >= (uint64_t)T) {
        const SampleT *xk = x + rel;
        float acc = 0.0f;
        SAME_RS_UNROLL8
        for (uint32_t j = 0; j < T; ++j) acc = acc + taps_p[(size_t)j * L] * (float)xk[-(ptrdiff_t)j];
        return acc;
    }
    const uint32_t jx = (uint32_t)(rel + 1);                                   // taps 0 .. jx-1 read this call's buffer
    float acc = 0.0f;
    for (uint32_t j = 0; j < jx; ++j) acc = acc + taps_p[(size_t)j * L] * (float)x[rel - j];
    for (uint32_t j = jx; j < T; ++j) acc = acc + taps_p[(size_t)j * L] * hist[(size_t)(T - 1 + (uint32_t)rel - j) * hs];
    return acc;
}

// The outputs [row0, row1) of one channel's per-source call, row1 - row0 <= 64, as far as the call makes them: lane i takes
// row row0 + i into y[i * ys].  A wavefront calls it with (lane, 64), a host loop with (0, 1); either way one 64-bit phase_of
// per call, every row's phase from it.  `x`: the channel's in_count samples of this call; `taps_t`: the [j][p] tables.
template <typename SampleT>
SAME_HD inline void source_rows(const Desc &d, const Ratio &r, const float *taps_t, const SampleT *x, const float *hist, size_t hs,
                                float *y, size_t ys, uint32_t row0, uint32_t row1, uint32_t lane, uint32_t lanes)
{
    if (row1 > d.out_count) row1 = d.out_count;
    if (row0 >= row1) return;
    const Phase ph0 = phase_of(d.n_out + row0, r.L, r.M);
    const float *h = taps_t + r.tap_off;
    for (uint32_t i = lane; i < row1 - row0; i += lanes) {
        const Phase ph = lane_phase(ph0, i, r.L, r.M);
        y[(size_t)i * ys] = eval_source(h + ph.p, r.L, r.T, ph.k - d.n_in, x, hist, hs);
    }
}

// The history behind a per-source call: update_history on the channel's own buffer.  Nothing of x is loaded when m == 0.
template <typename SampleT>
SAME_HD inline void update_history_source(float *hist, size_t hs, uint32_t T, const SampleT *x, uint32_t m)
{
    if (m == 0 || T == 1) return;
    update_history(hist, hs, T, x, 1, m);
}

}  // namespace rs
}  // namespace same
