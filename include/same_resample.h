/*
 * same_resample.h -- mixed-rate sources for a batch: a device resampler that takes every channel from its own source rate
 * to one output rate, the batch's, and writes exactly what a ragged call takes (same_batch_process_device_ragged, same_rx.h):
 * a time-major buffer and per-channel counts.
 *
 * A batch is n_channels receivers built from one builder, so it runs at one input rate; sources do not (web streams at 44.1
 * or 48 kHz, telephony and scanner feeds at 8, 11.025 or 16 kHz, archives at 32 kHz).  The resampler is a handle of its own
 * with kernels of its own: nothing of same_batch_* changes, and a batch fed through it sees an ordinary ragged call.
 *
 * Arithmetic (fixed: it is the contract, and it is reproduced bit for bit -- DESIGN.md 4.11).  Channel c has source rate r_in,
 * the handle one output rate r_out; g = gcd(r_in, r_out), L = r_out / g, M = r_in / g.
 *   - L == M == 1: T = 1, the tap is 1.0f; the channel passes through with its bits unchanged and no delay.
 *   - otherwise T = 2 ceil(8 max(1, M / L)) taps per phase, from a Kaiser-windowed sinc of n = T L points computed in double and
 *     rounded once to f32:  w = 2 * 0.45 * min(r_in, r_out) / (L r_in),  ctr = (n - 1) / 2,
 *         h[i] = L w sinc(w (i - ctr)) I0(8.6 sqrt(1 - ((i - ctr) / (n / 2))^2)) / I0(8.6),   sinc(x) = sin(pi x) / (pi x),
 *     stored [phase p][tap j] = h[p + j L].
 *   - output n of the channel's stream, counted from its start or last reset:  k = floor(n M / L),  p = (n M) mod L,
 *         acc = 0.0f;  for j = 0 .. T-1 in this order:  acc = acc + h[p][j] * x[k - j]
 *     one f32 multiply and one f32 add per tap, never fused; x[i] = 0 for i < 0; int16 input is converted to f32 exactly first.
 *   - after N source samples in total exactly ceil(N L / M) outputs exist; a call produces the difference to the total before
 *     it.  The outputs do not depend on how the stream is cut into calls; positions are 64-bit (streams of 2^40 samples).
 *   - the output stream lags the source by (T L - 1) / (2 M) output samples: 8.27 for 48 kHz -> 22.05 kHz, 22.05 for 8 kHz.
 *   - SAME_ERATE: L > 1024 or T > 96 (96 kHz -> 22.05 kHz, T = 70, is accepted; 192 kHz is not).  SAME_EINVAL: more than 16
 *     distinct ratios in one handle, resets with new rates included.
 *
 * Errors are same_rx.h's codes; same_resampler_last_error() has the text of the calling thread's last failure here.  A handle
 * is single-writer: the caller orders the calls of one handle among themselves.
 */
#ifndef SAME_RESAMPLE_H
#define SAME_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "same_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct same_resampler same_resampler;

/* in_rates: n_channels source rates in Hz */
int same_resampler_new(uint32_t n_channels, const uint32_t *in_rates, uint32_t out_rate, int device, same_resampler **out);
void same_resampler_free(same_resampler *rs);
const char *same_resampler_last_error(void);
uint32_t same_resampler_n_channels(const same_resampler *rs);
uint32_t same_resampler_out_rate(const same_resampler *rs);

/* the channel's ratio and taps per phase (any of L, M, T may be NULL) */
int same_resampler_plan(const same_resampler *rs, uint32_t channel, uint32_t *L, uint32_t *M, uint32_t *T);
/* the channel's taps, [p][j], T * L floats: *n = T * L; written when out != NULL and cap >= T * L (else SAME_EINVAL with *n set) */
int same_resampler_taps(const same_resampler *rs, uint32_t channel, float *out, size_t cap, size_t *n);
/* (T L - 1) / (2 M): output samples by which the channel's output lags its source; an event of the batch at sample counter s
 * lies at source sample (s - delay) * M / L.  Negative for a channel out of range. */
double same_resampler_delay(const same_resampler *rs, uint32_t channel);

/* What a process call with these in_counts would produce: out_counts[c] per channel and their maximum, the rows d_y needs.
 * No state changes.  in_counts and out_counts: n_channels entries. */
int same_resampler_out_counts(const same_resampler *rs, const uint32_t *in_counts, uint32_t *out_counts, uint32_t *max_out);

/* The hot path.  d_x: DEVICE pointer, time-major [n_rows x C] (x[t * C + c]), of which channel c owns its first in_counts[c]
 * <= n_rows rows; rows at or beyond in_counts[c] are never loaded (they may hold anything, NaN included).  in_counts is a HOST
 * array, read during the call and not kept.  d_y: DEVICE pointer, time-major [out_rows x C] f32; channel c's
 * out_counts[c] (written to the host array out_counts) outputs go to its first rows, and rows at or beyond out_counts[c] are
 * never written.  In this call a lane is a channel, so only time-major rows coalesce; sources that lie each in a buffer of
 * their own (channel-major input included) go through same_resampler_process_device_sources below.
 *
 * SAME_EINVAL, consuming nothing and moving no counter: out_rows below the largest output count, an in_counts[c] above n_rows,
 * a null pointer.  With in_counts all zero the call is a no-op (out_counts are zero).
 *
 * hip_stream is a real stream handle; NULL is the legacy default stream; there is no stream of the handle's own.  The call is
 * asynchronous and ordered on that stream (a copy of the call's per-channel descriptors, then the kernels).  The caller keeps
 * d_x and d_y valid until the stream has passed the call.  The host may block when three calls are already in flight.
 *
 * Feeding a batch at out_rate:
 *     same_resampler_process_device(rs, d_x, n_rows, in_counts, d_y, out_rows, out_counts, stream);
 *     same_batch_process_device_ragged(rx, d_y, out_rows, out_counts, SAME_LAYOUT_TIME_MAJOR, stream);
 * on the same stream -- or on SAME_STREAM_OWN after same_batch_order_after(rx, stream).  d_y then falls under the batch's
 * input-lifetime contract (same_rx.h, "Stream contract").  The batch's events count in output samples. */
int same_resampler_process_device(same_resampler *rs, const float *d_x, size_t n_rows, const uint32_t *in_counts,
                                  float *d_y, size_t out_rows, uint32_t *out_counts, void *hip_stream);
int same_resampler_process_device_i16(same_resampler *rs, const int16_t *d_x, size_t n_rows, const uint32_t *in_counts,
                                      float *d_y, size_t out_rows, uint32_t *out_counts, void *hip_stream);

/* Per-source calls: every channel from its own device buffer, at its own rate and of its own length.  d_src is a HOST array
 * of n_channels DEVICE pointers, read during the call and not kept, like in_counts; d_src[c] points at in_counts[c] contiguous
 * samples, the channel's next ones, aligned to the sample type (4 bytes for f32, 2 for int16).  Nothing outside
 * [d_src[c], d_src[c] + in_counts[c]) is ever loaded -- not the sample before the buffer, none behind it -- and d_src[c] may be
 * NULL where in_counts[c] == 0.  A [C x n_rows] channel-major matrix is the case d_src[c] = base + c * n_rows.
 *
 * The output is the time-major call's: d_y[n * C + c], out_counts[c] rows per channel, rows at or beyond out_counts[c] never
 * written, ready for same_batch_process_device_ragged(..., SAME_LAYOUT_TIME_MAJOR, ...).  So is the arithmetic, bit for bit:
 * the outputs depend neither on how the stream is cut into calls nor on which of the two kinds of call delivered a sample.
 * Both kinds may be mixed freely on one handle: they share the channels' clocks and histories, and
 * same_resampler_reset_channels acts between them as between time-major calls.
 *
 * SAME_EINVAL, consuming nothing and moving no counter: a null d_src, in_counts or out_counts; a NULL d_src[c] with
 * in_counts[c] > 0; a d_src[c] (of a channel with samples) not aligned to its sample type; out_rows below the largest output
 * count.  With in_counts all zero the call is a no-op.
 *
 * Stream and lifetimes as above: asynchronous and ordered on hip_stream (a copy of the descriptors and of the pointers, then
 * the kernels); the caller keeps every source buffer and d_y valid until the stream has passed the call; the host may block
 * when three calls are already in flight.
 *
 * Which call when.  Here a wavefront works on one channel with its lanes along the output samples, so a channel's rate, tap
 * count and table are the same in every lane and its reads are one contiguous stretch: the cost does not grow with the number
 * of rates that neighbouring channels mix.  Use it whenever sources arrive as buffers of their own (interleaving them first
 * costs more than either call), and whenever neighbouring channels differ in rate: with seven rates interleaved channel by
 * channel it took 22 ms where the time-major call took 112 ms (32 768 channels, 2-s calls, f32, one MI355X).
 * Groups of 64 adjacent channels at one rate are cheaper still here, as in the time-major call: such a group reads its tap
 * table from on-chip memory.  With every channel at 48 kHz this call took 17.5 ms and the time-major call 28 ms; with every
 * channel at 8 kHz the time-major call was the faster one, 7 ms against 13 ms, and it remains right for a producer that
 * already holds a time-major matrix with one rate per group of 64 channels. */
int same_resampler_process_device_sources(same_resampler *rs, const float *const *d_src, const uint32_t *in_counts,
                                          float *d_y, size_t out_rows, uint32_t *out_counts, void *hip_stream);
int same_resampler_process_device_sources_i16(same_resampler *rs, const int16_t *const *d_src, const uint32_t *in_counts,
                                              float *d_y, size_t out_rows, uint32_t *out_counts, void *hip_stream);

/* The listed channels start again at this position of the stream -- behind every call made so far, ahead of the next: clocks
 * at 0 and an empty (zero) history, which a small kernel in front of the next call's kernels clears on that call's stream.
 * new_rates: NULL keeps the channels' rates, otherwise n source rates, one per entry of channels.  On an error (a channel out
 * of range: SAME_EINVAL; SAME_ERATE; a 17th ratio: SAME_EINVAL) nothing is reset.  May wait for the calls in flight when a
 * rate never seen by the handle needs its taps on the device.  Pair it with same_batch_reset_channels between the same calls. */
int same_resampler_reset_channels(same_resampler *rs, const uint32_t *channels, size_t n, const uint32_t *new_rates);
/* source samples consumed / outputs produced by the channel since its start or last reset (0 for a channel out of range) */
uint64_t same_resampler_channel_input_counter(const same_resampler *rs, uint32_t channel);
uint64_t same_resampler_channel_output_counter(const same_resampler *rs, uint32_t channel);

#ifdef __cplusplus
}
#endif
#endif /* SAME_RESAMPLE_H */
