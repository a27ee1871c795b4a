/*
 * same_tones.h -- the tones in front of the voice message: the EAS two-tone attention signal (853 Hz and 960 Hz together) and
 * NOAA Weather Radio's 1050 Hz warning alarm tone, found on the device in the buffers a batch reads (same_rx.h) and reported
 * as events of their own that count in each channel's own samples.
 *
 * A same_tones handle watches n_channels streams at one rate.  It is a handle of its own with kernels of its own: nothing of
 * same_batch_* or same_resampler_* changes, and a batch beside it sees nothing of it.
 *
 * Arithmetic (fixed: it is the contract, and it is reproduced bit for bit -- DESIGN.md 4.13).
 *   - block length N = rate / 25 by integer division (40 ms); 8 000 <= rate <= 96 000, anything else is SAME_ERATE.
 *   - tones k = 0, 1, 2 are f_k = 853, 960 and 1050 Hz;  c_k = (float)(2.0 * cos(2.0 * pi * f_k / rate)), computed in double
 *     and rounded once;  halfN = (float)N * 0.5f;  invN = 1.0f / (float)N.
 *   - a channel's stream is cut into blocks of N samples, counted from the channel's start or last reset.  Every block starts
 *     from zero state (s1_k = s2_k = 0, E = S = 0).  For each sample x (int16 is converted to f32 exactly, with no scaling),
 *     for k = 0, 1, 2 in this order:
 *         t = c_k * s1_k;  u = t - s2_k;  s0 = x + u;  s2_k = s1_k;  s1_k = s0;
 *     then
 *         E = E + x * x;  S = S + x.
 *     Every operation is a single f32 operation, never fused (-ffp-contract=off on host and device).
 *   - at the block's last sample, for k = 0, 1, 2:
 *         a = s1*s1;  b = s2*s2;  d = c_k*s1;  e = d*s2;  P_k = (a + b) - e
 *         Em  = E - (S * S) * invN          (the block's energy without its mean)
 *         ref = Em * halfN
 *         live = Em > 0 && Em >= E * 0.015625f        (1/64, exact in f32: one multiply, one compare)
 *     the block qualifies as WAT        when  live && P_2 >= 0.5f * ref;
 *     the block qualifies as ATTENTION  when  live && P_0 >= 0.15f * ref && P_1 >= 0.15f * ref && (P_0 + P_1) >= 0.5f * ref.
 *     The mean is taken out of the energy but not out of the three sums: 853 Hz and 960 Hz make 34.12 and 38.4 cycles in a
 *     block, so a constant leaks into P_0 and P_1 (1050 Hz makes exactly 42 and does not leak).  On an idle channel -- a
 *     constant, or a constant with a few counts of noise -- Em is tiny against E, and the leak alone would pass both ATTENTION
 *     tests; `live` asks that the energy without the mean be a real share of the energy.  The limit that follows: a tone of
 *     amplitude A on a DC offset of up to 3 A still qualifies (Em / E >= 0.027); at an offset of 5 A the two-tone
 *     (Em / E = 0.0099) and at 6 A the 1050 Hz tone (0.0137) no longer do.
 *   - state machine, one per class and channel, independent of each other: active, run, miss, start.  It runs on the block
 *     index b (the block's first sample is b * N) with q = the block qualifies.
 *       not active:  q:  if run == 0, start = b * N;  run++;  if run == 25: active = 1, miss = 0, emit START with
 *                        sample_counter = start.        not q:  run = 0.
 *       active:      q:  miss = 0.                      not q:  if miss == 0, end = b * N;  miss++;  if miss == 5:
 *                        active = 0, run = 0, emit END with sample_counter = end and duration = end - start.
 *     A tone is therefore reported once it has held for 25 blocks (1 s) and ends where the first of 5 missing blocks began.
 *   - the outputs -- block values, events, counters -- do not depend on how a channel's stream is cut into calls: plain and
 *     ragged calls, f32 and int16, either layout, any mix of them on one handle.
 *
 * Events of one call.  A channel that completes n blocks in a call emits at most
 *         SAME_TONES_EVENTS_BOUND(n) = 2 * ((n + 29) / 30 + (n + 24) / 30)
 * events in it (same_tones_dev.h has the proof: per class the edges alternate, a START comes at least 25 blocks behind an END
 * and an END at least 5 behind a START, and the first edge may come with the call's first block).  Every channel has that
 * many slots of its own in the call's event storage, so no event is ever lost and none is ordered by an atomic.
 *
 * Cost.  About 20 flops per 4-byte or 2-byte sample: the pass is meant to be bound by reading the input once.  Work is
 * parallel over (64 adjacent channels, block).  Time-major: a lane is a channel, and the lanes of a wavefront read one row
 * together when their channels' block phases agree -- always so in plain calls, and in ragged calls for channels that have
 * received equal totals; channels whose phases differ read different rows, which is correct but uncoalesced.  Channel-major:
 * tiles of 64 channels x 64 samples go through on-chip memory, loaded with the lanes along time and consumed with the lanes
 * along channels, whatever the phases.  A call also copies its event slots to the host: 32 bytes per slot,
 * SAME_TONES_EVENTS_BOUND(n) slots per channel (8 for a 2-s call).  Measured figures: DESIGN.md 4.13.
 *
 * Errors are same_rx.h's codes; same_tones_last_error() has the text of the calling thread's last failure here.  A handle is
 * single-writer, and its calls run in the order they were made: give them one stream, or order the streams yourself.
 */
#ifndef SAME_TONES_H
#define SAME_TONES_H

#include <stddef.h>
#include <stdint.h>

#include "same_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct same_tones same_tones;

enum { SAME_TONE_ATTENTION = 1, SAME_TONE_WAT = 2 };          /* same_tone_event.kind */
enum { SAME_TONE_START = 1, SAME_TONE_END = 2 };              /* same_tone_event.edge */

#define SAME_TONES_MIN_RATE 8000u
#define SAME_TONES_MAX_RATE 96000u
#define SAME_TONES_START_BLOCKS 25u      /* qualifying blocks in a row before START */
#define SAME_TONES_END_BLOCKS 5u         /* missing blocks in a row before END */
#define SAME_TONES_EVENTS_BOUND(n) (2u * (((n) + 29u) / 30u + ((n) + 24u) / 30u))

typedef struct same_tone_event {
    uint32_t channel;
    uint32_t kind;            /* SAME_TONE_ATTENTION = 1, SAME_TONE_WAT = 2 */
    uint32_t edge;            /* SAME_TONE_START = 1, SAME_TONE_END = 2 */
    uint32_t reserved;        /* 0 */
    uint64_t sample_counter;  /* START: the first sample of the first of the 25 blocks; END: of the first of the 5 */
    uint64_t duration;        /* END: sample_counter - the START's sample_counter; 0 on START */
} same_tone_event;

int same_tones_new(uint32_t n_channels, uint32_t rate, int device, same_tones **out);
void same_tones_free(same_tones *th);
const char *same_tones_last_error(void);
uint32_t same_tones_n_channels(const same_tones *th);
uint32_t same_tones_rate(const same_tones *th);
uint32_t same_tones_block_length(const same_tones *th);                 /* N */
int same_tones_coefficients(const same_tones *th, float out[3]);        /* c_0, c_1, c_2 */

/* How many blocks each channel would complete in a call of these counts (NULL: every channel n_rows): block_counts, n_channels
 * entries, and their maximum, the rows d_blocks needs.  No state changes.  SAME_EINVAL: a counts[c] above n_rows. */
int same_tones_block_counts(const same_tones *th, const uint32_t *counts, size_t n_rows, uint32_t *block_counts, uint32_t *max_blocks);

/* The hot path.  d_x: DEVICE pointer, [n_rows x C] (SAME_LAYOUT_TIME_MAJOR, x[t * C + c]) or [C x n_rows]
 * (SAME_LAYOUT_CHANNEL_MAJOR, x[c * n_rows + t]), of which channel c owns its first counts[c] <= n_rows samples.  counts is a
 * HOST array, read during the call and not kept; NULL means a plain call, every channel n_rows.  Rows at or beyond counts[c]
 * are never loaded (they may hold anything, NaN included).
 *
 * d_blocks may be NULL.  Otherwise it is a DEVICE buffer [block_rows x C x 4] f32: the j-th block channel c completes in this
 * call goes to d_blocks[(j * C + c) * 4 + {0, 1, 2, 3}] = P_0, P_1, P_2, Em, and rows at or beyond block_counts[c] are never
 * written.
 *
 * SAME_EINVAL, consuming nothing and moving no counter: a null d_x with samples to read, a counts[c] above n_rows, a layout
 * that is neither of the two, block_rows below the largest block count when d_blocks is given.  With nothing to read the call
 * is a no-op.
 *
 * hip_stream is a real stream handle; NULL is the legacy default stream; there is no stream of the handle's own.  The call is
 * asynchronous and ordered on that stream: a copy of the call's per-channel descriptors, the kernels, one copy of the call's
 * event slots into pinned host memory, an event record.  The caller keeps d_x and d_blocks valid until the stream has passed
 * the call.  At most three calls are in flight: a fourth may block until the oldest has passed.
 *
 * Beside a batch: give the tone call the buffer, the counts and the stream of the batch call --
 *     same_batch_process_device(rx, d_x, n_rows, SAME_LAYOUT_TIME_MAJOR, stream);
 *     same_tones_process_device(th, d_x, n_rows, NULL, SAME_LAYOUT_TIME_MAJOR, NULL, 0, stream);
 * or, behind a resampler (same_resample.h),
 *     same_resampler_process_device(rs, d_src, n_rows, in_counts, d_y, out_rows, out_counts, stream);
 *     same_batch_process_device_ragged(rx, d_y, out_rows, out_counts, SAME_LAYOUT_TIME_MAJOR, stream);
 *     same_tones_process_device(th, d_y, out_rows, out_counts, SAME_LAYOUT_TIME_MAJOR, NULL, 0, stream);
 * -- and a tone event's sample_counter counts in the same samples as that channel's batch events and audio chunks.  A START's
 * sample_counter is where the tone began: behind the last header burst and ahead of SAME_TRANSPORT_MSG_END.  It may lie ahead
 * of SAME_TRANSPORT_MSG_START's counter, because the batch reports a message when the assembler's burst timeout (1.31 s) has
 * run out behind the last burst, and a tone may begin sooner; the sample at which the START was confirmed is sample_counter +
 * 25 N, one second later. */
int same_tones_process_device(same_tones *th, const float *d_x, size_t n_rows, const uint32_t *counts, int layout,
                              float *d_blocks, size_t block_rows, void *hip_stream);
int same_tones_process_device_i16(same_tones *th, const int16_t *d_x, size_t n_rows, const uint32_t *counts, int layout,
                                  float *d_blocks, size_t block_rows, void *hip_stream);

/* waits for every call in flight; their events are then on the host */
int same_tones_sync(same_tones *th);
/* Never blocks.  Up to cap events of the calls that have passed: calls in call order; inside a call by channel, then by the
 * block that emitted the event, then by kind.  *n_out: events written; *n_left: events on the host not yet handed out. */
int same_tones_poll(same_tones *th, same_tone_event *out, size_t cap, size_t *n_out, size_t *n_left);

/* The listed channels start again at this position of the stream -- behind every call made so far, ahead of the next: the
 * block position at 0, no open block, both state machines idle, the sample counter at 0.  A tone that is active at the reset
 * emits NO END: its START stays without a partner.  On an error (a channel out of range: SAME_EINVAL) nothing is reset.
 * Pair it with same_batch_reset_channels between the same calls. */
int same_tones_reset_channels(same_tones *th, const uint32_t *channels, size_t n);
/* samples consumed by the channel since its start or last reset (0 for a channel out of range) */
uint64_t same_tones_channel_sample_counter(const same_tones *th, uint32_t channel);

#ifdef __cplusplus
}
#endif
#endif /* SAME_TONES_H */
