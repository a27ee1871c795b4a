/*
 * same_tone_delivery.h -- tone-alert audio in delivery form: what follows a tone as 16-bit PCM at a voice rate, decimated and
 * quantised on the device.
 *
 * same_tone_audio.h hands the captured audio out as f32 at the batch's rate.  What follows a tone is a voice announcement, and
 * storage, relay and speech recognition want it at a voice rate in s16le; once more than a few channels capture, the call is
 * bound by the samples' way to the host.  A handle in delivery mode runs the resampler's arithmetic (same_resample.h, DESIGN.md
 * 4.11) behind the capture on the device and moves int16 at out_rate to the host: 22 050 Hz f32 -> 8 000 Hz int16 is 0.181 of
 * the bytes.  Nothing of same_tones.h or same_tone_audio.h changes; a handle that does not ask for delivery queues what it
 * queued before.
 *
 * Contract (fixed, bit for bit, and independent of how a stream is cut into calls -- DESIGN.md 4.15).
 * What is captured, and how it is split, is same_tone_audio.h's: the capture state machine, the rows that are captured, the
 * chunks (one per maximal run of captured rows of a call), their flags, their order, their bound and the pool rule.
 * samples_per_call counts captured SOURCE samples: room is handed out and cut exactly as there, so a chunk is
 * SAME_TONE_AUDIO_TRUNCATED exactly when the float path would mark it so, and its placed rows are the float chunk's samples.
 *
 * A capture's source stream is s[i], the channel's sample first + i, with s[i] = 0 for i < 0.  Its delivered stream follows the
 * resampler's contract on capture-local clocks.  With g = gcd(rate, out_rate), L = out_rate / g, M = rate / g, and T taps per
 * phase from the resampler's design (T = 2 ceil(8 M / L); a Kaiser window, beta 8.6, on a sinc cut at 0.45 out_rate, designed
 * in double and rounded once to f32), output n reads from k = floor(n M / L) downwards with the taps of phase p = (n M) mod L:
 *     acc = 0.0f;  for j = 0 .. T-1:  acc = acc + h[p][j] * s[k - j]
 * one f32 multiply and one f32 add per tap, never contracted.  Then the quantiser:
 *     v = acc * gain               one f32 multiply
 *     r = v rounded to the nearest integer, ties to even; NaN gives 0; clamped to [-32768, 32767]
 * out_rate == rate has T == 1 and the one tap 1.0: with gain == 1 an int16 input comes back unchanged.
 *
 * A chunk whose placed rows are the capture-local source samples [a, a + n) delivers the outputs
 *     [ceil(a L / M), ceil((a + n) L / M))
 * -- those whose newest source sample k lies in [a, a + n) -- and out_index is the first of them.  The concatenation of a
 * capture's chunks is its delivered stream from output 0 on, with no gap and no overlap, whatever the cut.  A chunk can have
 * zero samples (n < M / L), also the chunk that carries an END flag; it is still queued.  The delivered stream lags the source
 * by (T L - 1) / (2 M) outputs, and the filter's last tail is not flushed: the outputs that would read beyond the capture's
 * last sample do not exist.
 * A capture's filter history (its last T - 1 source samples) is always taken from the call's input, not from what got room in
 * the pool: after a truncated chunk, later chunks are what they would have been without the truncation.  A channel reset by
 * same_tones_reset_channels drops its history with its capture state.
 *
 * Memory, and how the samples travel.  same_tone_delivery_set allocates, per call that can be in flight (three), a staging pool
 * of samples_per_call floats -- the float path's pool, which in delivery mode never leaves the device -- and a delivery pool of
 * samples_per_call int16: L <= M, so a call delivers no more samples than it placed rows, and chunks are packed with no padding.
 * Beside them T - 1 floats and 8 bytes per channel (the history and the capture-local clock), the taps (T L floats) and the
 * float path's per-channel state.  A call copies its chunk records (80 bytes per slot) with its event slots.  Delivered samples
 * are copied lazily, as the float path's are: only the used part of a passed call's delivery pool, 2 bytes per delivered
 * sample, on a stream of the handle's own, into pinned host blocks that are recycled through a free list once their last chunk
 * has been dropped.
 */
#ifndef SAME_TONE_DELIVERY_H
#define SAME_TONE_DELIVERY_H

#include <stddef.h>
#include <stdint.h>

#include "same_tone_audio.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct same_tone_delivery_chunk {      /* 56 bytes */
    uint32_t channel, flags;                   /* flags: SAME_TONE_AUDIO_* */
    uint32_t kind;                             /* the tone that opened the capture */
    uint32_t rate;                             /* out_rate */
    uint64_t sample_counter;                   /* of the run's first captured source sample, as same_tone_audio_chunk's */
    uint64_t out_index;                        /* index of samples[0] in the capture's delivered stream */
    uint64_t n_samples;
    uint64_t tone_start;
    const int16_t *samples;                    /* handle-owned */
} same_tone_delivery_chunk;

/* In place of same_tone_audio_set, and under its rules: allowed only before the handle's first sample (SAME_EINVAL behind it);
 * SAME_EINVAL for a mask that is empty or names another kind, for max_blocks == 0, for a gain that is not finite and positive,
 * for out_rate == 0 or above the handle's rate; SAME_ERATE for a ratio the resampler refuses (more than 1024 phases or 96 taps:
 * 96 000 -> 8 000 would need 192).  samples_per_call == 0 turns capture off (the other arguments are then not looked at).
 * All device memory is allocated here (SAME_ENOMEM, capture is then off).  The last of same_tone_audio_set and
 * same_tone_delivery_set decides the handle's mode.  In delivery mode same_tone_audio_peek reports no chunks; on any other
 * handle same_tone_delivery_peek reports none. */
int same_tone_delivery_set(same_tones *th, uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, size_t samples_per_call,
                           uint32_t out_rate, float gain);

/* As same_tone_audio_peek / same_tone_audio_drop.  peek: *chunks points at the *n queued chunks of the calls that have passed;
 * the view and every `samples` pointer in it stay valid until the next same_tone_delivery_peek or same_tone_delivery_drop of
 * the handle.  It may wait for the copy of the used part of a passed call's delivery pool; it never waits for a call in flight
 * (same_tones_sync first to include those).  drop: the first n chunks of the view leave the queue. */
int same_tone_delivery_peek(same_tones *th, const same_tone_delivery_chunk **chunks, size_t *n);
int same_tone_delivery_drop(same_tones *th, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* SAME_TONE_DELIVERY_H */
