/*
 * same_tone_audio.h -- tone alert: the audio that follows a tone, captured on the device beside any kind of batch.
 *
 * A same_tones handle (same_tones.h) reports that a tone happened, one second after it began -- when the caller's buffer may
 * be gone.  With capture on, the handle also copies what follows a confirmed tone out of the buffers its process calls read,
 * while they are still the library's to read, as a weather radio unmutes on the tone and stays open for the voice message.
 * Nothing of same_tones.h changes: there is no new process entry point, same_tones_process_device(_i16) queue the extra work
 * on the caller's stream behind the state machines and inside the same call, and the caller's obligation to keep d_x valid
 * until the stream has passed the call is what it was.  With capture off a call queues exactly what it queued before.
 *
 * Contract (fixed, bit for bit, and independent of how a stream is cut into calls -- DESIGN.md 4.14).  Captures are made of
 * whole blocks of N = rate / 25 samples.  Every channel has, beside its two tone state machines, a capture state
 *     open, kind, len, left, first, tone_start.
 * Block b of a channel is captured if and only if open is set at its first sample.  Decisions fall at the end of each
 * completed block b, behind both tone state machines' steps of that block, with started = the enabled kinds that emitted
 * START in block b and act = some enabled kind is active behind block b:
 *     if (open) { len += 1;
 *                 if (act) left = tail_blocks;
 *                 else if (left == 0) close(END_TAIL);
 *                 else left -= 1;
 *                 if (open && len == max_blocks) close(END_MAX); }
 *     else if (started) { open = 1; kind = lowest enabled kind in started; tone_start = that class's start;
 *                         first = (b + 1) * N; len = 0; left = tail_blocks; }
 *   - a single tone is captured as [start + 25 N, end + (5 + tail_blocks) N), cut short at max_blocks blocks.  The capture
 *     begins behind the block that confirmed the tone, because that block may have begun in a call whose input is gone.
 *   - a START of an enabled kind while a capture is open re-arms the tail; the capture goes on under its first kind and
 *     tone_start.
 *   - after END_MAX a new capture needs a new START.
 *   - a channel reset by same_tones_reset_channels enters its next call with the capture state zero: an open capture is
 *     dropped with no END flag, as a tone that is active at a reset emits no END.
 *
 * Chunks.  Per call and channel, the chunks are the maximal runs of captured rows.  SAME_TONE_AUDIO_FIRST marks the chunk that
 * begins at `first`; SAME_TONE_AUDIO_END_TAIL or _END_MAX the chunk that holds the capture's last sample, which always has at
 * least one sample.  int16 input is delivered converted exactly, with no scaling.  Chunks are queued in call order, and inside
 * a call by channel, then by sample_counter.  The concatenation of a capture's chunks does not depend on the cut of the calls,
 * on plain or ragged calls, on the layout, or on f32 against int16 of the same integer values.
 * A channel that completes n blocks in a call has at most SAME_TONE_AUDIO_CHUNK_BOUND(n) chunks in it (the proof is in
 * sameold_amd/csrc/same_tone_audio_dev.h) and owns that many chunk slots of the call: none is lost, none ordered by an atomic.
 *
 * The pool.  A call has room for samples_per_call captured samples.  Room is handed out in channel order, then in stream
 * order, by a prefix sum over the channels' captured counts.  A pool that fills truncates the same chunks on every run: the
 * first chunk that does not fit is cut (it alone has fewer samples than its run), later chunks of the call carry 0 samples,
 * and all of them are marked SAME_TONE_AUDIO_TRUNCATED.  The capture state goes on regardless.
 *
 * How the samples travel, and the memory.  same_tone_audio_set allocates three pools of samples_per_call floats on the device,
 * one per call that can be in flight, 32 bytes of capture state per channel and one flag per 64 channels.  A call copies its
 * chunk records (48 bytes per slot, 4 bytes per channel and a 16-byte header that holds the pool's use) to pinned host memory
 * with its event slots.  Samples are copied lazily: a call that has passed and used u > 0 samples of its pool has those u
 * floats copied to a host block of the handle -- by same_tone_audio_peek, or by the process call that is about to reuse the
 * pool -- on a stream of the handle's own, so that the copy never waits for a call in flight.  A call in which no channel
 * captures moves no sample bytes to the host, and no call copies pool capacity instead of pool use.  A host block lives until
 * its last chunk has been dropped.
 */
#ifndef SAME_TONE_AUDIO_H
#define SAME_TONE_AUDIO_H

#include <stddef.h>
#include <stdint.h>

#include "same_tones.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SAME_TONE_AUDIO_FIRST = 1,
    SAME_TONE_AUDIO_END_TAIL = 2,     /* no enabled tone was active for tail_blocks blocks more */
    SAME_TONE_AUDIO_END_MAX = 4,      /* the capture reached max_blocks blocks */
    SAME_TONE_AUDIO_TRUNCATED = 8     /* the call's pool was full: n_samples is below the run's length */
};

#define SAME_TONE_AUDIO_CHUNK_BOUND(n) (1u + ((n) + 28u) / 30u + ((n) + 26u) / 30u)

typedef struct same_tone_audio_chunk {
    uint32_t channel, flags;
    uint32_t kind;               /* SAME_TONE_ATTENTION or SAME_TONE_WAT: the tone that opened the capture */
    uint32_t reserved;           /* 0 */
    uint64_t sample_counter;     /* the channel's counter of samples[0], in the samples of its tone events */
    uint64_t n_samples;
    uint64_t tone_start;         /* the sample_counter of the START that opened the capture */
    const float *samples;        /* handle-owned */
} same_tone_audio_chunk;

/* kinds: a mask of SAME_TONE_ATTENTION | SAME_TONE_WAT, non-zero; tail_blocks >= 0; max_blocks >= 1; samples_per_call: the pool
 * of one call, 0 turns capture off (the other arguments are then not looked at).  Allowed only before the handle's first sample
 * (SAME_EINVAL behind it, and for a mask or max_blocks out of range).  The pools are allocated here, so that running out of
 * memory fails here (SAME_ENOMEM, capture is then off). */
int same_tone_audio_set(same_tones *th, uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, size_t samples_per_call);

/* As same_batch_peek_audio / same_batch_drop_audio.  peek: *chunks points at the *n queued chunks of the calls that have passed;
 * the view and every `samples` pointer in it stay valid until the next same_tone_audio_peek or same_tone_audio_drop of the
 * handle.  It may wait for the copy of the used part of a passed call's pool; it never waits for a call in flight
 * (same_tones_sync first to include those).  drop: the first n chunks of the view leave the queue. */
int same_tone_audio_peek(same_tones *th, const same_tone_audio_chunk **chunks, size_t *n);
int same_tone_audio_drop(same_tones *th, size_t n);

/* SAME_TONE_AUDIO_CHUNK_BOUND(n_blocks): the chunks, and chunk slots, of a channel in a call in which it completes n_blocks */
uint32_t same_tone_audio_chunk_bound(uint32_t n_blocks);

#ifdef __cplusplus
}
#endif
#endif /* SAME_TONE_AUDIO_H */
