"""A numpy restatement of tone-alert audio in delivery form (include/same_tone_delivery.h), derived from what the
project already trusts and reading no library of it:
  1. the float chunks of tone_audio_reference.chunks_of_calls, with the pool asked for and with a pool that has room for the
     untruncated captures (same chunks, whole samples);
  2. per capture, y = quantise(resample_reference.resample_f32(capture stream, rate, out_rate), gain);
  3. each chunk is y[ceil(a L / M) : ceil((a + n) L / M)], a = sample_counter - first, n = the chunk's placed rows.
Nothing here works per call or per tile: a chunk only selects outputs of its capture's whole delivered stream."""
import numpy as np

import resample_reference as rr
import tone_audio_reference as ar


def quantise(y, gain: float) -> np.ndarray:
    """v = y * gain in f32; nearest integer, ties to even; NaN gives 0; clamped to int16"""
    v = np.asarray(y, np.float32) * np.float32(gain)
    assert v.dtype == np.float32
    r = np.rint(v)
    r = np.where(np.isnan(v), np.float32(0), r)
    return np.clip(r, -32768, 32767).astype(np.int16)


def chunks_of_calls(streams, rate: int, out_rate: int, gain: float, calls, kinds: int, tail_blocks: int, max_blocks: int, pool: int, resets=None):
    """As tone_audio_reference.chunks_of_calls.  Returns (per call the chunks (channel, flags, kind, sample_counter, tone_start,
    out_index, int16 samples) in queue order; the captures, in the order their FIRST chunks are queued, as dicts channel, first,
    stream (float32 source samples), f32 (the delivered stream before the quantiser), y (int16))."""
    L, M, _ = rr.plan(rate, out_rate)
    room = int(sum(int(np.sum(k)) for k in calls)) + 1
    cut = ar.chunks_of_calls(streams, rate, calls, kinds, tail_blocks, max_blocks, pool, resets)
    whole = ar.chunks_of_calls(streams, rate, calls, kinds, tail_blocks, max_blocks, room, resets)
    assert [[c[:1] + c[2:5] for c in call] for call in cut] == [[c[:1] + c[2:5] for c in call] for call in whole]
    # the captures: a FIRST chunk opens its channel's capture, every later chunk of the channel continues it
    caps, cur, where = [], {}, []
    for call in whole:
        for c, flags, kind, at, tone_start, samples in call:
            assert not flags & ar.TRUNCATED
            if flags & ar.FIRST:
                cur[c] = len(caps)
                caps.append(dict(channel=c, first=at, parts=[]))
            cap = caps[cur[c]]
            assert at == cap["first"] + sum(len(p) for p in cap["parts"])       # a capture's chunks follow each other
            cap["parts"].append(samples)
            where.append(cur[c])
    memo = {}
    for cap in caps:
        cap["stream"] = np.concatenate(cap.pop("parts")).astype(np.float32)
        key = cap["stream"].tobytes()                  # (channels that carry the same stream share the work)
        if key not in memo:
            memo[key] = rr.resample_f32(cap["stream"], rate, out_rate)
        cap["f32"] = memo[key]
        cap["y"] = quantise(cap["f32"], gain)
        assert len(cap["y"]) == rr.outputs_after(len(cap["stream"]), L, M)
    out, i = [], 0
    for call in cut:
        chunks = []
        for c, flags, kind, at, tone_start, samples in call:
            cap = caps[where[i]]
            i += 1
            a, n = at - cap["first"], len(samples)
            n0, n1 = rr.outputs_after(a, L, M), rr.outputs_after(a + n, L, M)
            chunks.append((c, flags, kind, at, tone_start, n0, cap["y"][n0:n1]))
        out.append(chunks)
    return out, caps
