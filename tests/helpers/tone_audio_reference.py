"""A numpy restatement of tone-alert audio's contract (include/same_tone_audio.h).  It reads no library of the
project: the capture state machine runs over the qualify bits and the tone state machines of tones_reference.py, every stream
gets a per-sample answer to "is this sample captured, and by which capture", and a list of calls is cut out of that by slicing.
Nothing here works per call: a call only selects rows."""
import numpy as np

import tones_reference as tr

FIRST, END_TAIL, END_MAX, TRUNCATED = 1, 2, 4, 8
END = END_TAIL | END_MAX

CHUNK_DTYPE = np.dtype([("channel", "<u4"), ("flags", "<u4"), ("kind", "<u4"), ("reserved", "<u4"), ("sample_counter", "<u8"),
                        ("n_samples", "<u8"), ("tone_start", "<u8"), ("samples", "<u8")])


def chunk_bound(n: int) -> int:
    return 1 + (n + 28) // 30 + (n + 26) // 30


def captures_of_bits(attn, wat, N: int, kinds: int, tail_blocks: int, max_blocks: int):
    """The capture state machine over a stream's blocks: a list of captures {first, end, kind, tone_start, flag}, in samples
    counted from the stream's start.  end is None (and flag 0) for a capture that is still open behind the last whole block."""
    ch = tr.Channel(0, N)
    out, cur = [], None
    for b, (qa, qw) in enumerate(zip(attn, wat)):
        events = ch.feed([qa], [qw])
        started = [e[1] for e in events if e[2] == tr.START and (e[1] & kinds)]
        act = any(ch.sm[k].active for k in (tr.ATTENTION, tr.WAT) if k & kinds)
        if cur is not None:
            cur["len"] += 1
            flag = 0
            if act:
                cur["left"] = tail_blocks
            elif cur["left"] == 0:
                flag = END_TAIL
            else:
                cur["left"] -= 1
            if not flag and cur["len"] == max_blocks:
                flag = END_MAX
            if flag:
                out.append(dict(first=cur["first"], end=(b + 1) * N, kind=cur["kind"], tone_start=cur["tone_start"], flag=flag))
                cur = None
        elif started:
            kind = min(started)
            cur = dict(first=(b + 1) * N, kind=kind, tone_start=ch.sm[kind].start, len=0, left=tail_blocks)
    if cur is not None:
        out.append(dict(first=cur["first"], end=None, kind=cur["kind"], tone_start=cur["tone_start"], flag=0))
    return out


def captures_of_stream(x, rate: int, kinds: int, tail_blocks: int, max_blocks: int):
    """captures_of_bits of one whole stream (1-D), with `samples`: the float32 slice of the stream, to its end for an open one"""
    N = tr.block_length(rate)
    vals, E = tr.blocks_f32(x, rate, True)
    attn, wat = tr.qualify_f32(vals, rate, E)
    caps = captures_of_bits(attn, wat, N, kinds, tail_blocks, max_blocks)
    for c in caps:
        c["samples"] = np.asarray(x[c["first"]:c["end"]]).astype(np.float32)
    return caps


def chunks_of_calls(streams, rate: int, calls, kinds: int, tail_blocks: int, max_blocks: int, pool: int, resets=None):
    """streams: [C, samples]; calls: a list of per-channel counts; resets: {call index: channels reset in front of that call}.
    Returns, per call, the chunks (channel, flags, kind, sample_counter, tone_start, float32 samples) in queue order, cut by a
    pool of `pool` samples per call as the contract has it."""
    C = len(streams)
    resets = resets or {}
    # every channel's stream in segments between resets; a segment's counters begin at 0
    bounds = [[0] for _ in range(C)]
    done = np.zeros(C, np.int64)
    for i, k in enumerate(calls):
        for c in resets.get(i, ()):
            if done[c] != bounds[c][-1]:
                bounds[c].append(int(done[c]))
        done += np.asarray(k, np.int64)
    segments, memo = [], {}
    for c in range(C):
        edges = bounds[c] + [int(done[c])]
        segs = []
        for a, b in zip(edges[:-1], edges[1:]):
            part = np.ascontiguousarray(streams[c][a:b])
            key = (part.dtype.str, part.tobytes())            # (channels that carry the same stream share the work)
            if key not in memo:
                which = np.full(b - a, -1, np.int64)          # per sample: the index of the capture that holds it
                caps = captures_of_stream(part, rate, kinds, tail_blocks, max_blocks)
                for n, cap in enumerate(caps):
                    which[cap["first"]:cap["end"]] = n
                memo[key] = (caps, which)
            segs.append((a, b) + memo[key])
        segments.append(segs)
    out = []
    done[:] = 0
    for i, k in enumerate(calls):
        chunks, room = [], pool
        for c in range(C):
            lo, hi = int(done[c]), int(done[c]) + int(k[c])
            for a, b, caps, which in segments[c]:
                s, e = max(lo, a), min(hi, b)
                if s >= e:
                    continue
                w = which[s - a:e - a]
                edges = np.flatnonzero(np.diff(np.concatenate([[-1], w, [-1]])) != 0)
                for r0, r1 in zip(edges[:-1], edges[1:]):
                    n = int(w[r0])
                    if n < 0:
                        continue
                    cap = caps[n]
                    at0, at1 = s - a + int(r0), s - a + int(r1)        # in the segment's counters
                    flags = (FIRST if at0 == cap["first"] else 0) | (cap["flag"] if at1 == cap["end"] else 0)
                    take = min(room, at1 - at0)
                    if take < at1 - at0:
                        flags |= TRUNCATED
                    room -= take
                    chunks.append((c, flags, cap["kind"], at0, cap["tone_start"],
                                   np.asarray(streams[c][a + at0:a + at0 + take]).astype(np.float32)))
        done += np.asarray(k, np.int64)
        out.append(chunks)
    return out


def join(chunks_per_call):
    """{(channel, tone_start of the capture, sample_counter of its first chunk, how many captures the channel had before):
    (concatenated samples, the chunks' flags or-ed together, kind)}"""
    caps, cur, seen = {}, {}, {}
    for chunks in chunks_per_call:
        for c, flags, kind, at, tone_start, samples in chunks:
            if flags & FIRST or c not in cur:
                cur[c] = (c, tone_start, at, seen.get(c, 0))
                seen[c] = seen.get(c, 0) + 1
                caps[cur[c]] = [[], 0, kind]
            caps[cur[c]][0].append(samples)
            caps[cur[c]][1] |= flags
            if flags & END:
                del cur[c]
    return {key: (np.concatenate(v[0]), v[1], v[2]) for key, v in caps.items()}
