"""Device paths of the tone family (same_tones.hip, same_tone_audio.hip, same_tone_delivery.hip) that the modules written
beside the code do not reach, each bit for bit against the numpy references (tests/helpers/tones_reference.py,
tone_audio_reference.py, tone_delivery_reference.py):
  1. three rounds of channels (2 114: 33 groups and two channels; the place kernels' rounds of 1 024, 1 024 and 66);
  2. calls in flight: no sync and no poll between the calls, a poll behind every call without a sync, the peek / drop view;
  3. two captures of one channel in one call;
  4. a chunk of more than 64 tiles of 256 outputs;
  5. ratios with many phases (L = 1 024, the limit, and L = 320);
  6. exactly eight and exactly nine capturing channels in a group of the time-major copy;
  7. a reset in mid-capture.
Every test first asserts on the reference alone that its case has the property it is named for.  The streams, the call cuts and
the call tensors are test_tone_audio_gpu.py's and test_tone_delivery_gpu.py's."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_reference as rr  # noqa: E402
import tones_reference as tr  # noqa: E402
import tone_audio_reference as ar  # noqa: E402
import tone_delivery_reference as dr  # noqa: E402
import test_tone_audio_gpu as ta  # noqa: E402
import test_tone_delivery_gpu as tdg  # noqa: E402
from test_tone_audio_gpu import (BOTH, CHANNEL_MAJOR, MAXB, NOISE, TAIL, TIME_MAJOR, TWO_TONE, WAT_LONG,  # noqa: E402
                                 base_streams, calls_of, device_input)
from test_tone_delivery_gpu import short_calls  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
F32_TIME, I16_CHANNEL, F32_CHANNEL, I16_TIME = (np.float32, TIME_MAJOR), (np.int16, CHANNEL_MAJOR), (np.float32, CHANNEL_MAJOR), (np.int16, TIME_MAJOR)
FORMS = {"f32-time": F32_TIME, "i16-channel": I16_CHANNEL, "f32-channel": F32_CHANNEL, "i16-time": I16_TIME}


@pytest.fixture(scope="module")
def sa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sameold_amd import build as sbuild
    sbuild.build()
    import sameold_amd
    sameold_amd.load_library()
    return sameold_amd


# ------------------------------------------------------------------------------------------------------ the references
def events_per_call(x, rate, calls, resets=None):
    """the reference's tone events of every call, in queue order: inside a call by channel, then by the block that emitted the
    event, then by kind.  An event belongs to the call that completes the block which emits it."""
    N = rate // 25
    C = len(x)
    resets = resets or {}
    memo = {}
    out = [[] for _ in calls]
    for c in range(C):
        bounds, done = [0], 0
        for i, k in enumerate(calls):
            if c in resets.get(i, ()) and done != bounds[-1]:
                bounds.append(done)
            done += int(k[c])
        ends = np.cumsum([int(k[c]) for k in calls])
        for a, b in zip(bounds, bounds[1:] + [done]):
            part = np.ascontiguousarray(x[c][a:b])
            key = part.tobytes()
            if key not in memo:
                vals, E = tr.blocks_f32(part, rate, True)
                attn, wat = tr.qualify_f32(vals, rate, E)
                ch, ev = tr.Channel(0, N), []
                for j in range(len(attn)):
                    ev += [(j, e) for e in ch.feed(attn[j:j + 1], wat[j:j + 1])]
                memo[key] = ev
            for j, e in memo[key]:
                call = int(np.searchsorted(ends, a + (j + 1) * N))
                out[call].append((c,) + tuple(e[1:]))
    return [sorted(call, key=lambda e: e[0]) for call in out]          # (stable: a channel's events stay in stream order)


def event_tuples(records):
    return [tuple(int(e[k]) for k in ("channel", "kind", "edge", "reserved", "sample_counter", "duration")) for e in records]


def float_tuples(got):
    assert all(int(r["reserved"]) == 0 and int(r["n_samples"]) == len(a) and a.dtype == np.float32 for r, a in got)
    return [(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), a) for r, a in got]


def delivery_tuples(got, out_rate):
    assert all(int(r["rate"]) == out_rate and int(r["n_samples"]) == len(a) and a.dtype == np.int16 for r, a in got)
    return [(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), int(r["out_index"]), a)
            for r, a in got]


def flat(per_call):
    return [[c for call in per_call for c in call]]


def run(sa, x, rate, calls, form, plain, mode, resets=None, pace="sync", stream=False, blocks=False):
    """The calls through a ToneDetector.  mode: None, ("float", kinds, tail, max_blocks, pool) or ("delivery", kinds, tail,
    max_blocks, pool, out_rate, gain).  pace: "sync" -- sync and poll behind every call; "poll" -- poll behind every call, sync
    only behind the last; "end" -- nothing between the calls, one sync and one poll behind the last.  stream: the calls go to a
    stream of their own.  Returns (events per poll, chunks per poll, block records per call or None, the detector)."""
    import torch
    dtype, layout = form
    C = x.shape[0]
    td = sa.ToneDetector(C, rate)
    if mode and mode[0] == "float":
        td.set_audio_capture(*mode[1:])
    elif mode:
        td.set_audio_delivery(*mode[1:])
    resets = resets or {}
    done = np.zeros(C, np.int64)
    tensors = []
    for k in calls:
        tensors.append(device_input(x, done, np.asarray(k), dtype, layout))
        done += k
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if stream else None

    def take():
        ev = event_tuples(td.poll())
        if mode and mode[0] == "delivery":
            assert td.poll_audio() == []
            return ev, delivery_tuples(td.poll_delivery(), mode[5])
        got = td.poll_audio()
        assert td.poll_delivery() == [] and (mode or got == [])
        return ev, float_tuples(got)

    events, chunks, records = [], [], []
    for i, (k, t) in enumerate(zip(calls, tensors)):
        if i in resets:
            td.reset_channels(resets[i])
        b = None
        if blocks:
            want, most = td.block_counts(int(np.max(k)), None if plain else k)
            b = torch.full((most + 1, C, 4), SENTINEL, dtype=torch.float32, device="cuda")
            records.append((want, b))
        td.process(t, None if plain else k, layout, b, stream=st.cuda_stream if st else None)
        if pace == "end":
            continue
        if pace == "sync":
            td.sync()
        e, c = take()
        events.append(e)
        chunks.append(c)
    td.sync()
    e, c = take()
    if pace != "sync":
        events.append(e)
        chunks.append(c)
    else:
        assert e == [] and c == []
    if st:
        st.synchronize()
    return events, chunks, ([(w, b.cpu().numpy()) for w, b in records] if blocks else None), td


# ------------------------------------------------------------------------------------- 1. three rounds of channels
C3, RATE3, BLOCKS3 = 2114, 8000, 45
N3 = RATE3 // 25
CAPTURING3 = sorted(set([0, 1023, 1024, 2047, 2048, 2113] + list(range(1088, 1152)) + list(range(0, C3, 97))))

_rounds = {}


def rounds_case():
    """(streams [2 114 x 45 blocks], the stream every channel carries, three plain calls cut at 13 N + 7)"""
    if not _rounds:
        base = base_streams(RATE3)[:, :BLOCKS3 * N3]
        kind_of = np.array([NOISE + c % 2 for c in range(C3)])
        for i, c in enumerate(CAPTURING3):
            kind_of[c] = i % 3
        x = base[kind_of].astype(np.float32)
        rows = [13 * N3 + 7, 13 * N3 + 7]
        rows.append(x.shape[1] - sum(rows))
        _rounds["case"] = (x, kind_of, base.astype(np.float32), calls_of(x.shape[1], C3, False, rows))
        assert C3 == 33 * 64 + 2 and C3 > 2 * 1024 and len(CAPTURING3) > 80
    return _rounds["case"]


def rounds_want(key, make):
    if key not in _rounds:
        _rounds[key] = make()
    return _rounds[key]


def test_three_rounds_blocks_and_events(sa):
    x, kind_of, base, calls = rounds_case()
    vals = tr.blocks_f32(base, RATE3)[kind_of]                 # [C, 45, 4]
    want_events = rounds_want("events", lambda: events_per_call(x, RATE3, calls))
    started = {e[0] for call in want_events for e in call if e[2] == tr.START}
    assert started == set(CAPTURING3) and max(started) >= 2048 and any(e[2] == tr.END for call in want_events for e in call)
    events, _, records, td = run(sa, x, RATE3, calls, F32_TIME, True, None, blocks=True)
    assert events == want_events
    got = np.concatenate([b[:int(w.max())] for w, b in records]).transpose(1, 0, 2)
    assert all(np.all(w == w[0]) and np.all(b[int(w[0]):] == np.float32(SENTINEL)) for w, b in records)
    assert got.shape == vals.shape
    bad = np.flatnonzero((got.view(np.uint32) != vals.view(np.uint32)).any(axis=(1, 2)))
    assert bad.size == 0, f"block records differ on {bad.size} channels, first {bad[0]}"


@pytest.mark.parametrize("form", ["f32-time", "i16-channel"])
def test_three_rounds_float_capture(sa, form):
    x, kind_of, base, calls = rounds_case()
    pool = len(CAPTURING3) * x.shape[1]
    want = rounds_want("float", lambda: ar.chunks_of_calls(x, RATE3, calls, BOTH, TAIL, MAXB, pool))
    caps = ar.join(want)
    assert sorted(k[0] for k in caps) == CAPTURING3 and not any(c[1] & ar.TRUNCATED for call in want for c in call)
    # channels of the second and third round have chunks behind others in the same call: their room needs the carried total
    assert all(any(c[0] >= 1024 for c in call) and any(c[0] >= 2048 for c in call) and call[0][0] < 1024 for call in want[1:])
    events, chunks, _, _ = run(sa, x, RATE3, calls, FORMS[form], True, ("float", BOTH, TAIL, MAXB, pool))
    ta.assert_same_chunks(chunks, want, "three rounds")
    assert events == rounds_want("events", lambda: events_per_call(x, RATE3, calls))


def test_three_rounds_delivery(sa):
    x, kind_of, base, calls = rounds_case()
    pool = len(CAPTURING3) * x.shape[1]
    want, caps = rounds_want("delivery", lambda: dr.chunks_of_calls(x, RATE3, 4000, 1.0, calls, BOTH, TAIL, MAXB, pool))
    assert sorted(cap["channel"] for cap in caps) == CAPTURING3
    assert all(any(c[0] >= 1024 and len(c[6]) for c in call) and any(c[0] >= 2048 and len(c[6]) for c in call) for call in want[1:])
    _, chunks, _, _ = run(sa, x, RATE3, calls, I16_TIME, True, ("delivery", BOTH, TAIL, MAXB, pool, 4000, 1.0))
    tdg.assert_same_chunks(chunks, want, "three rounds, 8 000 -> 4 000")


def test_three_rounds_a_pool_that_fills_in_the_third(sa):
    x, kind_of, base, calls = rounds_case()
    whole = rounds_want("float", lambda: ar.chunks_of_calls(x, RATE3, calls, BOTH, TAIL, MAXB, len(CAPTURING3) * x.shape[1]))
    # the last call's captured rows in front of channel 2 048, and a hundred more: the pool ends inside that channel's chunk
    pool = sum(len(c[5]) for c in whole[2] if c[0] < 2048) + 100
    want = ar.chunks_of_calls(x, RATE3, calls, BOTH, TAIL, MAXB, pool)
    cut = [c for call in want for c in call if c[1] & ar.TRUNCATED]
    assert cut and all(c[0] >= 2048 for c in cut) and [len(c[5]) for c in cut if c[0] == 2048] == [100]
    assert any(c[0] == 2113 and len(c[5]) == 0 for c in cut)
    _, chunks, _, _ = run(sa, x, RATE3, calls, F32_TIME, True, ("float", BOTH, TAIL, MAXB, pool))
    ta.assert_same_chunks(chunks, want, "three rounds, a pool that fills")


# ---------------------------------------------------------------------------------------------------- 2. in flight
def flight_case(kind, pattern):
    """the existing ragged cases: (streams, rate, calls, mode, the reference's chunks per call, the assertion that compares)"""
    if kind == "float":
        x, calls, want = ta.case(8000, pattern, True)
        return x, 8000, calls, ("float", BOTH, TAIL, MAXB, x.size), want, ta.assert_same_chunks
    x, calls, want, _ = tdg.case(22050, 8000, pattern, True)
    return x, 22050, calls, ("delivery", BOTH, TAIL, MAXB, x.size, 8000, 1.0), want, tdg.assert_same_chunks


@pytest.mark.parametrize("pace", ["end", "poll"])
@pytest.mark.parametrize("pattern", ["skip", "main"])
@pytest.mark.parametrize("kind", ["float", "delivery"])
def test_calls_in_flight(sa, kind, pattern, pace):
    x, rate, calls, mode, want, same = flight_case(kind, pattern)
    # more calls than slots; in the "skip" cut chunks in more than three of them (a slot is taken again while its pool waits to
    # be fetched), and the first chunks of two calls that share a slot hold different samples
    assert len(calls) > 6
    if pattern == "skip":
        assert sum(1 for call in want if call) > 3
        assert any(want[i] and want[i + 3] and not np.array_equal(want[i][0][-1][:50], want[i + 3][0][-1][:50]) for i in range(len(want) - 3))
    want_events = events_per_call(x, rate, calls)
    assert sum(len(e) for e in want_events) >= 3
    events, chunks, _, td = run(sa, x, rate, calls, F32_TIME if pattern == "skip" else I16_CHANNEL, False, mode, pace=pace, stream=True)
    assert len(chunks) == (1 if pace == "end" else len(calls) + 1)
    same(flat(chunks), flat(want), f"{kind}, {pattern}, {pace}")
    assert [e for poll in events for e in poll] == [e for call in want_events for e in call]
    assert all(td.channel_sample_counter(c) == x.shape[1] for c in range(x.shape[0]))


def test_the_delivery_view_and_its_pinned_blocks(sa):
    """same_tone_delivery_peek / _drop by hand: two peeks give one view, a drop leaves the rest as it was, and behind a view that
    was dropped whole the next calls' samples -- in host blocks that were handed back -- are the reference's"""
    import torch
    x, calls, want, _ = tdg.case(22050, 8000, "skip", True)
    split = 5
    assert sum(1 for call in want[:split] if call) >= 2 and sum(1 for call in want[split:split + 3] if any(len(c[6]) for c in call)) >= 2
    from sameold_amd import tones
    L = tones._lib()
    dt = tones.TONE_DELIVERY_CHUNK_DTYPE
    td = sa.ToneDetector(x.shape[0], 22050)
    td.set_audio_delivery(BOTH, TAIL, MAXB, x.size, 8000, 1.0)
    done = np.zeros(x.shape[0], np.int64)
    st = torch.cuda.Stream()

    def feed(some):
        for k in some:
            t = device_input(x, done, k, np.float32, TIME_MAJOR)
            torch.cuda.synchronize()
            td.process(t, k, TIME_MAJOR, stream=st.cuda_stream)
            done[:] += k
        td.sync()

    def peek():
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        assert L.same_tone_delivery_peek(td._h, ctypes.byref(ptr), ctypes.byref(n)) == 0
        if not n.value:
            return ptr.value, np.zeros(0, dt), []
        recs = np.frombuffer((ctypes.c_char * (n.value * dt.itemsize)).from_address(ptr.value), dtype=dt).copy()
        data = [np.ctypeslib.as_array(ctypes.cast(int(r["samples"]), ctypes.POINTER(ctypes.c_int16)), shape=(int(r["n_samples"]),)).copy()
                if r["n_samples"] else np.zeros(0, np.int16) for r in recs]
        return ptr.value, recs, data

    def tuples(recs, data):
        return [(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), int(r["out_index"]), a)
                for r, a in zip(recs, data)]

    feed(calls[:split])
    p1, r1, d1 = peek()
    p2, r2, d2 = peek()
    assert p1 == p2 and r1.tobytes() == r2.tobytes() and len(r1) > 2
    tdg.assert_same_chunks([tuples(r1, d1)], flat(want[:split]), "the view")
    assert L.same_tone_delivery_drop(td._h, 1) == 0
    _, r3, d3 = peek()
    assert len(r3) == len(r1) - 1 and r3.tobytes() == r1[1:].tobytes()          # (records and pointers: nothing moved)
    tdg.assert_same_chunks([tuples(r3, d3)], [flat(want[:split])[0][1:]], "the view behind a drop")
    assert L.same_tone_delivery_drop(td._h, len(r3) + 1) < 0                    # more than the view holds: refused, nothing dropped
    assert L.same_tone_delivery_drop(td._h, len(r3)) == 0
    assert peek()[1].size == 0
    for i in range(split, len(calls)):                        # call by call: each fetch takes a block that was handed back
        feed(calls[i:i + 1])
        _, r, d = peek()
        tdg.assert_same_chunks([tuples(r, d)], [want[i]], f"call {i} behind the drop")
        assert L.same_tone_delivery_drop(td._h, len(r)) == 0
    st.synchronize()


# ------------------------------------------------------------------------------- 3. two captures of a channel in one call
def twice_streams(rate, C=70):
    """every third channel: two-tone in blocks 2 .. 33, noise to 41, 1050 Hz in 42 .. 73, noise to block 110; the others noise
    or silence"""
    N = rate // 25
    n = 110 * N
    rng = np.random.default_rng(rate + 3)
    s = 3000.0 * rng.standard_normal(n)
    s[:2 * N] = 0.0
    s[2 * N:34 * N] = 8000.0 * tr.tone(tr.ATTENTION, 32 * N, rate, 1.0)
    s[42 * N:74 * N] = 8000.0 * tr.tone(tr.WAT, 32 * N, rate, 1.0)
    other = 3000.0 * rng.standard_normal(n)
    x = np.zeros((C, n))
    for c in range(C):
        x[c] = s if c % 3 == 0 else other if c % 3 == 1 else 0.0
    return (np.round(x) + 0.0).astype(np.float32)


_twice = {}


def twice_want(max_blocks, out_rate):
    key = (max_blocks, out_rate)
    if key not in _twice:
        x = _twice.setdefault("x", twice_streams(8000))
        calls = calls_of(x.shape[1], x.shape[0], False, [x.shape[1]])
        if out_rate:
            want = dr.chunks_of_calls(x, 8000, out_rate, 1.0, calls, BOTH, TAIL, max_blocks, x.size)[0]
        else:
            want = ar.chunks_of_calls(x, 8000, calls, BOTH, TAIL, max_blocks, x.size)
        # the reference alone: one call, two chunks of every third channel, both whole
        assert len(want) == 1 and [c[0] for c in want[0]] == [c for c in range(0, x.shape[0], 3) for _ in range(2)]
        at = {4: [8640, 21440], 20: [8640, 21440]}[max_blocks]
        rows = {4: 1280, 20: 4800}[max_blocks]
        for a, b in zip(want[0][0::2], want[0][1::2]):
            assert [a[3], b[3]] == at and a[1] & ar.FIRST and b[1] & ar.FIRST and a[1] & ar.END and b[1] & ar.END
            assert a[2] == tr.ATTENTION and b[2] == tr.WAT
            assert len(a[-1]) == len(b[-1]) == (rows if not out_rate else rows * out_rate // 8000)
        _twice[key] = (x, calls, want)
    return _twice[key]


@pytest.mark.parametrize("max_blocks", [4, 20])
@pytest.mark.parametrize("form", list(FORMS))
def test_two_captures_of_a_channel_in_one_call(sa, form, max_blocks):
    x, calls, want = twice_want(max_blocks, 0)
    _, chunks, _, _ = run(sa, x, 8000, calls, FORMS[form], True, ("float", BOTH, TAIL, max_blocks, x.size))
    ta.assert_same_chunks(chunks, want, f"two captures, at most {max_blocks} blocks")
    x, calls, want = twice_want(max_blocks, 4000)
    _, chunks, _, _ = run(sa, x, 8000, calls, FORMS[form], True, ("delivery", BOTH, TAIL, max_blocks, x.size, 4000, 1.0))
    tdg.assert_same_chunks(chunks, want, f"two captures delivered at 4 000, at most {max_blocks} blocks")


def test_two_captures_and_a_cut_inside_the_second(sa):
    rate, out_rate = 22050, 8000
    N = rate // 25
    x = twice_streams(rate)
    calls = calls_of(x.shape[1], x.shape[0], False, [70 * N + 11, x.shape[1] - 70 * N - 11])
    want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, x.size)
    # the first call holds a whole capture and the FIRST chunk of the next, which the second call continues and ends
    assert [c[0] for c in want[0]][:2] == [0, 0] and len(caps) == 2 * len(range(0, x.shape[0], 3))
    first, second = want[0][0], want[0][1]
    assert first[1] & ar.FIRST and first[1] & ar.END and second[1] == ar.FIRST and len(second[6]) > 0
    assert [c[0] for c in want[1]] == list(range(0, x.shape[0], 3)) and all(c[1] & ar.END and not c[1] & ar.FIRST for c in want[1])
    _, chunks, _, _ = run(sa, x, rate, calls, F32_TIME, True, ("delivery", BOTH, TAIL, MAXB, x.size, out_rate, 1.0))
    tdg.assert_same_chunks(chunks, want, "two captures, 22 050 -> 8 000")


# --------------------------------------------------------------------------------------- 4. a chunk of more than 64 tiles
@pytest.mark.parametrize("rate,out_rate,max_blocks,n_blocks,plan,outputs", [(8000, 8000, 70, 100, (1, 1, 1), 22400),
                                                                          (48000, 44100, 10, 40, (147, 160, 18), 17640)])
def test_a_chunk_of_more_than_sixty_four_tiles(sa, rate, out_rate, max_blocks, n_blocks, plan, outputs):
    assert rr.plan(rate, out_rate) == plan
    N, C = rate // 25, 66
    rng = np.random.default_rng(rate + 4)
    capturing = [0, 31, 65]
    x = np.round(3000.0 * rng.standard_normal((C, n_blocks * N)))
    x[1::2] = 0.0
    for i, c in enumerate(capturing):
        x[c] = np.round(8000.0 * tr.tone(tr.WAT, n_blocks * N, rate, 1.0, 0.3 + i))
    x = (x + 0.0).astype(np.float32)
    calls = calls_of(x.shape[1], C, False, [x.shape[1]])
    want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, max_blocks, x.size)
    # one chunk per capturing channel, more than 64 tiles of 256 outputs
    assert [c[0] for c in want[0]] == capturing and all(len(c[6]) == outputs and c[1] == ar.FIRST | ar.END_MAX for c in want[0])
    assert outputs > 64 * 256
    _, chunks, _, _ = run(sa, x, rate, calls, F32_TIME, True, ("delivery", BOTH, TAIL, max_blocks, x.size, out_rate, 1.0))
    tdg.assert_same_chunks(chunks, want, f"{rate} -> {out_rate}")
    if out_rate == rate:                                       # the int16 identity: the captured input rows come back
        for c in chunks[0]:
            assert np.array_equal(c[6], x[c[0], c[3]:c[3] + outputs].astype(np.int16))


# --------------------------------------------------------------------------------------------------- 5. many phases
_phases = {}


def phases_case(rate, out_rate):
    if (rate, out_rate) not in _phases:
        N, C = rate // 25, 66
        L, M, T = rr.plan(rate, out_rate)
        base = base_streams(rate)
        capturing = [c for c in ta.CAPTURING["main"] if c < C]
        kind_of = np.array([NOISE + c % 2 for c in range(C)])
        for i, c in enumerate(capturing):
            kind_of[c] = i % 3
        x = base[kind_of].astype(np.float32)
        calls = short_calls(x.shape[1], C, N, T, True)
        want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, x.size)
        assert sorted(cap["channel"] for cap in caps) == capturing
        # chunks begin at many phases of the table's row
        phases = {c[5] * M % L for call in want for c in call if len(c[6])}
        assert len(phases) >= 6 and max(phases) >= L // 2
        _phases[(rate, out_rate)] = (x, calls, want)
    return _phases[(rate, out_rate)]


@pytest.mark.parametrize("form", ["f32-time", "i16-channel"])
@pytest.mark.parametrize("rate,out_rate,plan", [(10250, 10240, (1024, 1025, 18)), (22050, 16000, (320, 441, 24))])
def test_ratios_with_many_phases(sa, rate, out_rate, plan, form):
    assert rr.plan(rate, out_rate) == plan and rr.MAX_L == 1024
    x, calls, want = phases_case(rate, out_rate)
    _, chunks, _, _ = run(sa, x, rate, calls, FORMS[form], False, ("delivery", BOTH, TAIL, MAXB, x.size, out_rate, 1.0))
    tdg.assert_same_chunks(chunks, want, f"{rate} -> {out_rate}")


# ------------------------------------------------------------------------------------------------ 6. eight and nine
EIGHT = [1, 5, 9, 17, 30, 41, 52, 62]                        # (no multiple of 7: those sit out the long call of the ragged cut)
NINE = [64, 67, 72, 79, 86, 97, 104, 118, 127]
_eight = {}


def eight_and_nine_case():
    if not _eight:
        rate, C = 8000, 130
        capturing = EIGHT + NINE + [129]
        kind_of = np.array([NOISE + c % 2 for c in range(C)])
        for i, c in enumerate(capturing):
            kind_of[c] = i % 3
        x = base_streams(rate)[kind_of].astype(np.float32)
        calls = calls_of(x.shape[1], C, True)
        want = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size)
        caps = ar.join(want)
        assert sorted(k[0] for k in caps) == capturing
        # in one call, rows that all eight (nine) channels of the group capture, and chunks that begin at different rows
        at = max(range(len(want)), key=lambda i: len(want[i]))
        big, done = want[at], np.sum(calls[:at], axis=0)
        for group, n in ((EIGHT, 8), (NINE, 9)):
            spans = [(c[3] - int(done[c[0]]), c[3] - int(done[c[0]]) + len(c[5])) for c in big if c[0] in group]
            assert len(spans) == n and max(s[0] for s in spans) + 64 < min(s[1] for s in spans)
            assert len({s[0] % 64 for s in spans}) > 2 and len({s[1] % 64 for s in spans}) > 2
        _eight["case"] = (x, calls, want)
    return _eight["case"]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_eight_and_nine_capturing_channels_in_a_group(sa, dtype):
    x, calls, want = eight_and_nine_case()
    _, chunks, _, _ = run(sa, x, 8000, calls, (dtype, TIME_MAJOR), False, ("float", BOTH, TAIL, MAXB, x.size))
    ta.assert_same_chunks(chunks, want, "eight and nine")


# ------------------------------------------------------------------------------------------ 7. a reset in mid-capture
RESET7, NEIGHBOURS7 = 5, [2, 8]


def reset_case(rate):
    """66 channels x 60 blocks; channels 2, 5 and 8 carry the 1050 Hz tone; channel 5 is reset in front of the second call, 5
    blocks and 5 rows into its capture; the second call ends 5 rows behind the first row of the capture that follows"""
    N, C = rate // 25, 66
    kind_of = np.array([NOISE + c % 2 for c in range(C)])
    kind_of[[RESET7] + NEIGHBOURS7] = WAT_LONG
    kind_of[40] = TWO_TONE
    x = base_streams(rate)[kind_of].astype(np.float32)
    rows = [30 * N + 5, 25 * N + 5]
    rows.append(x.shape[1] - sum(rows))
    return x, calls_of(x.shape[1], C, False, rows), {1: [RESET7]}


def check_reset_reference(want, N):
    mine = [c for call in want for c in call if c[0] == RESET7]
    # a capture without an END, then a FIRST chunk whose counters begin at 0 behind the reset, continued in the last call
    assert [c[1] for c in mine] == [ar.FIRST, ar.FIRST, 0] and [c[3] for c in mine] == [25 * N, 25 * N, 25 * N + 5]
    assert [c[4] for c in mine] == [0, 0, 0]
    for other in NEIGHBOURS7:
        theirs = [c for call in want for c in call if c[0] == other]
        assert [c[1] for c in theirs] == [ar.FIRST, ar.END_MAX] and [c[3] for c in theirs] == [25 * N, 30 * N + 5]


@pytest.mark.parametrize("form", ["f32-time", "i16-channel"])
def test_a_reset_in_mid_capture_float(sa, form):
    rate, N = 8000, 320
    x, calls, resets = reset_case(rate)
    want = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size, resets)
    check_reset_reference(want, N)
    want_events = events_per_call(x, rate, calls, resets)
    assert [e[1:] for call in want_events for e in call if e[0] == RESET7] == [(tr.WAT, tr.START, 0, 0, 0)] * 2
    events, chunks, _, td = run(sa, x, rate, calls, FORMS[form], True, ("float", BOTH, TAIL, MAXB, x.size), resets)
    ta.assert_same_chunks(chunks, want, "a reset in mid-capture")
    assert events == want_events
    assert [td.channel_sample_counter(c) for c in (RESET7, NEIGHBOURS7[0])] == [x.shape[1] - 30 * N - 5, x.shape[1]]


@pytest.mark.parametrize("form", ["f32-time", "i16-channel"])
def test_a_reset_in_mid_capture_delivery(sa, form):
    rate, out_rate, N = 22050, 8000, 882
    L, M, T = rr.plan(rate, out_rate)
    assert 5 < T - 1                     # the second call leaves fewer rows of the new capture than the history holds
    x, calls, resets = reset_case(rate)
    want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, x.size, resets)
    check_reset_reference(want, N)
    mine = [c for call in want for c in call if c[0] == RESET7]
    assert [c[5] for c in mine][:2] == [0, 0] and mine[2][5] == rr.outputs_after(5, L, M) and len(mine[2][6]) > 1000
    _, chunks, _, td = run(sa, x, rate, calls, FORMS[form], True, ("delivery", BOTH, TAIL, MAXB, x.size, out_rate, 1.0), resets)
    tdg.assert_same_chunks(chunks, want, "a reset in mid-capture, 22 050 -> 8 000")
    assert [td.channel_sample_counter(c) for c in (RESET7, NEIGHBOURS7[0])] == [x.shape[1] - 30 * N - 5, x.shape[1]]
