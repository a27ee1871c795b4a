"""Tone-alert audio in delivery form on the device (include/same_tone_delivery.h, sameold_amd/csrc/same_tone_delivery.hip)
against the numpy restatement of its contract (tests/helpers/tone_delivery_reference.py): every chunk's record and int16
samples bit for bit, in queue order, over 130 channels (two whole groups of 64 and a partial one) x 60 blocks, both layouts, f32
and int16, plain and ragged calls, at 8 000 -> 8 000, 8 000 -> 4 000 and 22 050 -> 8 000, and once at the tap limit
(48 000 -> 8 000, 66 channels), on the cut that puts calls of 1, 1, 2, T - 2, T - 1 and T rows inside open captures; a group in
which nobody captures; a pool that fills; the int16 identity; the refusals; calls that nobody polls between and a view dropped
in parts, as test_tone_audio_gpu.py has them.  The streams, the patterns and the call tensors
are test_tone_audio_gpu.py's."""
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
from test_tone_audio_gpu import (BOTH, C1, CAPTURING, CHANNEL_MAJOR, MAXB, NOISE, SILENCE, TAIL, TIME_MAJOR, TWO_TONE, TWO_TONE_OFF,  # noqa: E402
                                 WAT_LONG, assert_view_dropped_in_parts, base_streams, calls_of, device_input, run_unpolled)

pytestmark = pytest.mark.gpu

RATES = [(8000, 8000), (8000, 4000), (22050, 8000)]


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


def short_calls(length, C, N, T, ragged):
    """the cut with short calls inside open captures: 29 N + 3 rows, then 1, 1, 2, T - 2, T - 1, T rows (those that are
    positive), then the rest.  ragged: channel c takes (c mod 4) * 5 rows fewer of the two long calls, every seventh channel
    sits out every other short call with no row, and a last call hands every channel what it still lacks"""
    rows = [29 * N + 3] + [n for n in (1, 1, 2, T - 2, T - 1, T) if n > 0]
    rows.append(length - sum(rows))
    calls, done = [], np.zeros(C, np.int64)
    for i, n in enumerate(rows):
        k = np.full(C, n, np.int64)
        if ragged:
            if i in (0, len(rows) - 1):
                k = k - np.arange(C) % 4 * 5
            elif i % 2:
                k[::7] = 0
        calls.append(k)
        done += k
    if ragged:
        calls.append(length - done)
    return calls


_cases = {}


def case(rate, out_rate, pattern, ragged, C=C1):
    """(streams [C x samples], calls, the reference's chunks per call, its captures) -- computed once, shared by the layouts and
    sample types"""
    key = (rate, out_rate, pattern, ragged, C)
    if key not in _cases:
        N = rate // 25
        L, M, T = rr.plan(rate, out_rate)
        base = base_streams(rate)
        capturing = [c for c in CAPTURING[pattern] if c < C]
        kind_of = np.array([NOISE + c % 2 for c in range(C)])
        for i, c in enumerate(capturing):
            kind_of[c] = i % 3
        x = base[kind_of].astype(np.float32)
        if pattern == "main":
            calls = short_calls(x.shape[1], C, N, T, ragged)
        else:                                     # "skip": every 7 blocks and 13 samples, as test_tone_audio_gpu.py cuts it
            step = 7 * N + 13
            calls = calls_of(x.shape[1], C, ragged, [step] * (x.shape[1] // step) + [x.shape[1] % step])
        want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, x.size)
        # the reference alone: one capture on every capturing channel, none elsewhere; chunks that continue a capture
        assert sorted(cap["channel"] for cap in caps) == sorted(capturing) and len(capturing) > 0
        flat = [c for call in want for c in call]
        assert any(not c[1] & ar.FIRST for c in flat) and sum(1 for c in flat if c[1] & ar.END) == len(capturing)
        if pattern == "main":
            # every capturing channel that has rows in a short call has a chunk in it, none of them FIRST
            for i in range(1, len(calls) - (2 if ragged else 1)):
                assert [c[0] for c in want[i]] == [c for c in sorted(capturing) if calls[i][c] > 0] and all(c[1] == 0 for c in want[i])
            if M > L:
                assert any(len(c[6]) == 0 for c in want[1] + want[2])
        _cases[key] = (x, calls, want, caps)
    return _cases[key]


def run_calls(sa, x, rate, calls, dtype, layout, plain, delivery):
    """the calls through a ToneDetector in delivery form: (its events, its chunks per call as the reference lists them)"""
    td = sa.ToneDetector(x.shape[0], rate)
    if delivery:
        td.set_audio_delivery(*delivery)
    done = np.zeros(x.shape[0], np.int64)
    chunks = []
    for k in calls:
        td.process(device_input(x, done, k, dtype, layout), None if plain else k, layout)
        done += k
        td.sync()
        assert td.poll_audio() == []
        got = td.poll_delivery()
        assert all(int(r["rate"]) == delivery[4] and int(r["n_samples"]) == len(a) and a.dtype == np.int16 for r, a in got)
        chunks.append([(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), int(r["out_index"]), a)
                       for r, a in got])
    assert all(td.channel_sample_counter(c) == x.shape[1] for c in range(x.shape[0]))
    return td.poll(), chunks


def assert_same_chunks(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c[:6] for c in g] == [c[:6] for c in w], f"{what}: call {i}"
        for a, b in zip(g, w):
            assert np.array_equal(a[6], b[6]), f"{what}: call {i} channel {a[0]}"


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("layout", [TIME_MAJOR, CHANNEL_MAJOR], ids=["time", "channel"])
@pytest.mark.parametrize("rate,out_rate", RATES)
def test_chunks_equal_the_reference_bit_for_bit(sa, rate, out_rate, layout, dtype, ragged):
    x, calls, want, caps = case(rate, out_rate, "main", ragged)
    events, chunks = run_calls(sa, x, rate, calls, dtype, layout, not ragged, (BOTH, TAIL, MAXB, x.size, out_rate, 1.0))
    assert_same_chunks(chunks, want, "main")
    if out_rate == rate:
        # the int16 identity: the captured input rows come back exactly
        rows = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size)
        for g, w in zip(chunks, rows):
            assert len(g) == len(w) and all(np.array_equal(a[6], b[5].astype(np.int16)) and np.array_equal(a[6].astype(np.float32), b[5])
                                            for a, b in zip(g, w))
    if layout == TIME_MAJOR and dtype == np.float32:
        # the tone events beside a delivery are those of a handle with no capture
        td = sa.ToneDetector(x.shape[0], rate)
        done = np.zeros(x.shape[0], np.int64)
        for k in calls:
            td.process(device_input(x, done, k, dtype, layout), None if not ragged else k, layout)
            done += k
        td.sync()
        assert td.poll_delivery() == [] and td.poll_audio() == []
        plain_events = td.poll()
        assert len(events) >= len(CAPTURING["main"]) and np.array_equal(events, plain_events)


def test_the_rate_at_the_tap_limit(sa):
    rate, out_rate = 48000, 8000
    assert rr.plan(rate, out_rate) == (1, 6, 96)
    x, calls, want, caps = case(rate, out_rate, "main", True, C=66)
    _, chunks = run_calls(sa, x, rate, calls, np.float32, TIME_MAJOR, False, (BOTH, TAIL, MAXB, x.size, out_rate, 1.0))
    assert_same_chunks(chunks, want, "48 000 -> 8 000")


@pytest.mark.parametrize("dtype,layout", [(np.float32, TIME_MAJOR), (np.int16, CHANNEL_MAJOR)], ids=["f32-time", "i16-channel"])
def test_a_group_in_which_nobody_captures_is_skipped(sa, dtype, layout):
    x, calls, want, caps = case(8000, 4000, "skip", True)
    _, chunks = run_calls(sa, x, 8000, calls, dtype, layout, False, (BOTH, TAIL, MAXB, x.size, 4000, 1.0))
    assert_same_chunks(chunks, want, "skip")
    assert {c[0] for call in chunks for c in call} == {0, 63, 129}
    assert sum(len(call) for call in chunks) > 6             # the captures came in pieces


@pytest.mark.parametrize("layout", [TIME_MAJOR, CHANNEL_MAJOR], ids=["time", "channel"])
def test_a_pool_that_fills_and_the_history_behind_it(sa, layout):
    rate, out_rate, N = 22050, 8000, 882
    L, M, T = rr.plan(rate, out_rate)
    base = base_streams(rate)
    x = base[[TWO_TONE, TWO_TONE_OFF, WAT_LONG, NOISE, SILENCE, WAT_LONG]].astype(np.float32)
    calls = short_calls(x.shape[1], 6, N, T, False)
    pool = 2 * N + 11
    want, _ = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, pool)
    # the reference alone: the first call fills the pool inside its second capturing channel; the short calls have room
    assert [c[0] for c in want[0]] == [0, 1, 2, 5] and [bool(c[1] & ar.TRUNCATED) for c in want[0]] == [False, True, True, True]
    assert len(want[0][1][6]) > 0 and len(want[0][2][6]) == 0 and len(want[0][3][6]) == 0
    assert not any(c[1] & ar.TRUNCATED for call in want[1:7] for c in call) and all(len(call) == 4 for call in want[1:7])
    _, chunks = run_calls(sa, x, rate, calls, np.float32, layout, True, (BOTH, TAIL, MAXB, pool, out_rate, 1.0))
    assert_same_chunks(chunks, want, "a pool that fills")
    # the history went on regardless: behind the truncation the chunks are those of a pool with room, which gives the whole captures
    whole_want, caps = dr.chunks_of_calls(x, rate, out_rate, 1.0, calls, BOTH, TAIL, MAXB, x.size)
    _, whole = run_calls(sa, x, rate, calls, np.int16, layout, True, (BOTH, TAIL, MAXB, x.size, out_rate, 1.0))
    assert_same_chunks(whole, whole_want, "a pool with room")
    for i in range(1, 7):
        assert [c[:6] for c in chunks[i]] == [c[:6] for c in whole[i]] and all(np.array_equal(a[6], b[6]) for a, b in zip(chunks[i], whole[i]))
    for cap in caps:
        got = np.concatenate([c[6] for call in whole for c in call if c[0] == cap["channel"]])
        assert np.array_equal(got, cap["y"])


def test_a_gain_that_clips(sa):
    rate, out_rate, gain = 8000, 4000, 8.0
    x, calls, _, _ = case(rate, out_rate, "skip", True)
    want, caps = dr.chunks_of_calls(x, rate, out_rate, gain, calls, BOTH, TAIL, MAXB, x.size)
    y = np.concatenate([cap["y"] for cap in caps])
    assert (y == 32767).sum() > 10 and (y == -32768).sum() > 10 and (np.abs(y.astype(np.int32)) < 32000).sum() > 10
    _, chunks = run_calls(sa, x, rate, calls, np.float32, CHANNEL_MAJOR, False, (BOTH, TAIL, MAXB, x.size, out_rate, gain))
    assert_same_chunks(chunks, want, "gain 8")


def test_refusals_and_the_modes(sa):
    import torch
    td = sa.ToneDetector(6, 8000)
    bad = [(0, 0, 1, 100, 8000, 1.0), (4, 0, 1, 100, 8000, 1.0), (3, 0, 0, 100, 8000, 1.0),      # the mask, max_blocks
           (3, 0, 1, 100, 0, 1.0), (3, 0, 1, 100, 8001, 1.0), (3, 0, 1, 100, 16000, 1.0),           # out_rate: zero, above the rate
           (3, 0, 1, 100, 8000, 0.0), (3, 0, 1, 100, 8000, -1.0), (3, 0, 1, 100, 8000, float("nan")), (3, 0, 1, 100, 8000, float("inf"))]
    for args in bad:
        with pytest.raises(sa.SameError) as e:
            td.set_audio_delivery(*args)
        assert e.value.code == -1, args
    fast = sa.ToneDetector(6, 96000)
    with pytest.raises(sa.SameError) as e:                   # 96 000 -> 8 000 would need 192 taps
        fast.set_audio_delivery(BOTH, TAIL, MAXB, 100, 8000)
    assert e.value.code == -9 and "taps" in str(e.value)      # SAME_ERATE
    fast.set_audio_delivery(BOTH, TAIL, MAXB, 100, 16000)    # (96 taps: the limit)
    td.set_audio_delivery(BOTH, TAIL, MAXB, 0, 0, 0.0)       # off: the other arguments are not looked at
    td.set_audio_delivery(BOTH, TAIL, MAXB, 100, 4000)
    assert td.poll_delivery() == [] and td.poll_audio() == []
    td.process(torch.zeros((10, 6), dtype=torch.float32, device="cuda"))
    for call in (lambda: td.set_audio_delivery(BOTH, TAIL, MAXB, 100, 4000), lambda: td.set_audio_capture(BOTH, TAIL, MAXB, 100)):
        with pytest.raises(sa.SameError) as e:               # behind the handle's first sample
            call()
        assert e.value.code == -1
    td.sync()
    assert td.poll_delivery() == [] and td.poll_audio() == [] and len(td.poll()) == 0


def test_a_handle_in_float_capture_mode_is_what_it_was(sa):
    """the last of the two set calls decides the mode: float capture behind a delivery set gives the float chunks, and no
    delivery chunk"""
    rate = 8000
    x, calls, _, _ = case(rate, 4000, "skip", True)
    want = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size)
    td = sa.ToneDetector(x.shape[0], rate)
    td.set_audio_delivery(BOTH, TAIL, MAXB, x.size, 4000)
    td.set_audio_capture(BOTH, TAIL, MAXB, x.size)
    done = np.zeros(x.shape[0], np.int64)
    for k, w in zip(calls, want):
        td.process(device_input(x, done, k, np.float32, TIME_MAJOR), k, TIME_MAJOR)
        done += k
        td.sync()
        assert td.poll_delivery() == []
        got = td.poll_audio()
        assert [(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"])) for r, a in got] == [c[:5] for c in w]
        assert all(np.array_equal(a.view(np.uint32), c[5].view(np.uint32)) for (r, a), c in zip(got, w))


DELIVERY_FIELDS = ("channel", "flags", "kind", "sample_counter", "tone_start", "out_index")


def unpolled_delivery(sa):
    x, calls, want, _ = case(8000, 4000, "skip", True)
    # the reference alone: more calls carry samples than there are slots, so a slot is taken again with its samples unfetched
    assert sum(1 for call in want if any(len(c[6]) for c in call)) >= 4
    td = run_unpolled(sa, x, 8000, calls, np.int16, CHANNEL_MAJOR, lambda td: td.set_audio_delivery(BOTH, TAIL, MAXB, x.size, 4000, 1.0))
    return td, [c for call in want for c in call]


def test_calls_nobody_polls_between(sa):
    td, flat = unpolled_delivery(sa)
    assert td.poll_audio() == []
    got = td.poll_delivery()
    assert all(int(r["rate"]) == 4000 and int(r["n_samples"]) == len(a) and a.dtype == np.int16 for r, a in got)
    assert_same_chunks([[tuple(int(r[f]) for f in DELIVERY_FIELDS) + (a,) for r, a in got]], [flat], "one poll behind all calls")
    assert td.poll_delivery() == []


def test_a_view_dropped_in_parts(sa):
    import ctypes
    td, flat = unpolled_delivery(sa)
    assert_view_dropped_in_parts(td, td._L.same_tone_delivery_peek, td._L.same_tone_delivery_drop, sa.TONE_DELIVERY_CHUNK_DTYPE,
                                 DELIVERY_FIELDS, ctypes.c_int16, flat, assert_same_chunks)
