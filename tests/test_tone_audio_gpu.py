"""Tone-alert audio on the device (include/same_tone_audio.h, sameold_amd/csrc/same_tone_audio.hip) against the numpy
restatement of its contract (tests/helpers/tone_audio_reference.py): every chunk bit for bit with its flags, counters and
queue order, over 130 channels (two whole groups of 64 and a partial one), both layouts, f32 and int16, plain and ragged calls;
a group in which nobody captures between two that do; a pool that fills; a handle with capture off; calls that nobody syncs or
polls between, so that a slot is taken again with its samples still on the device, with one poll behind them and with a view
dropped in parts through the raw peek and drop.  The tone events beside a capture are those of a handle without one."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402
import tone_audio_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_MAJOR, CHANNEL_MAJOR = 0, 1
BOTH = tr.ATTENTION | tr.WAT
TAIL, MAXB, BLOCKS = 3, 20, 60
C1 = 130
TWO_TONE, TWO_TONE_OFF, WAT_LONG, NOISE, SILENCE = range(5)
CAPTURING = {"main": [0, 63, 129] + list(range(64, 128)), "skip": [0, 63, 129]}     # "skip": nobody in the group 64 .. 127


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


def base_streams(rate):
    """[5 x 60 blocks], integer-valued (f32 and int16 hold the same values): tones at 8 000, white noise at 3 000 as the voice"""
    N = rate // 25
    length = BLOCKS * N
    rng = np.random.default_rng(rate)
    x = np.zeros((5, length))
    x[TWO_TONE, 2 * N:34 * N] = 8000.0 * tr.tone(tr.ATTENTION, 32 * N, rate, 1.0)
    x[TWO_TONE, 34 * N:] = 3000.0 * rng.standard_normal(length - 34 * N)
    x[TWO_TONE_OFF, 2 * N + 7:34 * N + 7] = 8000.0 * tr.tone(tr.ATTENTION, 32 * N, rate, 1.0)
    x[TWO_TONE_OFF, 34 * N + 7:] = 3000.0 * rng.standard_normal(length - 34 * N - 7)
    x[WAT_LONG] = 8000.0 * tr.tone(tr.WAT, length, rate, 1.0)
    x[NOISE] = 3000.0 * rng.standard_normal(length)
    return np.round(x) + 0.0              # (no -0.0: int16 cannot carry it)


def calls_of(length, C, ragged, rows=None):
    """the cut 1, 319, 320, 321, 1 000, rest (or `rows`); ragged: channel c takes (c mod 4) rows fewer of every call but keeps up with 0 of
    every third, and a last call hands every channel what it still lacks"""
    if rows is None:
        rows = [1, 319, 320, 321, 1000]
        rows.append(length - sum(rows))
    calls = []
    done = np.zeros(C, np.int64)
    for i, n in enumerate(rows):
        k = np.full(C, n, np.int64)
        if ragged:
            k = np.maximum(k - np.arange(C) % 4 * 5, 0)
            if i % 3 == 2:
                k[::7] = 0
        calls.append(k)
        done += k
    if ragged:
        calls.append(length - done)
    return calls


_cases = {}


def case(rate, pattern, ragged):
    """(streams [130 x samples], calls, the reference's chunks per call) -- computed once, shared by the layouts and sample types"""
    key = (rate, pattern, ragged)
    if key not in _cases:
        base = base_streams(rate)
        capturing = CAPTURING[pattern]
        kind_of = np.array([NOISE + c % 2 for c in range(C1)])
        for i, c in enumerate(capturing):
            kind_of[c] = i % 3
        x = base[kind_of].astype(np.float32)
        # "skip" cuts the streams every 7 blocks and 13 samples, so that captures cross calls and begin and end inside them
        step = 7 * (rate // 25) + 13
        rows = None if pattern == "main" else [step] * (x.shape[1] // step) + [x.shape[1] % step]
        calls = calls_of(x.shape[1], C1, ragged, rows)
        want = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size)
        # the reference alone: one capture on every capturing channel, none elsewhere
        caps = ar.join(want)
        assert sorted(k[0] for k in caps) == sorted(capturing) and len(caps) == len(capturing) > 0
        assert all(v[1] == ar.FIRST | (ar.END_MAX if kind_of[k[0]] == WAT_LONG else ar.END_TAIL) for k, v in caps.items())
        _cases[key] = (x, calls, want)
    return _cases[key]


def device_input(x, done, k, dtype, layout):
    """the call's tensor: channel c's next k[c] samples in its first rows, NaN (f32) or 32767 (int16) behind them"""
    import torch
    n_rows = int(k.max())
    rows = np.full((n_rows, x.shape[0]), np.nan if dtype == np.float32 else 32767, dtype=dtype)
    for c in range(x.shape[0]):
        rows[:k[c], c] = x[c, done[c]:done[c] + k[c]]
    if layout == CHANNEL_MAJOR:
        rows = np.ascontiguousarray(rows.T)
    return torch.from_numpy(rows).cuda()


def run_calls(sa, x, rate, calls, dtype, layout, plain, capture):
    """the calls through a ToneDetector: (its events, its chunks per call as the reference lists them)"""
    td = sa.ToneDetector(x.shape[0], rate)
    if capture:
        td.set_audio_capture(*capture)
    done = np.zeros(x.shape[0], np.int64)
    chunks = []
    for k in calls:
        td.process(device_input(x, done, k, dtype, layout), None if plain else k, layout)
        done += k
        td.sync()
        got = td.poll_audio()
        assert all(int(r["reserved"]) == 0 and int(r["n_samples"]) == len(a) and a.dtype == np.float32 for r, a in got)
        chunks.append([(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), a) for r, a in got])
    assert all(td.channel_sample_counter(c) == x.shape[1] for c in range(x.shape[0]))
    return td.poll(), chunks


def assert_same_chunks(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c[:5] for c in g] == [c[:5] for c in w], f"{what}: call {i}"
        for a, b in zip(g, w):
            assert np.array_equal(a[5].view(np.uint32), b[5].view(np.uint32)), f"{what}: call {i} channel {a[0]}"


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("layout", [TIME_MAJOR, CHANNEL_MAJOR], ids=["time", "channel"])
@pytest.mark.parametrize("rate", [8000, 22050])
def test_chunks_equal_the_reference_bit_for_bit(sa, rate, layout, dtype, ragged):
    x, calls, want = case(rate, "main", ragged)
    events, chunks = run_calls(sa, x, rate, calls, dtype, layout, not ragged, (BOTH, TAIL, MAXB, x.size))
    assert_same_chunks(chunks, want, "main")
    plain_events, none = run_calls(sa, x, rate, calls, dtype, layout, not ragged, None)
    assert len(events) >= len(CAPTURING["main"]) and np.array_equal(events, plain_events)
    assert all(call == [] for call in none)


@pytest.mark.parametrize("dtype,layout", [(np.float32, TIME_MAJOR), (np.int16, CHANNEL_MAJOR), (np.int16, TIME_MAJOR), (np.float32, CHANNEL_MAJOR)],
                         ids=["f32-time", "i16-channel", "i16-time", "f32-channel"])
def test_a_group_in_which_nobody_captures_is_skipped(sa, dtype, layout):
    x, calls, want = case(8000, "skip", True)
    events, chunks = run_calls(sa, x, 8000, calls, dtype, layout, False, (BOTH, TAIL, MAXB, x.size))
    assert_same_chunks(chunks, want, "skip")
    assert {c[0] for call in chunks for c in call} == {0, 63, 129}
    assert sum(len(call) for call in chunks) > 6             # the captures came in pieces


@pytest.mark.parametrize("layout", [TIME_MAJOR, CHANNEL_MAJOR], ids=["time", "channel"])
def test_a_pool_that_fills_truncates_as_the_reference_does(sa, layout):
    rate, N = 8000, 320
    base = base_streams(rate)
    x = base[[TWO_TONE, TWO_TONE_OFF, WAT_LONG, NOISE, SILENCE, WAT_LONG]].astype(np.float32)
    calls = calls_of(x.shape[1], 6, False)
    pool = 5 * N
    want = ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, pool)
    assert [c[0] for c in want[-1]] == [0, 1, 2, 5] and [len(c[5]) for c in want[-1]] == [5 * N, 0, 0, 0]     # four capturing channels
    assert all(c[1] & ar.TRUNCATED for c in want[-1])
    _, chunks = run_calls(sa, x, rate, calls, np.float32, layout, True, (BOTH, TAIL, MAXB, pool))
    assert_same_chunks(chunks, want, "pool of 5 N")
    # the state went on regardless: a pool with room gives the whole captures, in the same chunks
    _, whole = run_calls(sa, x, rate, calls, np.int16, layout, True, (BOTH, TAIL, MAXB, x.size))
    assert [[c[:1] + c[2:5] for c in call] for call in whole] == [[c[:1] + c[2:5] for c in call] for call in chunks]
    assert_same_chunks(whole, ar.chunks_of_calls(x, rate, calls, BOTH, TAIL, MAXB, x.size), "pool with room")
    assert [len(c[5]) for c in whole[-1]][::2] == [15 * N, 20 * N]


def test_refusals_and_the_view(sa):
    import torch
    td = sa.ToneDetector(6, 8000)
    for kinds, maxb in ((0, 1), (4, 1), (3, 0)):
        with pytest.raises(sa.SameError) as e:
            td.set_audio_capture(kinds, 0, maxb, 100)
        assert e.value.code == -1
    td.set_audio_capture(BOTH, TAIL, MAXB, 100)
    assert td.poll_audio() == []
    td.process(torch.zeros((10, 6), dtype=torch.float32, device="cuda"))
    with pytest.raises(sa.SameError) as e:                   # behind the handle's first sample
        td.set_audio_capture(BOTH, TAIL, MAXB, 100)
    assert e.value.code == -1
    td.sync()
    assert td.poll_audio() == [] and len(td.poll()) == 0


def run_unpolled(sa, x, rate, calls, dtype, layout, setup):
    """the ragged calls through a ToneDetector that `setup` has put into its mode, with no sync and no poll between them, then
    one sync: a slot is taken again while the samples of the call before are still on the device"""
    td = sa.ToneDetector(x.shape[0], rate)
    setup(td)
    done = np.zeros(x.shape[0], np.int64)
    for k in calls:
        td.process(device_input(x, done, k, dtype, layout), k, layout)
        done += k
    td.sync()
    return td


def raw_view(td, peek, rec_dtype, fields, sample):
    """the view of a raw same_tone_*_peek, as the reference lists chunks: the `fields` of each record, then its samples read through
    the record's pointer"""
    import ctypes
    ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert peek(td._h, ctypes.byref(ptr), ctypes.byref(n)) == 0
    if not n.value:
        return []
    recs = np.frombuffer((ctypes.c_char * (n.value * rec_dtype.itemsize)).from_address(ptr.value), dtype=rec_dtype)
    out = []
    for r in recs:
        k = int(r["n_samples"])
        assert (int(r["samples"]) != 0) == (k != 0)
        a = np.ctypeslib.as_array(ctypes.cast(int(r["samples"]), ctypes.POINTER(sample)), shape=(k,)).copy() if k else np.zeros(0, sample)
        out.append(tuple(int(r[f]) for f in fields) + (a,))
    return out


def assert_view_dropped_in_parts(td, peek, drop, rec_dtype, fields, sample, flat, same):
    """drop 1, peek, drop half of the rest, peek, drop all: after each peek the view is the matching tail of `flat`"""
    view = lambda: raw_view(td, peek, rec_dtype, fields, sample)  # noqa: E731
    n = len(flat)
    assert n > 6
    same([view()], [flat], "the whole view")
    assert drop(td._h, n + 1) < 0                            # more than the view holds: refused, nothing changes
    assert drop(td._h, 1) == 0
    same([view()], [flat[1:]], "behind drop(1)")
    half = (n - 1) // 2
    assert 0 < half < n - 1 and drop(td._h, half) == 0
    same([view()], [flat[1 + half:]], "behind half of the rest")
    assert drop(td._h, n - 1 - half) == 0
    assert view() == [] and drop(td._h, 0) == 0 and drop(td._h, 1) < 0


AUDIO_FIELDS = ("channel", "flags", "kind", "sample_counter", "tone_start")


def unpolled_audio(sa):
    x, calls, want = case(8000, "skip", True)
    # the reference alone: more calls carry samples than there are slots, so a slot is taken again with its samples unfetched
    assert sum(1 for call in want if any(len(c[5]) for c in call)) >= 4
    td = run_unpolled(sa, x, 8000, calls, np.float32, TIME_MAJOR, lambda td: td.set_audio_capture(BOTH, TAIL, MAXB, x.size))
    return td, [c for call in want for c in call]


def test_calls_nobody_polls_between(sa):
    td, flat = unpolled_audio(sa)
    got = td.poll_audio()
    assert all(int(r["reserved"]) == 0 and int(r["n_samples"]) == len(a) and a.dtype == np.float32 for r, a in got)
    assert_same_chunks([[tuple(int(r[f]) for f in AUDIO_FIELDS) + (a,) for r, a in got]], [flat], "one poll behind all calls")
    assert td.poll_audio() == []


def test_a_view_dropped_in_parts(sa):
    import ctypes
    td, flat = unpolled_audio(sa)
    assert_view_dropped_in_parts(td, td._L.same_tone_audio_peek, td._L.same_tone_audio_drop, sa.TONE_AUDIO_CHUNK_DTYPE, AUDIO_FIELDS,
                                 ctypes.c_float, flat, assert_same_chunks)
