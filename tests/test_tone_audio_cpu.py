"""Tone-alert audio's host plan (sameold_amd/csrc/same_tone_audio_plan.h) and device core (same_tone_audio_dev.h: the text the
device runs) compiled with plain g++ under ASan + UBSan, driven by tests/helpers/tone_audio_main.cpp the way same_tones.hip and
same_tone_audio.hip drive them -- the harvest, the published view and the drop are the library's own (same_tone_queue.h) --
and held against the numpy reference (tests/helpers/tone_audio_reference.py): every chunk's samples bit for bit, flags, counters and the queue order, three cuts of the same streams, a pool that fills, a reset in
mid-capture, a tail that bridges two tones, the chunk bound on its adversarial pattern.  Every test first holds the reference
alone to the captures the streams were made for."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402
import tone_audio_reference as ar  # noqa: E402

RATE = 8000
N = RATE // 25
BLOCKS = 60
LENGTH = BLOCKS * N
BOTH = tr.ATTENTION | tr.WAT
TAIL, MAXB = 3, 20
TWO_TONE, TWO_TONE_OFF, WAT_LONG, NOISE, SILENCE, WAT_RESET = range(6)
N_CH = 6
RESET_AFTER = 30 * N + 100
BIG_POOL = N_CH * LENGTH
CUTS = ("fixed", "3", "4")


def make_streams():
    """[6 x 60 blocks] float64 at the int16 scale: tones at 8 000, white noise at 3 000 as the voice behind them"""
    rng = np.random.default_rng(17)
    A = 8000.0
    x = np.zeros((N_CH, LENGTH))
    x[TWO_TONE, 2 * N:34 * N] = A * tr.tone(tr.ATTENTION, 32 * N, RATE, 1.0)               # the two-tone in blocks 2 .. 33
    x[TWO_TONE, 34 * N:] = 3000.0 * rng.standard_normal(LENGTH - 34 * N)
    x[TWO_TONE_OFF, 2 * N + 7:34 * N + 7] = A * tr.tone(tr.ATTENTION, 32 * N, RATE, 1.0)   # the same, 7 samples late
    x[TWO_TONE_OFF, 34 * N + 7:] = 3000.0 * rng.standard_normal(LENGTH - 34 * N - 7)
    x[WAT_LONG] = A * tr.tone(tr.WAT, LENGTH, RATE, 1.0)                                   # 1050 Hz throughout: END_MAX
    x[NOISE] = 3000.0 * rng.standard_normal(LENGTH)
    #  SILENCE: zeros
    x[WAT_RESET] = A * tr.tone(tr.WAT, LENGTH, RATE, 1.0, 0.7)                             # 1050 Hz throughout, reset in mid-capture
    return x


def make_bridge():
    """[1 x 120 blocks]: tone 30 blocks, noise 8 blocks, tone 30 blocks, noise"""
    rng = np.random.default_rng(18)
    x = 3000.0 * rng.standard_normal((1, 120 * N))
    x[0, :30 * N] = 8000.0 * tr.tone(tr.WAT, 30 * N, RATE, 1.0)
    x[0, 38 * N:68 * N] = 8000.0 * tr.tone(tr.WAT, 30 * N, RATE, 1.0)
    return x


# (+ 0.0: no -0.0, which int16 cannot carry)
STREAMS = {"f32": (np.round(make_streams()) + 0.0).astype(np.float32), "i16": np.round(make_streams()).astype(np.int16)}
BRIDGE = (np.round(make_bridge()) + 0.0).astype(np.float32)


def stated_captures():
    """The reference alone on the whole streams: the captures they were made for.  Returns them per channel."""
    caps = [ar.captures_of_stream(STREAMS["f32"][c], RATE, BOTH, TAIL, MAXB) for c in range(N_CH)]
    assert [len(c) for c in caps] == [1, 1, 1, 0, 0, 1]
    a = caps[TWO_TONE][0]
    assert (a["first"], a["end"], a["flag"], a["kind"], a["tone_start"]) == (27 * N, (42 + TAIL - 3) * N, ar.END_TAIL, tr.ATTENTION, 2 * N)
    assert len(a["samples"]) == 15 * N                                                     # blocks 27 .. 41
    b = caps[TWO_TONE_OFF][0]
    assert b["flag"] == ar.END_TAIL and b["first"] % N == 0 and b["end"] % N == 0 and abs(b["first"] - 27 * N) <= N
    for ch in (WAT_LONG, WAT_RESET):
        w = caps[ch][0]
        assert (w["first"], w["end"], w["flag"], w["kind"], w["tone_start"]) == (25 * N, 45 * N, ar.END_MAX, tr.WAT, 0)    # blocks 25 .. 44
    # and with one kind disabled its tones give nothing
    assert [len(ar.captures_of_stream(STREAMS["f32"][c], RATE, tr.ATTENTION, TAIL, MAXB)) for c in range(N_CH)] == [1, 1, 0, 0, 0, 0]
    assert [len(ar.captures_of_stream(STREAMS["f32"][c], RATE, tr.WAT, TAIL, MAXB)) for c in range(N_CH)] == [0, 0, 1, 0, 0, 1]
    return caps


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("tone_audio")
    path = str(d / "tone_audio_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "tone_audio_main.cpp"), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return path


def run_exe(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln]
    assert lines[-1] == ["OK"], lines[-4:]
    return lines


_runs = {}


def run_driver(exe, tmp_path_factory, streams, kind, cut, kinds, tail, maxb, pool, reset=False):
    """the driver over `streams`: (calls' counts, {call index: channels reset in front of it}, chunks per call as the
    reference lists them, events per channel)"""
    key = (streams.shape, kind, cut, kinds, tail, maxb, pool, reset)
    if key in _runs:
        return _runs[key]
    d = tmp_path_factory.mktemp("run")
    src, dst = str(d / "in.bin"), str(d / "out.f32")
    streams.tofile(src)
    lines = run_exe(exe, "streams", src, kind, RATE, streams.shape[0], cut, kinds, tail, maxb, pool, WAT_RESET if reset else -1,
                    RESET_AFTER, dst)
    samples = np.fromfile(dst, dtype="<f4")
    calls, resets, chunks, order = [], {}, [], []
    events = [[] for _ in range(streams.shape[0])]
    for w in lines:
        if w[0] == "call":
            assert int(w[1]) == len(calls)
            calls.append(np.array([int(v) for v in w[2:]], np.int64))
            chunks.append([])
        elif w[0] == "reset":
            resets.setdefault(len(calls), []).append(int(w[1]))
        elif w[0] == "event":
            call, c, kind_, edge, at, dur = (int(v) for v in w[1:])
            events[c].append((c, kind_, edge, 0, at, dur))
        elif w[0] == "chunk":
            call, c, flags, kind_, at, n, tone_start, where = (int(v) for v in w[1:])
            chunks[call].append((c, flags, kind_, at, tone_start, samples[where:where + n]))
            order.append((call, c, at))
    assert order == sorted(order)                            # the queue: calls in call order, inside a call by channel, then counter
    _runs[key] = (calls, resets, chunks, events)
    return _runs[key]


def assert_same_chunks(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c[:5] for c in g] == [c[:5] for c in w], f"{what}: call {i}"
        for a, b in zip(g, w):
            assert a[5].dtype == b[5].dtype == np.float32 and np.array_equal(a[5].view(np.uint32), b[5].view(np.uint32)), f"{what}: call {i} channel {a[0]}"


@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("cut", CUTS)
def test_driver_equals_the_reference(exe, tmp_path_factory, kind, cut):
    stated_captures()
    x = STREAMS[kind]
    reset = cut != "fixed"                                   # (the fixed cut's last call takes the rest: no call to reset behind)
    calls, resets, chunks, events = run_driver(exe, tmp_path_factory, x, kind, cut, BOTH, TAIL, MAXB, BIG_POOL, reset=reset)
    want = ar.chunks_of_calls(x, RATE, calls, BOTH, TAIL, MAXB, BIG_POOL, resets)
    assert_same_chunks(chunks, want, f"{kind} cut {cut}")
    assert not any(c[1] & ar.TRUNCATED for call in chunks for c in call)
    got = ar.join(chunks)
    per_channel = [[k for k in got if k[0] == c] for c in range(N_CH)]
    if not reset:
        assert not resets and [len(p) for p in per_channel] == [1, 1, 1, 0, 0, 1]
        return
    assert len(resets) == 1 and list(resets.values()) == [[WAT_RESET]]
    # the reset channel: its capture is open at the reset and dropped with no END flag; a second one opens behind it and stays open
    assert [len(p) for p in per_channel] == [1, 1, 1, 0, 0, 2]
    at = int(sum(k[WAT_RESET] for k in calls[:list(resets)[0]]))
    assert 25 * N < at < 45 * N
    first, second = sorted(per_channel[WAT_RESET], key=lambda k: k[3])
    assert first[:3] == second[:3] == (WAT_RESET, 0, 25 * N)      # (the counters begin again at the reset)
    assert got[first][1] == ar.FIRST and len(got[first][0]) == at - 25 * N
    assert np.array_equal(got[first][0], x[WAT_RESET, 25 * N:at].astype(np.float32))
    assert got[second][1] == ar.FIRST and len(got[second][0]) == LENGTH - at - 25 * N
    # the tone events beside the capture are the detector's
    for c in range(N_CH):
        ch = tr.Channel(c, N)
        parts = [x[c]] if c != WAT_RESET else [x[c, :at], x[c, at:]]
        ref = []
        for part in parts:
            ch.reset()
            vals, E = tr.blocks_f32(part, RATE, True)
            ref += ch.feed(*tr.qualify_f32(vals, RATE, E))
        assert events[c] == ref, f"channel {c}"


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_captures_do_not_depend_on_the_cut(exe, tmp_path_factory, kind):
    caps = stated_captures()
    joined = []
    for cut in CUTS:
        calls, resets, chunks, _ = run_driver(exe, tmp_path_factory, STREAMS[kind], kind, cut, BOTH, TAIL, MAXB, BIG_POOL)
        assert not resets and (cut == "fixed") == (len(calls) == 6)
        if cut == "fixed":
            assert [int(k[0]) for k in calls] == [1, 319, 320, 321, 1000, LENGTH - 1961]
        else:
            assert len(calls) > 40 and any(len(set(k.tolist())) > 1 for k in calls)      # ragged counts
        joined.append(ar.join(chunks))
    assert sorted(joined[0]) == sorted((c, caps[c][0]["tone_start"], caps[c][0]["first"], 0) for c in (TWO_TONE, TWO_TONE_OFF, WAT_LONG, WAT_RESET))
    for key, (samples, flags, kind_) in joined[0].items():
        cap = caps[key[0]][0]
        assert flags == (ar.FIRST | cap["flag"]) and kind_ == cap["kind"]
        assert np.array_equal(samples.view(np.uint32), cap["samples"].view(np.uint32))    # (f32 and int16 hold the same integers)
        for other in joined[1:]:
            assert other[key][1:] == (flags, kind_) and np.array_equal(other[key][0].view(np.uint32), samples.view(np.uint32))
    assert all(sorted(j) == sorted(joined[0]) for j in joined)


def test_a_pool_that_fills_truncates_as_the_reference_does(exe, tmp_path_factory):
    stated_captures()
    x = STREAMS["f32"]
    pool = 5 * N
    calls, resets, chunks, _ = run_driver(exe, tmp_path_factory, x, "f32", "fixed", BOTH, TAIL, MAXB, pool)
    want = ar.chunks_of_calls(x, RATE, calls, BOTH, TAIL, MAXB, pool, resets)
    assert_same_chunks(chunks, want, "pool of 5 N")
    last = chunks[-1]                                        # the call that holds all four captures
    assert [c[0] for c in last] == [TWO_TONE, TWO_TONE_OFF, WAT_LONG, WAT_RESET]
    assert [len(c[5]) for c in last] == [5 * N, 0, 0, 0]
    assert all(c[1] & ar.TRUNCATED for c in last) and all(c[1] & ar.FIRST and c[1] & ar.END for c in last)
    assert sum(len(c[5]) for call in chunks for c in call) == pool


@pytest.mark.parametrize("kinds,capturing", [(tr.ATTENTION, [TWO_TONE, TWO_TONE_OFF]), (tr.WAT, [WAT_LONG, WAT_RESET])])
def test_a_disabled_kind_captures_nothing(exe, tmp_path_factory, kinds, capturing):
    stated_captures()
    x = STREAMS["i16"]
    calls, resets, chunks, _ = run_driver(exe, tmp_path_factory, x, "i16", "3", kinds, TAIL, MAXB, BIG_POOL)
    assert_same_chunks(chunks, ar.chunks_of_calls(x, RATE, calls, kinds, TAIL, MAXB, BIG_POOL), f"kinds {kinds}")
    assert sorted({k[0] for k in ar.join(chunks)}) == capturing


@pytest.mark.parametrize("cut", CUTS)
def test_a_long_tail_bridges_two_tones(exe, tmp_path_factory, cut):
    caps = ar.captures_of_stream(BRIDGE[0], RATE, BOTH, 40, 200)
    assert len(caps) == 1                                    # one capture across both tones
    cap = caps[0]
    assert (cap["first"], cap["end"], cap["flag"], cap["tone_start"]) == (25 * N, (68 + 5 + 40) * N, ar.END_TAIL, 0)       # end + (5 + tail_blocks) N
    assert len(ar.captures_of_stream(BRIDGE[0], RATE, BOTH, TAIL, 200)) == 2          # (a short tail gives two)
    calls, resets, chunks, events = run_driver(exe, tmp_path_factory, BRIDGE, "f32", cut, BOTH, 40, 200, 120 * N)
    assert_same_chunks(chunks, ar.chunks_of_calls(BRIDGE, RATE, calls, BOTH, 40, 200, 120 * N), f"cut {cut}")
    got = ar.join(chunks)
    assert list(got) == [(0, 0, 25 * N, 0)]
    samples, flags, kind = got[(0, 0, 25 * N, 0)]
    assert flags == ar.FIRST | ar.END_TAIL and kind == tr.WAT and np.array_equal(samples.view(np.uint32), cap["samples"].view(np.uint32))
    assert [(e[1], e[2]) for e in events[0]] == [(tr.WAT, tr.START), (tr.WAT, tr.END)] * 2     # the second START re-armed the tail


def test_chunk_bound_holds_with_equality_on_the_adversarial_pattern(exe):
    stated_captures()
    lines = run_exe(exe, "bound")
    rows = [(int(w[1]), int(w[2]), int(w[3])) for w in lines if w[0] == "bound"]
    assert [r[0] for r in rows] == list(range(201))
    for n, chunks, limit in rows:
        assert chunks == limit == ar.chunk_bound(n), (n, chunks, limit)
    assert ar.chunk_bound(0) == 1 and ar.chunk_bound(1) == 1 and ar.chunk_bound(4) == 3 and ar.chunk_bound(50) == 5
    # the pattern opens a capture in blocks 1, 3, 31, 33, ... beside the one that was open on entry
    for n in range(201):
        assert 1 + sum(1 for b in range(n) if b % 30 in (1, 3)) == ar.chunk_bound(n)
