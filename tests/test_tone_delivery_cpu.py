"""Tone-alert audio in delivery form: the host plan (sameold_amd/csrc/same_tone_delivery_plan.h) and the device core
(same_tone_delivery_dev.h: the text the device runs) compiled with plain g++ under ASan + UBSan, driven by
tests/helpers/tone_delivery_main.cpp the way same_tones.hip and same_tone_delivery.hip drive them (the harvest, the
published view and the drop are the library's own: same_tone_queue.h), and held bit for bit
against the numpy reference (tests/helpers/tone_delivery_reference.py): every chunk's record and int16 samples in queue order,
at 8 000 -> 8 000, 8 000 -> 4 000 (T = 32), 22 050 -> 8 000 (T = 46) and 48 000 -> 8 000 (T = 96, the limit), over three cuts of
the same streams -- one with calls of 1, 1, 2, T - 2, T - 1 and T rows inside open captures and a ragged call that gives a
capturing channel no row -- with a pool that fills, a reset in mid-capture and a gain that clips.  Every test first holds the
reference alone to what the streams were made for.

The one bound that is not bit for bit (test_the_f32_form_stays_within_one_count_of_float64): the quantised f32 form against the
float64 form rounded, over unclamped samples, at most 1 count.  Measured: 0 at 8 000 -> 8 000 and, with gain 1, at 8 000 -> 4 000;
1 at 22 050 -> 8 000 and 48 000 -> 8 000, and at 8 000 -> 4 000 with gain 8.  The f32 sums themselves differ from float64 by at
most 0.0031 counts at gain 1 and 0.0154 at gain 8, so a difference of 1 is a value near a half that rounds the other way."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_reference as rr  # noqa: E402
import tones_reference as tr  # noqa: E402
import tone_audio_reference as ar  # noqa: E402
import tone_delivery_reference as dr  # noqa: E402

BLOCKS = 60
BOTH = tr.ATTENTION | tr.WAT
TAIL, MAXB = 3, 20
TWO_TONE, TWO_TONE_OFF, WAT_LONG, NOISE, SILENCE, WAT_RESET = range(6)
N_CH = 6
CAPTURING = [TWO_TONE, TWO_TONE_OFF, WAT_LONG, WAT_RESET]
CUTS = ("short", "3", "4")
RATES = [(8000, 8000), (8000, 4000), (22050, 8000), (48000, 8000)]
PLANS = {(8000, 8000): (1, 1, 1), (8000, 4000): (1, 2, 32), (22050, 8000): (160, 441, 46), (48000, 8000): (1, 6, 96)}


def make_streams(rate):
    """[6 x 60 blocks] float64 at the int16 scale, the stream kinds of test_tone_audio_cpu.py: tones at 8 000, white noise at
    3 000 as the voice behind them"""
    N = rate // 25
    length = BLOCKS * N
    rng = np.random.default_rng(17)
    A = 8000.0
    x = np.zeros((N_CH, length))
    x[TWO_TONE, 2 * N:34 * N] = A * tr.tone(tr.ATTENTION, 32 * N, rate, 1.0)
    x[TWO_TONE, 34 * N:] = 3000.0 * rng.standard_normal(length - 34 * N)
    x[TWO_TONE_OFF, 2 * N + 7:34 * N + 7] = A * tr.tone(tr.ATTENTION, 32 * N, rate, 1.0)
    x[TWO_TONE_OFF, 34 * N + 7:] = 3000.0 * rng.standard_normal(length - 34 * N - 7)
    x[WAT_LONG] = A * tr.tone(tr.WAT, length, rate, 1.0)
    x[NOISE] = 3000.0 * rng.standard_normal(length)
    x[WAT_RESET] = A * tr.tone(tr.WAT, length, rate, 1.0, 0.7)
    return x


_streams = {}


def streams_of(rate, kind):
    if (rate, kind) not in _streams:
        x = make_streams(rate)
        # (+ 0.0: no -0.0, which int16 cannot carry)
        _streams[(rate, kind)] = (np.round(x) + 0.0).astype(np.float32) if kind == "f32" else np.round(x).astype(np.int16)
    return _streams[(rate, kind)]


def stated_captures(rate):
    """The float reference alone on the whole streams: one capture on every capturing channel, none elsewhere, all of them open
    from block 29 to block 41 -- where the short cut puts its calls."""
    N = rate // 25
    caps = [ar.captures_of_stream(streams_of(rate, "f32")[c], rate, BOTH, TAIL, MAXB) for c in range(N_CH)]
    assert [len(c) for c in caps] == [1, 1, 1, 0, 0, 1]
    for c in CAPTURING:
        assert caps[c][0]["first"] <= 29 * N and caps[c][0]["end"] >= 42 * N and caps[c][0]["flag"] in (ar.END_TAIL, ar.END_MAX)
    return caps


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("tone_delivery")
    path = str(d / "tone_delivery_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "tone_delivery_main.cpp"), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return path


_runs = {}


def run_driver(exe, tmp_path_factory, rate, out_rate, kind, cut, pool, gain=1.0, reset=False):
    """the driver over the streams of `rate`: (calls' counts, {call index: channels reset in front of it}, chunks per call as
    the reference lists them, with the placed rows appended)"""
    key = (rate, out_rate, kind, cut, pool, gain, reset)
    if key in _runs:
        return _runs[key]
    x = streams_of(rate, kind)
    N = rate // 25
    d = tmp_path_factory.mktemp("run")
    src, dst = str(d / "in.bin"), str(d / "out.i16")
    x.tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    args = [exe, src, kind, rate, N_CH, cut, BOTH, TAIL, MAXB, pool, WAT_RESET if reset else -1, 30 * N + 100, out_rate, repr(float(gain)), dst]
    r = subprocess.run([str(a) for a in args], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln]
    assert lines[-1] == ["OK"], lines[-4:]
    assert lines[0] == ["plan"] + [str(v) for v in PLANS[(rate, out_rate)]]
    samples = np.fromfile(dst, dtype="<i2")
    calls, resets, chunks, order = [], {}, [], []
    for w in lines[1:]:
        if w[0] == "call":
            assert int(w[1]) == len(calls)
            calls.append(np.array([int(v) for v in w[2:]], np.int64))
            chunks.append([])
        elif w[0] == "reset":
            resets.setdefault(len(calls), []).append(int(w[1]))
        elif w[0] == "chunk":
            call, c, flags, kind_, at, rows, tone_start, out_index, n, where = (int(v) for v in w[1:])
            chunks[call].append((c, flags, kind_, at, tone_start, out_index, samples[where:where + n], rows))
            order.append((call, c, at))
    assert order == sorted(order)                            # the queue: calls in call order, inside a call by channel, then counter
    _runs[key] = (calls, resets, chunks)
    return _runs[key]


def assert_same_chunks(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c[:6] for c in g] == [c[:6] for c in w], f"{what}: call {i}"
        for a, b in zip(g, w):
            assert a[6].dtype == b[6].dtype == np.int16 and np.array_equal(a[6], b[6]), f"{what}: call {i} channel {a[0]}"


def reference(rate, out_rate, kind, calls, pool, resets, gain=1.0):
    return dr.chunks_of_calls(streams_of(rate, kind), rate, out_rate, gain, calls, BOTH, TAIL, MAXB, pool, resets)


def big_pool(rate):
    return N_CH * BLOCKS * (rate // 25)


@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("rate,out_rate", RATES)
def test_driver_equals_the_reference(exe, tmp_path_factory, rate, out_rate, cut, kind):
    stated_captures(rate)
    L, M, T = rr.plan(rate, out_rate)
    assert (L, M, T) == PLANS[(rate, out_rate)]
    reset = cut != "short"
    calls, resets, chunks = run_driver(exe, tmp_path_factory, rate, out_rate, kind, cut, big_pool(rate), reset=reset)
    want, caps = reference(rate, out_rate, kind, calls, big_pool(rate), resets)
    # the reference alone, before the driver is compared
    flat = [c for call in want for c in call]
    rows = [c[7] for call in chunks for c in call]            # (placed rows: the driver's own, checked below through n_samples)
    assert sorted({cap["channel"] for cap in caps}) == CAPTURING and len(caps) == len(CAPTURING) + (1 if reset else 0)
    assert any(not c[1] & ar.FIRST for c in flat)
    if cut == "short":
        # the short calls lie inside the four open captures: calls of 1, 1, 2, T - 2, T - 1, T rows and the ragged one
        N = rate // 25
        assert not resets and int(calls[0][0]) == 29 * N + 3
        short = [n for n in (1, 1, 2, T - 2, T - 1, T) if n > 0]
        assert [int(k[1]) for k in calls[1:len(short) + 1]] == short and all(len(set(k.tolist())) == 1 for k in calls[:len(short) + 1])
        ragged = calls[len(short) + 1]
        assert ragged.tolist() == [0] + [5] * (N_CH - 1)
        for i in range(1, len(short) + 2):
            assert [c[0] for c in want[i]] == [c for c in CAPTURING if calls[i][c] > 0] and all(c[1] == 0 for c in want[i])
        if T > 2:
            assert sum(1 for k in calls if 0 < k[1] < T - 1) >= 3        # chunks shorter than the history
        if M > L:
            assert any(len(c[6]) == 0 for c in want[1]) or any(len(c[6]) == 0 for c in want[2])      # a 1-row chunk with no output
    else:
        assert len(resets) == 1 and list(resets.values()) == [[WAT_RESET]]
        assert sum(1 for cap in caps if cap["channel"] == WAT_RESET) == 2
    assert_same_chunks(chunks, want, f"{rate} -> {out_rate} {kind} cut {cut}")
    assert not any(c[1] & ar.TRUNCATED for c in flat)
    # a capture's chunks are its delivered stream from output 0 on, with no gap
    at = {}
    for c in [c for call in chunks for c in call]:
        if c[1] & ar.FIRST:
            at[c[0]] = 0
        assert c[5] == at[c[0]]
        at[c[0]] += len(c[6])
    assert len(rows) == len(flat)
    if out_rate == rate:
        # the identity: integer-valued input comes back unchanged
        for cap in caps:
            assert np.array_equal(cap["y"], cap["stream"].astype(np.int16)) and np.array_equal(cap["y"].astype(np.float32), cap["stream"])


@pytest.mark.parametrize("rate,out_rate", RATES)
def test_delivered_streams_do_not_depend_on_the_cut(exe, tmp_path_factory, rate, out_rate):
    caps = stated_captures(rate)
    x = streams_of(rate, "f32")
    L, M, T = rr.plan(rate, out_rate)
    joined = []
    for cut in CUTS:
        calls, resets, chunks = run_driver(exe, tmp_path_factory, rate, out_rate, "f32", cut, big_pool(rate))
        assert not resets
        got = {}
        for call in chunks:
            for c in call:
                got.setdefault(c[0], []).append(c[6])
        joined.append({c: np.concatenate(v) for c, v in got.items()})
    for c in CAPTURING:
        cap = caps[c][0]
        whole = dr.quantise(rr.resample_f32(x[c, cap["first"]:cap["end"]], rate, out_rate), 1.0)
        assert len(whole) == rr.outputs_after(cap["end"] - cap["first"], L, M)
        for j in joined:
            assert np.array_equal(j[c], whole), c
    assert all(sorted(j) == CAPTURING for j in joined)


@pytest.mark.parametrize("rate,out_rate", [(8000, 4000), (22050, 8000)])
def test_a_pool_that_fills_truncates_as_the_float_path_and_the_history_goes_on(exe, tmp_path_factory, rate, out_rate):
    stated_captures(rate)
    N = rate // 25
    L, M, T = rr.plan(rate, out_rate)
    pool = 2 * N + 11
    calls, resets, chunks = run_driver(exe, tmp_path_factory, rate, out_rate, "f32", "short", pool)
    want, caps = reference(rate, out_rate, "f32", calls, pool, resets)
    flat = [c for call in want for c in call]
    assert any(c[1] & ar.TRUNCATED and len(c[6]) == 0 for c in flat) and any(c[1] & ar.TRUNCATED and len(c[6]) > 0 for c in flat)
    # truncated in the first call (29 N + 3 rows hold more than 2 N captured rows) and whole in the short calls behind it
    assert all(c[1] & ar.TRUNCATED for c in want[0][1:]) and not any(c[1] & ar.TRUNCATED for call in want[1:8] for c in call)
    assert_same_chunks(chunks, want, "a pool that fills")
    # the chunks behind a truncated one are what a pool with room gives: the history came from the input
    roomy = run_driver(exe, tmp_path_factory, rate, out_rate, "f32", "short", big_pool(rate))[2]
    for i in range(1, 8):
        assert [c[:6] for c in chunks[i]] == [c[:6] for c in roomy[i]] and all(np.array_equal(a[6], b[6]) for a, b in zip(chunks[i], roomy[i]))


def test_a_gain_that_clips(exe, tmp_path_factory):
    rate, out_rate, gain = 22050, 8000, 8.0
    stated_captures(rate)
    calls, resets, chunks = run_driver(exe, tmp_path_factory, rate, out_rate, "f32", "short", big_pool(rate), gain=gain)
    want, caps = reference(rate, out_rate, "f32", calls, big_pool(rate), resets, gain=gain)
    # the reference alone: the noise behind the tone (3 000 rms, times 8) clips on both sides, and not everywhere
    y = next(cap["y"] for cap in caps if cap["channel"] == TWO_TONE)
    assert (y == 32767).sum() > 10 and (y == -32768).sum() > 10 and (np.abs(y.astype(np.int32)) < 32000).sum() > 10
    v = next(cap["f32"] for cap in caps if cap["channel"] == TWO_TONE) * np.float32(gain)
    assert v.max() > 40000 and v.min() < -40000
    assert_same_chunks(chunks, want, "gain 8")
    assert dr.quantise(np.array([np.nan, np.inf, -np.inf, 0.5, 1.5, 2.5, -0.5, -1.5, 32767.5, -32768.5], np.float32), 1.0).tolist() == \
        [0, 32767, -32768, 0, 2, 2, 0, -2, 32767, -32768]


@pytest.mark.parametrize("rate,out_rate", RATES)
@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_the_f32_form_stays_within_one_count_of_float64(rate, out_rate, gain):
    """Rounding a value whose f32 error is far below half a count moves the result by at most one."""
    caps = stated_captures(rate)
    x = streams_of(rate, "f32")
    worst, worst_sum = 0, 0.0
    for c in CAPTURING:
        s = x[c, caps[c][0]["first"]:caps[c][0]["end"]]
        f32 = rr.resample_f32(s, rate, out_rate)
        y = dr.quantise(f32, gain).astype(np.int64)
        v64 = rr.resample_f64(s, rate, out_rate) * gain
        y64 = np.rint(v64).astype(np.int64)
        keep = (np.abs(y64) < 32767) & (y > -32768) & (y < 32767)
        assert keep.sum() > 100
        worst = max(worst, int(np.abs(y - y64)[keep].max()))
        worst_sum = max(worst_sum, float(np.abs(f32.astype(np.float64) * gain - v64)[keep].max()))
    print(f"{rate} -> {out_rate} gain {gain}: quantised f32 against float64 rounded: {worst} counts; the sums: {worst_sum:.5f} counts")
    assert worst <= 1
