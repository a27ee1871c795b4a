"""The tone detector's host plan (sameold_amd/csrc/same_tones_plan.h) and arithmetic (same_tones_dev.h: the text the device
runs) compiled with plain g++ under ASan + UBSan, driven by tests/helpers/tones_main.cpp the way same_tones.hip drives them,
and held against the numpy reference (tests/helpers/tones_reference.py): every block's four values bit for bit, events and
counters, two cuts of the same streams, a reset in mid-tone, the event bound on its adversarial pattern.  Then the reference
against itself (f32 against float64), on the golden recordings (no tone there) and on generated messages (exactly one tone)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402

RATE, N_CH, LENGTH = 8000, 9, 14000
N = RATE // 25
RESET_CHANNEL, RESET_AFTER = 0, 9000
TEST_RATES = (8000, 22050, 48000)


def make_streams():
    """[9 x 14000] float64 at the int16 scale: tones, noise and silence"""
    rng = np.random.default_rng(11)
    A = 8000.0
    x = np.zeros((N_CH, LENGTH))
    x[0] = A * tr.tone(tr.WAT, LENGTH, RATE, 1.0)                                      # 1050 Hz throughout (reset in mid-tone)
    x[1, 2 * N:34 * N] = A * tr.tone(tr.ATTENTION, 32 * N, RATE, 1.0)                  # the two-tone in blocks 2 .. 33: START and END
    x[2] = 3000.0 * rng.standard_normal(LENGTH)                                        # white noise
    #  3: silence (Em == 0: never qualifies)
    x[4] = A * tr.tone(tr.WAT, LENGTH, RATE * 1.003, 1.0) + 0.3 * A + A * np.sqrt(0.05) * rng.standard_normal(LENGTH)   # 10 dB, DC
    x[5] = A * tr.tone(tr.WAT, LENGTH, RATE, 1.0) * np.linspace(0.0, 1.0, LENGTH) + 800.0 * rng.standard_normal(LENGTH)  # fades in
    for b in range(0, LENGTH // N, 20):                                                # the two-tone 10 blocks on, 10 off: no START
        x[6, b * N:(b + 10) * N] = A * tr.tone(tr.ATTENTION, len(x[6, b * N:(b + 10) * N]), RATE, 1.0)
    x[7] = A * tr.tone(tr.WAT, LENGTH, RATE, 1.0)                                      # 1050 Hz with gaps of 3 blocks: no END
    x[7, 27 * N:30 * N] = 0.0
    x[7, 36 * N + 7:39 * N + 7] = 0.0
    x[8] = 0.8 * A * tr.tone(tr.WAT, LENGTH, RATE, 1.0) + 0.25 * A * tr.tone(tr.ATTENTION, LENGTH, RATE, 1.0)            # both, 1050 wins
    return x


STREAMS = {"f32": make_streams().astype(np.float32), "i16": np.round(make_streams()).astype(np.int16)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("tones")
    path = str(d / "tones_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "tones_main.cpp"), "-o", path]
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


def run_streams(exe, tmp_path_factory, kind, seed, reset):
    """the driver over STREAMS[kind] cut by `seed`: (blocks per channel, events per channel, counters, lines)"""
    key = (kind, seed, reset)
    if key not in _runs:
        d = tmp_path_factory.mktemp(f"run_{kind}_{seed}_{int(reset)}")
        src = str(d / "in.bin")
        STREAMS[kind].tofile(src)
        lines = run_exe(exe, "streams", src, kind, RATE, N_CH, seed, RESET_CHANNEL if reset else -1, RESET_AFTER, d)
        blocks = [np.fromfile(str(d / f"blocks_c{c}.f32"), dtype="<f4").reshape(-1, 4) for c in range(N_CH)]
        events = [[] for _ in range(N_CH)]
        order = []
        for w in lines:
            if w[0] == "event":
                call, c, kind_, edge, at, dur = (int(v) for v in w[1:])
                events[c].append((c, kind_, edge, 0, at, dur))
                order.append((call, c))
        assert order == sorted(order)                    # poll order: calls in call order, inside a call by channel
        counters = {int(w[1]): int(w[2]) for w in lines if w[0] == "counter"}
        _runs[key] = (blocks, events, counters, lines)
    return _runs[key]


def reference(kind, reset_at=None):
    """(blocks per channel, events per channel) of STREAMS[kind]; channel RESET_CHANNEL reset behind reset_at samples"""
    x = STREAMS[kind]
    blocks, events = [], []
    for c in range(N_CH):
        cuts = [x[c]] if reset_at is None or c != RESET_CHANNEL else [x[c, :reset_at], x[c, reset_at:]]
        ch = tr.Channel(c, N)
        bl, ev = [], []
        for part in cuts:
            ch.reset()
            v, E = tr.blocks_f32(part, RATE, True)
            bl.append(v)
            ev += ch.feed(*tr.qualify_f32(v, RATE, E))
        blocks.append(np.concatenate(bl))
        events.append(ev)
    return blocks, events


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_blocks_events_and_counters_equal_the_reference_whatever_the_cut(exe, tmp_path_factory, kind):
    ref_blocks, ref_events = reference(kind)
    first = None
    for seed in (3, 4):
        blocks, events, counters, lines = run_streams(exe, tmp_path_factory, kind, seed, False)
        # the cuts included counts of 0, 1, N - 1, N and N + 1
        assert sorted(int(w[1]) for w in lines if w[0] == "saw") == [0, 1, N - 1, N, N + 1]
        assert [int(w[1]) for w in lines if w[0] == "calls"][0] > 40
        for c in range(N_CH):
            assert blocks[c].shape == ref_blocks[c].shape == (LENGTH // N, 4)
            assert np.array_equal(blocks[c].view(np.uint32), ref_blocks[c].view(np.uint32)), f"{kind} seed {seed} channel {c}"
            assert events[c] == ref_events[c], f"{kind} seed {seed} channel {c}"
            assert counters[c] == LENGTH
        if first is None:
            first = (blocks, events)
        else:                                             # a second cut of the same streams: identical output
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first[0], blocks))
            assert first[1] == events
    # the streams do what they were made for
    kinds = [[(e[1], e[2]) for e in ev] for ev in ref_events]
    assert kinds[0] == [(tr.WAT, tr.START)] and kinds[1] == [(tr.ATTENTION, tr.START), (tr.ATTENTION, tr.END)]
    assert kinds[2] == kinds[3] == kinds[6] == []
    assert kinds[4] == kinds[7] == kinds[8] == [(tr.WAT, tr.START)]
    assert ref_events[1][0][4] == 2 * N and ref_events[1][1][4] == 34 * N and ref_events[1][1][5] == 32 * N


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_reset_in_mid_tone_gives_no_end_and_a_fresh_block_phase(exe, tmp_path_factory, kind):
    blocks, events, counters, lines = run_streams(exe, tmp_path_factory, kind, 5, True)
    resets = [(int(w[1]), int(w[2])) for w in lines if w[0] == "reset"]
    assert len(resets) == 1 and resets[0][0] == RESET_CHANNEL
    at = resets[0][1]
    assert at >= RESET_AFTER and at >= 25 * N            # the 1050 Hz tone of the channel was active
    ref_blocks, ref_events = reference(kind, at)
    for c in range(N_CH):
        assert np.array_equal(blocks[c].view(np.uint32), ref_blocks[c].view(np.uint32)), f"channel {c}"
        assert events[c] == ref_events[c], f"channel {c}"
        assert counters[c] == (LENGTH - at if c == RESET_CHANNEL else LENGTH)
    # one START before the reset, no END, and too few blocks behind it for another START
    assert [(e[1], e[2]) for e in events[RESET_CHANNEL]] == [(tr.WAT, tr.START)]
    assert len(blocks[RESET_CHANNEL]) == at // N + (LENGTH - at) // N


def test_event_bound_holds_with_equality_on_the_adversarial_pattern(exe):
    lines = run_exe(exe, "bound")
    rows = [(int(w[1]), int(w[2]), int(w[3])) for w in lines if w[0] == "bound"]
    assert [r[0] for r in rows] == list(range(201))
    for n, events, limit in rows:
        assert events == limit == tr.events_bound(n) // 2, (n, events, limit)
        # and the reference's state machine on the same pattern
        sm = tr.StateMachine()
        sm.run = tr.START_BLOCKS - 1
        got = sum(sm.step(b == 0 or (b - 1) % 30 >= 5, b, N) is not None for b in range(n))
        assert got == limit
    assert tr.events_bound(0) == 0 and tr.events_bound(1) == 2 and tr.events_bound(50) == 8


def test_numpy_and_glibc_agree_on_the_coefficients(exe):
    lines = run_exe(exe, "coef", *TEST_RATES, 7999, 96001, 96000)
    got = {int(w[1]): (int(w[2]), [int(v, 16) for v in w[3:]]) for w in lines if w[0] == "coef"}
    for rate in TEST_RATES + (96000,):
        n, bits = got[rate]
        assert n == tr.block_length(rate)
        ref = tr.coefficients(rate).view(np.uint32).tolist()
        for k in range(3):
            assert bits[k] == ref[k], f"{rate} Hz, {tr.TONES_HZ[k]} Hz: glibc gives {bits[k]:08x}, numpy {ref[k]:08x}"
    assert sorted((int(w[1]), int(w[2])) for w in lines if w[0] == "erate") == [(7999, -9), (96001, -9)]       # SAME_ERATE
    for rate in (7999, 96001):
        with pytest.raises(ValueError):
            tr.block_length(rate)


def test_f32_and_float64_forms_take_the_same_decisions():
    total = clear = 0
    for kind in ("f32", "i16"):
        x = STREAMS[kind]
        r = tr.ratios_f64(x, RATE)
        a64, w64 = tr.qualify_f64(r, tr.share_f64(x, RATE))
        vals, E = tr.blocks_f32(x, RATE, True)
        a32, w32 = tr.qualify_f32(vals, RATE, E)
        far = tr.clear_of_thresholds(r)
        assert np.array_equal(a32[far], a64[far]) and np.array_equal(w32[far], w64[far])
        total += far.size
        clear += int(far.sum())
    print(f"{clear} of {total} blocks lie at least 0.05 from every threshold")
    assert clear >= 0.95 * total


@pytest.mark.parametrize("name", ["npt", "two_and_two", "long_message"])
def test_golden_recordings_hold_no_tone(name):
    pcm = np.fromfile(os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), dtype="<i2")
    vals, E = tr.blocks_f32(pcm, 22050, True)
    attn, wat = tr.qualify_f32(vals, 22050, E)
    assert not attn.any() and not wat.any()
    r = tr.ratios_f64(pcm, 22050)
    print(f"{name}: {len(r)} blocks, largest ratio {r.max():.5f}")
    assert r.max() < 0.01
    # the f32 form's own ratios, where a block has energy
    ref = vals[:, 3].astype(np.float64) * (882 / 2.0)
    live = ref > 0
    assert (vals[live, :3].astype(np.float64) / ref[live, None]).max() < 0.01


@pytest.mark.parametrize("rate", [22050, 48000])
@pytest.mark.parametrize("kind", [tr.ATTENTION, tr.WAT])
@pytest.mark.parametrize("snr_db,clock", [(None, 1.0), (10.0, 1.003)])
def test_generated_messages_give_one_start_and_one_end(rate, kind, snr_db, clock):
    x, tone_at, tone_len = tr.message(rate, kind, 21, snr_db, clock)
    n = tr.block_length(rate)
    ev = tr.events_of_stream(x, rate)
    assert [(e[1], e[2]) for e in ev] == [(kind, tr.START), (kind, tr.END)], ev
    start, end = ev
    print(f"tone at {tone_at}, START at {start[4]}, duration {end[5]} ({tone_len} made)")
    assert abs(start[4] - tone_at) <= n
    assert end[4] - start[4] == end[5] and abs(end[5] - 3 * rate) <= 2 * n
    # int16 samples of the same message decide alike
    assert [(e[1], e[2], e[4]) for e in tr.events_of_stream(np.round(np.clip(x, -32768, 32767)).astype(np.int16), rate)] == \
        [(e[1], e[2], e[4]) for e in ev]
