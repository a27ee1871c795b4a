"""The mixed-rate resampler's host plan (sameold_amd/csrc/same_resample_plan.h) and per-output arithmetic
(same_resample_dev.h: the text the device runs) compiled with plain g++ under ASan + UBSan, driven by
tests/helpers/resample_plan_main.cpp the way same_resample.hip drives them, and held against the numpy reference
(tests/helpers/resample_reference.py): ratios and tap counts, the taps against the float64 design, streams cut into random
calls (empty ones, and runs of calls shorter than the history) bit for bit against the f32 reference over the whole stream,
clocks at 2^40, resets with and without a new rate."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_reference as rr  # noqa: E402

OUT_RATE = 22050
RATES = [48000, 44100, 32000, 24000, 16000, 11025, 8000, 96000, 22050]
PLANS = [(147, 320, 36), (1, 2, 32), (441, 640, 24), (147, 160, 18), (441, 320, 16), (2, 1, 16), (441, 160, 16), (147, 640, 70), (1, 1, 1)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("resample")
    exe = str(d / "resample_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "resample_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = d / "out"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(out), "7"], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.decode().split("\n")
    assert lines[-2] == "OK", lines[-4:]
    return str(out), [ln.split() for ln in lines if ln]


def _streams(run, tag):
    """(channel, rate, x, y) of every stream the driver wrote under `tag`"""
    out, lines = run
    got = []
    for w in lines:
        if w[0] == "stream" and w[1] == tag:
            c, rate, n_in, n_out = (int(v) for v in w[2:])
            kind = "i16" if tag.startswith("i16") else "f32"
            x = np.fromfile(os.path.join(out, f"{tag}_c{c}_x.{kind}"), dtype="<i2" if kind == "i16" else "<f4")
            y = np.fromfile(os.path.join(out, f"{tag}_c{c}_y.f32"), dtype="<f4")
            assert len(x) == n_in and len(y) == n_out
            got.append((c, rate, x, y))
    return got


def test_ratios_and_tap_counts(run):
    _, lines = run
    plans = {int(w[1]): tuple(int(v) for v in w[2:]) for w in lines if w[0] == "plan"}
    assert [plans[r] for r in RATES] == PLANS
    assert [rr.plan(r, OUT_RATE) for r in RATES] == PLANS            # the reference agrees with the contract's table too
    assert [w for w in lines if w[0] == "erate"] == [["erate", "192000", "-9"]]           # SAME_ERATE
    assert [w for w in lines if w[0] == "ratios17"] == [["ratios17", "-1"]]               # SAME_EINVAL
    with pytest.raises(ValueError):
        rr.plan(192000, OUT_RATE)
    delays = {int(w[1]): float(w[2]) for w in lines if w[0] == "delay"}
    for r in RATES:
        assert abs(delays[r] - rr.delay(r, OUT_RATE)) < 1e-6
    assert round(delays[48000], 2) == 8.27 and round(delays[8000], 2) == 22.05 and delays[22050] == 0.0


@pytest.mark.parametrize("rate", RATES)
def test_taps_are_the_float64_design_rounded_once(run, rate):
    out, _ = run
    L, M, T = rr.plan(rate, OUT_RATE)
    h = np.fromfile(os.path.join(out, f"taps_{rate}.f32"), dtype="<f4")
    ref = rr.taps64(rate, OUT_RATE)
    assert h.shape == (L * T,) and ref.shape == (L, T)
    err = np.abs(h.astype(np.float64) - ref.reshape(-1)).max()
    print(f"{rate}: largest |tap - float64 design| = {err:.3e}, largest tap {np.abs(h).max():.4f}")
    # a value below 1 rounds to f32 within 2^-25; the bound leaves a factor of four, a design error shows at 1e-4 or more
    assert np.abs(ref).max() < 1.0 or T == 1
    assert err <= 2.0 ** -23


@pytest.mark.parametrize("tag", ["f32", "i16"])
def test_streams_cut_into_calls_equal_the_reference_over_the_whole_stream(run, tag):
    got = _streams(run, tag)
    assert [g[1] for g in got] == RATES
    for c, rate, x, y in got:
        L, M, T = rr.plan(rate, OUT_RATE)
        assert len(x) == 6000 and len(y) == -(-len(x) * L // M)            # the out_counts sum to ceil(N L / M)
        ref = rr.resample_f32(x, rate, OUT_RATE)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), f"{tag} channel {c} ({rate} Hz)"
        if rate == OUT_RATE:
            assert np.array_equal(y.view(np.uint32), x.astype(np.float32).view(np.uint32))


def test_clock_at_2_to_the_40_continues_like_the_reference_there(run):
    got = _streams(run, "far")
    assert [g[1] for g in got] == RATES
    for c, rate, x, y in got:
        ref = rr.resample_f32(x, rate, OUT_RATE, start_in=(1 << 40) + c)
        assert len(x) == 2000 and len(y) == len(ref)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), f"channel {c} ({rate} Hz)"


@pytest.mark.parametrize("tag", ["f32reset", "i16reset"])
def test_after_a_reset_the_outputs_are_a_fresh_streams(run, tag):
    got = _streams(run, tag)
    rates = list(RATES)
    rates[0], rates[3] = 8000, 12000                    # the driver's new sources; channel 5 restarts at its own rate
    assert [g[1] for g in got] == rates
    for c, rate, x, y in got:
        if c not in (0, 3, 5):
            continue                                     # (the others carried on: their streams are checked above)
        ref = rr.resample_f32(x, rate, OUT_RATE)
        assert len(x) == 1500 and len(y) == len(ref)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), f"{tag} channel {c} ({rate} Hz)"


def test_float64_form_is_close_to_the_f32_form():
    """the reference's own two forms against each other, on int16-range noise.  The bound is the f32 format's: with
    A = 32768 * max_p sum_j |h[p][j]| no partial sum exceeds A, each of the T products and T sums rounds within 2^-24 of its
    value, and each tap was rounded within 2^-25 (it is below 1): |f32 - f64| <= 2 T 2^-24 A + T 2^-25 32768."""
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, 20000).astype(np.int16)
    for rate in RATES:
        L, M, T = rr.plan(rate, OUT_RATE)
        A = 32768.0 * np.abs(rr.taps64(rate, OUT_RATE)).sum(axis=1).max()
        bound = 2 * T * 2.0 ** -24 * A + T * 2.0 ** -25 * 32768.0 if T > 1 else 0.0
        d = np.abs(rr.resample_f32(x, rate, OUT_RATE).astype(np.float64) - rr.resample_f64(x, rate, OUT_RATE)).max()
        print(f"{rate}: largest |f32 - f64| = {d:.4f} (bound {bound:.4f})")
        assert d <= bound, (rate, d, bound)
