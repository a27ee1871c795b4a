"""The resampler's per-source calls (same_resampler_process_device_sources) without a device: the host plan
(sameold_amd/csrc/same_resample_plan.h) and the per-source arithmetic of same_resample_dev.h (the text the kernels run)
compiled with plain g++ under ASan + UBSan and driven by tests/helpers/resample_sources_main.cpp the way same_resample.hip
drives them, every channel's samples of every call in a heap block of exactly in_count samples.  Held against the numpy
reference (tests/helpers/resample_reference.py) bit for bit over the whole stream: the nine rates cut into random calls (empty
ones, runs of calls shorter than the history), f32 and int16; per-source and time-major calls alternating at random on one
plan and history; clocks at 2^40, where the 32-bit per-lane phase must be phase_of; resets with and without a new rate."""
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


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("resample_sources")
    exe = str(d / "resample_sources_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "resample_sources_main.cpp"), "-o", exe]
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


def _whole_streams_equal_the_reference(run, tag):
    got = _streams(run, tag)
    assert [g[1] for g in got] == RATES
    for c, rate, x, y in got:
        L, M, T = rr.plan(rate, OUT_RATE)
        assert len(x) == 6000 and len(y) == -(-len(x) * L // M)            # the out_counts sum to ceil(N L / M)
        ref = rr.resample_f32(x, rate, OUT_RATE)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), f"{tag} channel {c} ({rate} Hz)"
        if rate == OUT_RATE:
            assert np.array_equal(y.view(np.uint32), x.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("tag", ["f32", "i16"])
def test_per_source_streams_cut_into_calls_equal_the_reference_over_the_whole_stream(run, tag):
    _whole_streams_equal_the_reference(run, tag)


@pytest.mark.parametrize("tag", ["f32mixed", "i16mixed"])
def test_per_source_and_time_major_calls_share_one_stream(run, tag):
    _whole_streams_equal_the_reference(run, tag)


def test_lane_phase_is_phase_of_and_far_clocks_continue_like_the_reference(run):
    _, lines = run
    assert [w for w in lines if w[0] == "phases"] == [["phases", str(len(RATES) * 400 * 64)]]
    got = _streams(run, "far")
    assert [g[1] for g in got] == RATES
    for c, rate, x, y in got:
        ref = rr.resample_f32(x, rate, OUT_RATE, start_in=(1 << 40) + c)
        assert len(x) == 2000 and len(y) == len(ref)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), f"channel {c} ({rate} Hz)"


@pytest.mark.parametrize("tag", ["f32reset", "i16reset"])
def test_after_a_reset_between_per_source_calls_the_outputs_are_fresh_streams(run, tag):
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
