"""The capture spans of alert audio (sameold_amd/csrc/same_capture_dev.h, walked by the transport kernel of SAME_BATCH_MESSAGES_ONLY
batches with same_batch_set_audio_capture) compiled with plain g++ under ASan + UBSan: random per-channel message streams (SOM,
EOM, a SOM with no EOM before it, several messages on one counter) with flushes and resets, cut into random launches, must give
launch by launch the captures the rule of include/same_rx.h gives over the whole stream; a pool or span list smaller than the
data truncates, marks what it truncated and never writes past either."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    out = str(tmp_path_factory.mktemp("capture") / "capture_spans_fuzz")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(ROOT, "tests", "helpers", "capture_spans_fuzz.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_launch_by_launch_spans_equal_the_rule_over_the_whole_stream(driver, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, "40000", str(seed)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.decode().split("\n")
    assert lines[-2] == "OK", lines[-4:]
    summary = lines[-3]
    assert summary.endswith("equal"), summary
    streams, launches, captures, chunks, truncated, lost = (int(w) for w in re.findall(r"\d+", summary))
    assert streams == 40000 and launches > 200_000 and captures > 200_000 and chunks > captures
    assert truncated > 1000 and lost > 1000, summary       # the tight pools and span lists were exercised


def test_joiner_joins_chunks_into_captures():
    from sameold_amd import receiver as R
    j = R.AudioJoiner()
    a = np.arange(5, dtype=np.float32)
    done = j.feed([(3, 10, R.AUDIO_FIRST, a[:2]), (1, 7, R.AUDIO_FIRST | R.AUDIO_END_FLUSH, a[:0])])
    assert [(d["channel"], d["sample_counter"], d["end"], len(d["samples"])) for d in done] == [(1, 7, R.AUDIO_END_FLUSH, 0)]
    assert list(j.open) == [3]
    done = j.feed([(3, 12, R.AUDIO_END_MESSAGE, a[2:])])
    assert len(done) == 1 and done[0]["channel"] == 3 and done[0]["sample_counter"] == 10
    assert done[0]["end"] == R.AUDIO_END_MESSAGE and np.array_equal(done[0]["samples"], a)
    assert not j.open
    with pytest.raises(ValueError):
        j.feed([(2, 5, 0, a)])                        # outside any capture
    with pytest.raises(ValueError):
        R.AudioJoiner().feed([(2, 5, R.AUDIO_FIRST, a), (2, 11, 0, a)])      # a gap without TRUNCATED
