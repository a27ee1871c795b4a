"""The host half of a harvest, without a GPU: sameold_amd/csrc/same_harvest.cpp is host-only (the event queue, the audio queue, the
replay of a launch's ordered log: ordering, time-parallel stitch, transport layer), so the driver
(tests/helpers/harvest_main.cpp) compiles with plain g++ under ASan + UBSan and, in a second build, under TSan.

tests/golden/harvest_digest.txt holds a digest of what the replay made of the two recorded launches under profiles/harvest/
(three consecutive repetitions each) when that code still lived in same_batch.cpp: it was printed by the commit before the
move, from same_debug_harvest_replay, on one replay thread.  The unit must reproduce it byte for byte on 1, 4 and 32 threads."""
import lzma
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "sameold_amd", "csrc")
SHAPES = ("shard", "headline")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
           TSAN_OPTIONS="halt_on_error=0")


def _build(tmp_path_factory, name, sanitize):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    out = str(tmp_path_factory.mktemp(name) / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + sanitize + ["-fno-omit-frame-pointer", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "helpers", "harvest_main.cpp"),
           os.path.join(CSRC, "same_harvest.cpp"), os.path.join(CSRC, "same_transport.cpp"), "-o", out, "-lm", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "harvest_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def driver_tsan(tmp_path_factory):
    """The TSan build as a command line.  The sanitizer's runtime is linked into the program (it then starts before any shared
    object of the process does), and where the system lets a process switch address-space randomisation off for itself the
    program runs that way: the runtime expects its shadow memory at fixed places, which a wide randomisation can take."""
    out = _build(tmp_path_factory, "harvest_tsan", ["-fsanitize=thread", "-static-libtsan"])
    setarch = shutil.which("setarch")
    fixed = [setarch, os.uname().machine, "-R"] if setarch else []
    if fixed and subprocess.run(fixed + ["true"], capture_output=True).returncode != 0:
        fixed = []
    return fixed + [out]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    d = tmp_path_factory.mktemp("harvest_records")
    paths = {}
    for shape in SHAPES:
        paths[shape] = str(d / f"harvest_{shape}.bin")
        with lzma.open(os.path.join(ROOT, "profiles", "harvest", f"harvest_{shape}.bin.xz")) as src, open(paths[shape], "wb") as dst:
            shutil.copyfileobj(src, dst)
    return paths


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "harvest_digest.txt"), "rb") as f:
        rows = f.read().splitlines()
    assert len(rows) == 3 * len(SHAPES)
    return {shape: b"".join(r + b"\n" for r in rows if r.startswith(shape.encode() + b" ")) for shape in SHAPES}


def _run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, env=ENV, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    for mark in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer", b"LeakSanitizer"):
        assert mark not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("threads", [1, 4, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_replay_of_the_recorded_launches_equals_the_recorded_digest(driver, records, shape, threads):
    want = _golden()[shape]
    assert want.count(b"\n") == 3
    assert _run([driver, "digest", shape, records[shape], str(threads), "3"]) == want


def test_replay_threads_do_not_race(driver_tsan, records):
    assert _run(driver_tsan + ["digest", "shard", records["shard"], "4", "3"]) == _golden()["shard"]


def test_event_log_equals_a_naive_model(driver):
    assert _run([driver, "eventlog"]) == b"OK\n"


def test_audio_log_equals_a_naive_model(driver):
    assert _run([driver, "audiolog"]) == b"OK\n"
