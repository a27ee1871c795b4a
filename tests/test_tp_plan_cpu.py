"""How a call is cut, without a GPU: sameold_amd/csrc/same_tp_plan.cpp is host-only arithmetic (the launch cap, the uniform
time-parallel cut, the plan of a channel-major call with per-channel boundaries, the output capacities), so the driver
(tests/helpers/tp_plan_main.cpp) compiles with plain g++ under ASan + UBSan and prints every output of the unit over a grid of
rates, channel counts, arithmetics, SAME_TP_KERNEL / SAME_TP_SORT settings, same_batch_time_parallel_config values and both
layouts -- at the shortest call that is cut and the one a sample shorter, at the headline length, and at each qualification
limit of the channel-major plan with its neighbour.  tests/golden/tp_plan.txt was printed by the same driver over the
expressions as they stood in same_batch.cpp before they moved (tests/golden/README.md has them); the unit must reproduce it
byte for byte."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "sameold_amd", "csrc")


def test_tp_plan_equals_the_recorded_table(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    out = str(tmp_path / "tp_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "helpers", "tp_plan_main.cpp"), os.path.join(CSRC, "same_tp_plan.cpp"),
           os.path.join(CSRC, "same_select.cpp"), os.path.join(CSRC, "same_config.cpp"), "-o", out, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    with open(os.path.join(ROOT, "tests", "golden", "tp_plan.txt"), "rb") as f:
        want = f.read()
    got_rows, want_rows = r.stdout.split(b"\n"), want.split(b"\n")
    assert len(got_rows) == len(want_rows) and len(want_rows) > 300
    wrong = [(g, w) for g, w in zip(got_rows, want_rows) if g != w]
    assert not wrong, (len(wrong), wrong[:3])


def test_the_unit_needs_no_hip():
    """same_tp_plan.* includes only the host-only headers, and compiles with nothing of HIP on the include path"""
    for name in ("same_tp_plan.h", "same_tp_plan.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            quoted = [ln.split('"')[1] for ln in f if ln.startswith("#include \"")]
        assert set(quoted) <= {"same_tp_plan.h", "same_select.h", "same_device.h", "same_config.h"}, (name, quoted)
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(CSRC, "same_tp_plan.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
