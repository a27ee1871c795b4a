"""Ragged calls (same_batch_process_*_ragged), the parts that need no GPU: the four entry points are declared in
include/same_rx.h with the prototypes the issue fixes, exported by the built library and declared by receiver.py; the counter
shifts of ragged launches in the ledger (sameold_amd/csrc/same_resets.h) run a synthesised stream of launches, resets and
harvests under ASan + UBSan against a per-channel model; so does the per-launch arithmetic of a ragged call
(same::ragged_launch_split, the function the batch host calls), over random calls cut into launches at random chunk limits --
limits of 1 and limits beyond the call's largest count among them: every launch's common prefix and lags equal a row-by-row
model's, the lags of a call's launches sum to M - counts[c], and every channel's counter base ends where the model puts it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
import sameold_amd as sa
from sameold_amd import build as sbuild

NAMES = {
    "same_batch_process_device_ragged": "same_batch *rx, const float *d_x, size_t n_rows, const uint32_t *counts, uint32_t layout, void *hip_stream",
    "same_batch_process_device_ragged_i16": "same_batch *rx, const int16_t *d_x, size_t n_rows, const uint32_t *counts, uint32_t layout, void *hip_stream",
    "same_batch_process_host_ragged": "same_batch *rx, const float *h_x, size_t n_rows, const uint32_t *counts, uint32_t layout",
    "same_batch_process_host_ragged_i16": "same_batch *rx, const int16_t *h_x, size_t n_rows, const uint32_t *counts, uint32_t layout",
}


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return sa.load_library()


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "same_rx.h")).read(), flags=re.S)
    m = re.search(r"([A-Za-z_0-9 ]+?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return " ".join(m.group(1).split()), " ".join(m.group(2).split())


def test_header_prototypes():
    for name, args in NAMES.items():
        assert _prototype(name) == ("int", args), name


def test_exported_and_declared(lib):
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert fn.argtypes[2] is C.c_size_t and fn.argtypes[3] == C.POINTER(C.c_uint32)
    assert lib.same_rx_abi_version() == 2
    assert callable(sa.SameBatchReceiver.process_ragged) and callable(sa.SameBatchReceiver.process_host_ragged)


def test_null_handle(lib):
    k = (C.c_uint32 * 1)(0)
    assert lib.same_batch_process_device_ragged(None, None, 0, k, 0, None) == -1
    assert lib.same_batch_process_host_ragged_i16(None, None, 0, k, 0) == -1


def test_ragged_ledger_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    out = str(tmp_path / "ragged_ledger")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Wall", os.path.join(ROOT, "tests", "helpers", "ragged_ledger_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "OK"
