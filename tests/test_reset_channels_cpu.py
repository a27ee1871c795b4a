"""Per-channel reset of a batched receiver (same_batch_reset_channels), the parts that need no GPU: the two entry points are
exported with the prototypes include/same_rx.h gives them and declared by receiver.py, and the bookkeeping that places a
reset's halves in the stream (sameold_amd/csrc/same_resets.h) runs a synthesised stream of launches, harvests and resets
under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
import sameold_amd as sa
from sameold_amd import build as sbuild


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
    assert _prototype("same_batch_reset_channels") == ("int", "same_batch *rx, const uint32_t *channels, size_t n")
    assert _prototype("same_batch_channel_input_sample_counter") == ("uint64_t", "const same_batch *rx, uint32_t channel")


def test_exported_and_declared(lib):
    assert hasattr(lib, "same_batch_reset_channels") and hasattr(lib, "same_batch_channel_input_sample_counter")
    assert lib.same_batch_reset_channels.restype is C.c_int
    assert lib.same_batch_reset_channels.argtypes == [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t]
    assert lib.same_batch_channel_input_sample_counter.restype is C.c_uint64
    assert lib.same_batch_channel_input_sample_counter.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.same_rx_abi_version() == 2
    assert callable(sa.decode_recordings)
    assert callable(sa.SameBatchReceiver.reset_channels) and callable(sa.SameBatchReceiver.channel_input_sample_counter)


def test_null_handle(lib):
    ch = (C.c_uint32 * 1)(0)
    assert lib.same_batch_reset_channels(None, ch, 1) == -1
    assert lib.same_batch_channel_input_sample_counter(None, 0) == 0


def test_reset_ledger_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    out = str(tmp_path / "reset_ledger")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Wall", os.path.join(ROOT, "tests", "helpers", "reset_ledger_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "OK"
