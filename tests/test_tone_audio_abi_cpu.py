"""CPU-side checks of tone-alert audio's C ABI (include/same_tone_audio.h): the library exports every same_tone_audio_* name
the header declares, the receiver ABI's version did not move, the header's constants are the package's, null handles are
answered, and -- where there is a device -- same_tone_audio_set behind the first sample is refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import sameold_amd as sa
from sameold_amd import build as sbuild

SAME_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    sa.load_library()
    from sameold_amd import tones
    return tones._lib()


def header():
    return open(os.path.join(ROOT, "include", "same_tone_audio.h")).read()


def test_exports_every_declared_symbol(lib):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(same_tone_audio_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["same_tone_audio_chunk_bound", "same_tone_audio_drop", "same_tone_audio_peek", "same_tone_audio_set"]
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.same_rx_abi_version() == 2
    # same_tones.h was not touched: it declares what it declared
    tones_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "same_tones.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(same_tones_[a-z0-9_]+)\s*\(", tones_h))) == 14 and "same_tone_audio" not in tones_h


def test_chunk_record_constants_and_bound(lib):
    assert sa.TONE_AUDIO_CHUNK_DTYPE.itemsize == 48
    assert [sa.TONE_AUDIO_CHUNK_DTYPE.fields[n][1] for n in ("channel", "flags", "kind", "reserved", "sample_counter", "n_samples",
                                                             "tone_start", "samples")] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert (sa.TONE_AUDIO_FIRST, sa.TONE_AUDIO_END_TAIL, sa.TONE_AUDIO_END_MAX, sa.TONE_AUDIO_TRUNCATED) == (1, 2, 4, 8)
    assert sa.TONE_AUDIO_END == 6
    text = header()
    for name, value in (("FIRST", 1), ("END_TAIL", 2), ("END_MAX", 4), ("TRUNCATED", 8)):
        assert re.search(rf"\bSAME_TONE_AUDIO_{name} = {value}\b", text), name
    for n in list(range(0, 100)) + [1000, 2 ** 31]:
        assert lib.same_tone_audio_chunk_bound(n) == sa.tone_audio_chunk_bound(n) == 1 + (n + 28) // 30 + (n + 26) // 30


def test_null_handles_are_answered(lib):
    ptr, n = C.c_void_p(), C.c_size_t(7)
    assert lib.same_tone_audio_set(None, 3, 0, 1, 16) == SAME_EINVAL
    assert lib.same_tone_audio_peek(None, C.byref(ptr), C.byref(n)) == SAME_EINVAL
    assert lib.same_tone_audio_drop(None, 0) == SAME_EINVAL
    assert b"null" in lib.same_tones_last_error()


def test_set_is_checked_and_refused_behind_the_first_sample(lib):
    import torch
    if not torch.cuda.is_available():
        # there is no handle without a device (test_tones_abi_cpu.py); the refusals are test_tone_audio_gpu.py's then
        with pytest.raises(sa.SameError):
            sa.ToneDetector(4, 8000)
        return
    td = sa.ToneDetector(4, 8000)
    for kinds, tail, maxb in ((0, 0, 1), (4, 0, 1), (7, 0, 1), (3, 0, 0)):
        with pytest.raises(sa.SameError) as e:
            td.set_audio_capture(kinds, tail, maxb, 1000)
        assert e.value.code == SAME_EINVAL
    td.set_audio_capture(sa.TONE_WAT, 0, 1, 1000)
    td.set_audio_capture(0, 0, 0, 0)                          # off: the other arguments are not looked at
    td.set_audio_capture(sa.TONE_WAT | sa.TONE_ATTENTION, 3, 20, 1000)
    assert td.poll_audio() == []
    td.process(torch.zeros((10, 4), dtype=torch.float32, device="cuda"))
    td.sync()
    with pytest.raises(sa.SameError) as e:
        td.set_audio_capture(sa.TONE_WAT, 0, 1, 1000)
    assert e.value.code == SAME_EINVAL
    with pytest.raises(sa.SameError) as e:
        td.set_audio_capture(0, 0, 0, 0)
    assert e.value.code == SAME_EINVAL
    assert td.poll_audio() == [] and np.array_equal(td.poll(), td.poll())
