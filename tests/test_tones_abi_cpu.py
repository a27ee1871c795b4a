"""CPU-side checks of the tone detector's C ABI (include/same_tones.h): the library exports every same_tones_* name the header
declares, the receiver ABI's version did not move, a refused rate is refused with or without a device, and without a GPU the
constructor fails loudly (there is no CPU path)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
import sameold_amd as sa
from sameold_amd import build as sbuild

SAME_EINVAL, SAME_ENODEVICE, SAME_EHIP, SAME_ERATE = -1, -5, -6, -9


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    sa.load_library()
    from sameold_amd import tones
    return tones._lib()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "same_tones.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(same_tones_[a-z0-9_]+)\s*\(", text)))


def test_exports_every_declared_symbol(lib):
    syms = declared_symbols()
    assert len(syms) == 14, syms
    for want in ("same_tones_new", "same_tones_free", "same_tones_last_error", "same_tones_n_channels", "same_tones_rate",
                 "same_tones_block_length", "same_tones_coefficients", "same_tones_block_counts", "same_tones_process_device",
                 "same_tones_process_device_i16", "same_tones_sync", "same_tones_poll", "same_tones_reset_channels",
                 "same_tones_channel_sample_counter"):
        assert want in syms
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.same_rx_abi_version() == 2


def test_event_record_and_constants():
    assert sa.TONE_EVENT_DTYPE.itemsize == 32
    assert [sa.TONE_EVENT_DTYPE.fields[n][1] for n in ("channel", "kind", "edge", "reserved", "sample_counter", "duration")] == \
        [0, 4, 8, 12, 16, 24]
    assert (sa.TONE_ATTENTION, sa.TONE_WAT, sa.TONE_START, sa.TONE_END) == (1, 2, 1, 2)
    assert (sa.TONE_START_BLOCKS, sa.TONE_END_BLOCKS) == (25, 5)
    assert (sa.TONE_WAT_SHARE, sa.TONE_ATTENTION_EACH_SHARE, sa.TONE_ATTENTION_SUM_SHARE) == (0.5, 0.15, 0.5)
    assert sa.block_length(22050) == 882 and sa.block_length(8000) == 320 and sa.block_length(48000) == 1920
    text = open(os.path.join(ROOT, "include", "same_tones.h")).read()
    for name, value in (("SAME_TONE_ATTENTION", 1), ("SAME_TONE_WAT", 2), ("SAME_TONE_START", 1), ("SAME_TONE_END", 2)):
        assert re.search(rf"\b{name} = {value}\b", text), name


@pytest.mark.parametrize("rate", [7999, 96001, 0])
def test_a_refused_rate_is_refused_with_or_without_a_device(lib, rate):
    h = C.c_void_p()
    assert lib.same_tones_new(4, rate, 0, C.byref(h)) == SAME_ERATE
    assert not h.value
    assert b"8000" in lib.same_tones_last_error()
    with pytest.raises(sa.SameError) as e:
        sa.ToneDetector(4, rate)
    assert e.value.code == SAME_ERATE


def test_no_cpu_fallback(lib):
    """Without a GPU the constructor must fail, not silently run elsewhere."""
    import torch
    h = C.c_void_p()
    assert lib.same_tones_new(0, 22050, 0, C.byref(h)) == SAME_EINVAL       # zero channels
    # null handles are answered, not dereferenced
    assert lib.same_tones_n_channels(None) == 0 and lib.same_tones_channel_sample_counter(None, 0) == 0
    assert lib.same_tones_sync(None) == SAME_EINVAL
    if torch.cuda.is_available():                        # (where there is a device the constructor works: test_tones_gpu.py)
        td = sa.ToneDetector(64, 22050)
        assert td.n_channels == 64 and td.rate == 22050 and td.block_length == 882
        return
    for rate in (8000, 22050, 96000):
        h = C.c_void_p()
        assert lib.same_tones_new(4, rate, 0, C.byref(h)) in (SAME_ENODEVICE, SAME_EHIP)
        assert not h.value and lib.same_tones_last_error()
    with pytest.raises(sa.SameError) as e:
        sa.ToneDetector(64, 22050)
    assert e.value.code in (SAME_ENODEVICE, SAME_EHIP)
