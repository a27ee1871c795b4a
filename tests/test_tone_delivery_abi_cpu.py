"""CPU-side checks of the C ABI of tone-alert audio in delivery form (include/same_tone_delivery.h): the library exports every
same_tone_delivery_* name the header declares, the record is 56 bytes with the header's field offsets, null handles are
refused, and the receiver ABI's version did not move."""
import ctypes as C
import os
import re

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
    return open(os.path.join(ROOT, "include", "same_tone_delivery.h")).read()


def test_exports_every_declared_symbol(lib):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(same_tone_delivery_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["same_tone_delivery_drop", "same_tone_delivery_peek", "same_tone_delivery_set"]
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.same_rx_abi_version() == 2
    # the two headers beside it declare no delivery name
    for name in ("same_tones.h", "same_tone_audio.h"):
        assert "same_tone_delivery" not in open(os.path.join(ROOT, "include", name)).read()


def test_the_record_is_56_bytes_with_the_headers_offsets():
    d = sa.TONE_DELIVERY_CHUNK_DTYPE
    assert d.itemsize == 56
    names = ("channel", "flags", "kind", "rate", "sample_counter", "out_index", "n_samples", "tone_start", "samples")
    assert d.names == names and [d.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48]

    # the header's own struct, field by field in its order: uint32 x 4, uint64 x 4, a pointer
    body = re.search(r"typedef struct same_tone_delivery_chunk \{(.*?)\} same_tone_delivery_chunk;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const int16_t \*|uint32_t|uint64_t)\s*(.*)", decl)
        assert m, decl
        for name in m.group(2).split(","):
            fields.append((name.strip(), m.group(1)))
    assert tuple(f[0] for f in fields) == names
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "const int16_t *": C.c_void_p}

    class Chunk(C.Structure):
        _fields_ = [(n, ctype[t]) for n, t in fields]

    assert C.sizeof(Chunk) == 56 and [getattr(Chunk, n).offset for n in names] == [d.fields[n][1] for n in names]


def test_null_handles_are_refused(lib):
    ptr, n = C.c_void_p(), C.c_size_t(7)
    assert lib.same_tone_delivery_set(None, 3, 0, 1, 16, 8000, 1.0) == SAME_EINVAL
    assert b"null" in lib.same_tones_last_error()
    assert lib.same_tone_delivery_peek(None, C.byref(ptr), C.byref(n)) == SAME_EINVAL
    assert lib.same_tone_delivery_drop(None, 0) == SAME_EINVAL
    assert b"null" in lib.same_tones_last_error()
