"""Ties tests/golden/tp_plan.txt (how a call is cut: sameold_amd/csrc/same_tp_plan.cpp, held to the table without a GPU by
tests/test_tp_plan_cpu.py) to the library: a time-parallel batch of 64 channels, fed silence, answers
time_parallel_chunks(), time_parallel_per_channel() and kernel_name() as the table's row for that call says.  Every expected
value is read from the table; no environment knobs; one batch per case."""
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _rows():
    rows = []
    with open(os.path.join(GOLDEN, "tp_plan.txt")) as f:
        for line in f:
            if line.startswith("r=") and " | " in line:
                rows.append(dict(kv.split("=", 1) for kv in line.replace(" | ", " ").split()))
    return rows


ROWS = _rows()
# samples a channel-major call is transposed in at a time (same_batch.cpp, transpose_in_slabs): a longer call is several launches
TRANSPOSE_SLAB = 65520


def row(rate, layout, why=None, n=None):
    """the row of a 64-channel time-parallel batch as created (relaxed arithmetic in the chunks, every setting at its default)"""
    want = dict(r=str(rate), c="64", a="rel", cfg="-/0/0/0/-1/0", l=layout)
    if why is not None:
        want["why"] = why
    if n is not None:
        want["n"] = str(n)
    hits = [r for r in ROWS if all(r[k] == v for k, v in want.items())]
    assert hits, want
    assert all(h == hits[0] or (h["n"], h["k"]) == (hits[0]["n"], hits[0]["k"]) for h in hits)
    return hits[0]


def expected(rate, layout, why):
    """(chunks, per-channel boundaries, kernel) of the call the row describes.  A channel-major call that does not qualify for
    per-channel boundaries is transposed and cut like a time-major call of its length (one slab: these calls are short)."""
    r = row(rate, layout, why)
    n = int(r["n"])
    per_channel = layout == "cm" and r["q"] == "1"
    if layout == "cm" and not per_channel:
        assert n <= TRANSPOSE_SLAB
        r = row(rate, "tm", n=n)
    k = int(r["k"])
    return n, k, per_channel, (r["kern"] if k > 1 else r["plain"])


@pytest.fixture(scope="module")
def sa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sameold_amd import build as sbuild
    sbuild.build()
    import sameold_amd
    sameold_amd.load_library()
    return sameold_amd


@pytest.mark.parametrize("rate", [22050, 48000])
@pytest.mark.parametrize("layout,why", [("tm", "min"), ("tm", "min-1"), ("cm", "tie"), ("cm", "tie+2")])
def test_the_library_cuts_a_call_as_the_table_says(sa, rate, layout, why):
    import torch
    n, k, per_channel, kernel = expected(rate, layout, why)
    if why == "min":
        assert k > 1 and expected(rate, layout, "min-1")[:2] == (n - 1, 1)      # the threshold, and the call below it
    if why == "tie+2":
        assert n % 4 != 0 and not per_channel
    x = torch.zeros((n, 64) if layout == "tm" else (64, n), dtype=torch.float32, device="cuda")
    rx = sa.SameReceiverBuilder(rate).build_batch(64, time_parallel=True)
    rx.process_tensor(x, layout=sa.LAYOUT_TIME_MAJOR if layout == "tm" else sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    assert (rx.time_parallel_chunks(), rx.time_parallel_per_channel(), rx.kernel_name()) == (k, per_channel, kernel)
    assert rx.input_sample_counter() == n
