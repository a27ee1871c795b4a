"""The resampler's per-source calls on the GPU (same_resampler_process_device_sources, Resampler.process_sources /
process_channel_major / process_source_ptrs, MixedRateReceiver.process_sources): every channel from its own device buffer.

1. The kernels against the numpy reference (tests/helpers/resample_reference.py), bit for bit, f32 and int16: 131 channels of
   eight ratios (two full tiles of 64 and a tile of three), counts of 0 (None), 1, 10 and 700, sources that are slices of one
   allocation in shuffled order at odd offsets with a guard sample (NaN / 32767) before and behind each, a sentinel behind
   every channel's outputs; resets between per-source calls.
2. Per-source and time-major calls alternating on one handle: the reference over the whole stream, and a handle fed through
   `process` only.
3. process_channel_major against `process` on the transpose.
4. End to end against the oracle: the three golden recordings at seven rates, each channel its own tensor per call, through
   MixedRateReceiver.process_sources on a strict and on a messages-only batch.
5. The refusals, each with no counter moved."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_reference as rr  # noqa: E402
from test_resample_gpu import E2E_RATES, MIX, OUT_RATE, SENTINEL, _expected_lines, _lines, ob, sa, sources  # noqa: E402,F401

pytestmark = pytest.mark.gpu

C131 = 131
RATES131 = [MIX[c % 7] for c in range(130)] + [96000]


def _blank(dtype):
    return np.nan if dtype == np.float32 else 32767


def _noise(rng, n, dtype):
    if dtype == np.int16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.uniform(-32768.0, 32767.0, n).astype(np.float32)


def _forced_counts(rng, i, hi=700):
    """counts drawn from 0 .. hi with some channels forced to 0, 1, 10 and hi; returns (counts, the channels handed None)"""
    counts = rng.integers(0, hi + 1, C131).astype(np.uint32)
    none = [3 + i, 70 + i, 129]
    counts[none] = 0
    counts[[10 + i, 80 + i, 128, 130]] = 1
    counts[[20 + i, 90 + i]] = min(10, hi)
    counts[[32, 100 + i, 130 if i % 2 else 127]] = hi         # (channel 32 is an 8 kHz source; 130 the 96 kHz one)
    return counts, none


def _slices(rng, counts, none, dtype, logs):
    """seeded noise for every channel as slices of one device allocation: shuffled channel order, each slice at an odd sample
    offset, a guard sample before and behind it.  Appends the samples to logs[c]; returns the list for process_sources."""
    import torch
    C = len(counts)
    pool = np.full(int(counts.sum()) + 3 * C + 8, _blank(dtype), dtype)
    where = [None] * C
    at = 0
    for c in rng.permutation(C):
        start = at + 1                                        # pool[at] stays a guard
        start += 1 - start % 2
        n = int(counts[c])
        v = _noise(rng, n, dtype)
        pool[start:start + n] = v
        logs[c].append(v)
        where[c] = (start, n)
        at = start + n                                        # pool[at] stays a guard
    dev = torch.from_numpy(pool).cuda()
    return [None if c in none else dev[s:s + n] for c, (s, n) in enumerate(where)]


def _source_call(rs, rng, counts, none, dtype, logs):
    """one per-source call; returns (y rows as numpy, out_counts)"""
    import torch
    srcs = _slices(rng, counts, none, dtype, logs)
    for c, t in enumerate(srcs):
        assert t is None or t.numel() == 0 or (t.data_ptr() // t.element_size()) % 2 == 1
    want, rows = rs.out_counts(counts)
    y = torch.full((rows + 3, len(counts)), SENTINEL, dtype=torch.float32, device="cuda")
    _, out = rs.process_sources(srcs, y)
    torch.cuda.synchronize()
    assert np.array_equal(out, want)
    return y.cpu().numpy(), out


def _matrix_call(rs, rng, counts, dtype, logs):
    """one time-major call of the same kind of noise (NaN / 32767 behind every channel's count)"""
    import torch
    C, n_rows = len(counts), max(int(counts.max()), 1)
    x = np.full((n_rows, C), _blank(dtype), dtype)
    for c in range(C):
        v = _noise(rng, int(counts[c]), dtype)
        x[:len(v), c] = v
        logs[c].append(v)
    _, rows = rs.out_counts(counts)
    y = torch.full((rows + 3, C), SENTINEL, dtype=torch.float32, device="cuda")
    _, out = rs.process(torch.from_numpy(x).cuda(), counts, y)
    torch.cuda.synchronize()
    return y.cpu().numpy(), out


def _collect(got, y, out, what):
    for c in range(len(out)):
        got[c].append(y[:out[c], c])
        # rows at or beyond out_counts[c] are never written
        assert np.all(y[out[c]:, c] == np.float32(SENTINEL)), f"{what} channel {c}"


def _whole_stream_equals_the_reference(rs, rates, logs, got):
    for c in range(len(rates)):
        x = np.concatenate(logs[c])
        ref = rr.resample_f32(x, rates[c], OUT_RATE)
        mine = np.concatenate(got[c])
        assert rs.channel_input_counter(c) == len(x) and rs.channel_output_counter(c) == len(ref) == len(mine)
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), f"channel {c} ({rates[c]} Hz)"
        if rates[c] == OUT_RATE:
            assert np.array_equal(mine.view(np.uint32), x.astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------ 1. the kernels against the reference; resets
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_per_source_kernel_equals_the_reference_bit_for_bit(sa, dtype):
    rates = list(RATES131)
    rs = sa.Resampler(rates, OUT_RATE)
    assert len({rs.plan(c)[:2] for c in range(C131)}) == 8
    rng = np.random.default_rng(21 if dtype == np.float32 else 22)
    logs = [[] for _ in range(C131)]
    got = [[] for _ in range(C131)]
    for i in range(4):
        counts, none = _forced_counts(rng, i)
        y, out = _source_call(rs, rng, counts, none, dtype, logs)
        _collect(got, y, out, f"call {i}")
        if i == 0:
            assert out.max() == 1930 and rates[int(out.argmax())] == 8000          # 700 samples at 8 kHz: 31 row tiles
    _whole_stream_equals_the_reference(rs, rates, logs, got)

    # resets between per-source calls: five channels with a new source rate, five at their own; the others carry on
    new = {5: 8000, 17: 48000, 64: 22050, 65: 44100, 129: 16000}
    keep = [0, 2, 63, 66, 128]
    rs.reset_channels(list(new), [new[c] for c in new])
    rs.reset_channels(keep)
    for c in list(new) + keep:
        assert rs.channel_input_counter(c) == 0 and rs.channel_output_counter(c) == 0
        rates[c] = new.get(c, rates[c])
        logs[c] = []
    before = [len(np.concatenate(g)) for g in got]
    counts = rng.integers(1, 701, C131).astype(np.uint32)
    y, out = _source_call(rs, rng, counts, [], dtype, logs)
    for c in range(C131):
        ref = rr.resample_f32(np.concatenate(logs[c]), rates[c], OUT_RATE)
        if c not in new and c not in keep:
            ref = ref[before[c]:]
        assert len(ref) == out[c]
        assert np.array_equal(y[:out[c], c].view(np.uint32), ref.view(np.uint32)), f"after the reset: channel {c} ({rates[c]} Hz)"


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_tiles_of_one_ratio_equal_the_reference_bit_for_bit(sa, dtype):
    """A tile whose 64 channels share one ratio reads its tap table from LDS.  Four such tiles (48 kHz; 32 kHz, the largest
    table that is staged; 8 kHz; three channels at 96 kHz, the longest history), one tile at the output rate (one tap, never
    staged) and one mixed tile between them; then a channel of the 48 kHz tile changes its rate, so that tile takes the other
    path from one call to the next."""
    rates = [48000] * 64 + [32000] * 64 + [MIX[c % 7] for c in range(64)] + [8000] * 64 + [22050] * 64 + [96000] * 3
    C = len(rates)
    rs = sa.Resampler(rates, OUT_RATE)
    rng = np.random.default_rng(25 if dtype == np.float32 else 26)
    logs = [[] for _ in range(C)]
    got = [[] for _ in range(C)]

    def call(i):
        counts = rng.integers(0, 301, C).astype(np.uint32)
        none = [1 + i, 64 + i, 200 + i, C - 1 - i % 2]
        counts[[10 + i, 70 + i, 256 + i]] = 1
        counts[[20, 100, 260, C - 3]] = 300
        counts[none] = 0
        y, out = _source_call(rs, rng, counts, none, dtype, logs)
        _collect(got, y, out, f"call {i}")

    for i in range(3):
        call(i)
    _whole_stream_equals_the_reference(rs, rates, logs, got)
    rs.reset_channels([5], [8000])
    rates[5], logs[5], got[5] = 8000, [], []
    call(3)
    _whole_stream_equals_the_reference(rs, rates, logs, got)


# ------------------------------------------------------------------ 2. both kinds of call on one stream
def test_calls_of_both_kinds_share_one_stream(sa):
    import torch
    rs = sa.Resampler(RATES131, OUT_RATE)
    only_matrix = sa.Resampler(RATES131, OUT_RATE)
    rng = np.random.default_rng(23)
    logs = [[] for _ in range(C131)]
    got = [[] for _ in range(C131)]
    for i in range(6):
        counts, none = _forced_counts(rng, i, hi=10 if i in (2, 3) else 700)      # (calls 2 and 3: one of each kind, shorter than T - 1)
        if i % 2:
            y, out = _source_call(rs, rng, counts, none, np.float32, logs)
        else:
            y, out = _matrix_call(rs, rng, counts, np.float32, logs)
        _collect(got, y, out, f"call {i}")
        # the same samples through `process` on the second handle
        x = np.full((max(int(counts.max()), 1), C131), np.nan, np.float32)
        for c in range(C131):
            x[:counts[c], c] = logs[c][-1]
        y2, out2 = only_matrix.process(torch.from_numpy(x).cuda(), counts)
        torch.cuda.synchronize()
        y2 = y2.cpu().numpy()
        assert np.array_equal(out, out2)
        for c in range(C131):
            assert np.array_equal(y[:out[c], c].view(np.uint32), y2[:out[c], c].view(np.uint32)), f"call {i} channel {c}"
    _whole_stream_equals_the_reference(rs, RATES131, logs, got)


# ------------------------------------------------------------------ 3. channel-major input
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_channel_major_equals_process_on_the_transpose(sa, dtype):
    import torch
    a, b = sa.Resampler(RATES131, OUT_RATE), sa.Resampler(RATES131, OUT_RATE)
    rng = np.random.default_rng(24)
    n_rows = 301
    for i in range(2):
        counts = rng.integers(0, n_rows + 1, C131).astype(np.uint32)
        counts[[1, 64]] = n_rows
        x = np.full((C131, n_rows), _blank(dtype), dtype)
        for c in range(C131):
            x[c, :counts[c]] = _noise(rng, int(counts[c]), dtype)
        ya, outa = a.process_channel_major(torch.from_numpy(x).cuda(), counts)
        yb, outb = b.process(torch.from_numpy(np.ascontiguousarray(x.T)).cuda(), counts)
        torch.cuda.synchronize()
        ya, yb = ya.cpu().numpy(), yb.cpu().numpy()
        assert np.array_equal(outa, outb) and ya.shape == yb.shape
        for c in range(C131):
            assert np.array_equal(ya[:outa[c], c].view(np.uint32), yb[:outa[c], c].view(np.uint32)), f"call {i} channel {c}"
    for c in range(C131):
        assert a.channel_input_counter(c) == b.channel_input_counter(c) and a.channel_output_counter(c) == b.channel_output_counter(c)


# ------------------------------------------------------------------ 4. end to end against the oracle
def _feed_sources(sa, sources, **flags):
    import torch
    n_calls, chans = sources
    rates = [ch[1] for ch in chans]
    rx = sa.MixedRateReceiver(sa.SameReceiverBuilder(OUT_RATE).samedec(), rates, **flags)
    dev = [torch.from_numpy(ch[2]).cuda() for ch in chans]            # one tensor per channel, at its own rate and length
    fed = np.zeros(len(chans), np.int64)
    for i in range(n_calls):
        # each channel its own half second: no padding, no common matrix
        fed += rx.process_sources([d[i * (r // 2):(i + 1) * (r // 2)] for d, r in zip(dev, rates)])
    rx.sync()
    for c, ch in enumerate(chans):
        assert fed[c] == len(ch[3]) == rx.batch.channel_input_sample_counter(c)
    return rx


def test_per_source_mixed_rate_batch_equals_the_oracle_event_for_event(sa, ob, sources):
    rx = _feed_sources(sa, sources)
    events = rx.poll_events()
    got = {}
    for e in events:
        got.setdefault(int(e.channel), []).append((int(e.kind), int(e.sample_counter), int(e.len), e.data()))
    lines = _lines(events)
    for c, (name, rate, _, y) in enumerate(sources[1]):
        ref = [(int(e.kind), int(e.sample_counter), int(e.len), e.data()) for e in ob.Receiver(ob.samedec_config()).run(y)]
        assert got.get(c, []) == ref, f"channel {c}: {name} at {rate} Hz"
        assert lines.get(c, []) == _expected_lines(name), f"channel {c}: {name} at {rate} Hz"

    lines = _lines(_feed_sources(sa, sources, messages_only=True).poll_events())
    for c, (name, rate, _, _) in enumerate(sources[1]):
        assert lines.get(c, []) == _expected_lines(name), f"messages only, channel {c}: {name} at {rate} Hz"


# ------------------------------------------------------------------ 5. refusals
def test_per_source_refusals_move_no_counter(sa):
    import torch
    C, n = 70, 100
    rs = sa.Resampler([MIX[c % 7] for c in range(C)], OUT_RATE)
    f32 = torch.zeros(C * n + 4, dtype=torch.float32, device="cuda")
    i16 = torch.zeros(C * n + 4, dtype=torch.int16, device="cuda")
    counts = np.full(C, n, np.uint32)
    _, rows = rs.out_counts(counts)
    assert rows == 276                                   # ceil(100 * 441 / 160): the 8 kHz channels
    y = torch.empty((rows, C), dtype=torch.float32, device="cuda")
    ptrs = np.uint64(f32.data_ptr()) + np.arange(C, dtype=np.uint64) * np.uint64(4 * n)
    ptrs16 = np.uint64(i16.data_ptr()) + np.arange(C, dtype=np.uint64) * np.uint64(2 * n)

    def counters():
        return [(rs.channel_input_counter(c), rs.channel_output_counter(c)) for c in range(C)]

    zero = counters()

    def refused(p, k, rows_given, i16_call=False):
        with pytest.raises(sa.SameError) as e:
            rs.process_source_ptrs(p, k, y.data_ptr(), rows_given, 0, i16_call)
        assert e.value.code == -1 and counters() == zero

    bad = ptrs.copy()
    bad[69] = 0
    refused(bad, counts, rows)                           # a NULL pointer with a non-zero count
    bad = ptrs16.copy()
    bad[5] += 1
    refused(bad, counts, rows, True)                     # an int16 pointer at an odd byte address
    bad = ptrs.copy()
    bad[0] += 2
    refused(bad, counts, rows)                           # an f32 pointer at base + 2
    refused(ptrs, counts, rows - 1)                      # out_rows one below the largest count
    with pytest.raises(TypeError):                       # float32 and int16 in one list
        rs.process_sources([f32[:n] if c % 2 else i16[:n] for c in range(C)])
    assert counters() == zero
    out = rs.process_source_ptrs(np.zeros(C, np.uint64), np.zeros(C, np.uint32), 0, 0)           # all zero: a no-op
    assert not out.any() and counters() == zero
    _, out = rs.process_sources([None] * C)
    assert not out.any() and counters() == zero
    good = rs.process_source_ptrs(ptrs, counts, y.data_ptr(), rows)
    torch.cuda.synchronize()
    assert counters() == [(n, int(k)) for k in good] and int(good.max()) == rows
