"""The mixed-rate resampler on the GPU (include/same_resample.h, sameold_amd/resample.py).

1. The kernels against the numpy reference (tests/helpers/resample_reference.py), bit for bit: 130 channels whose rates change
   from lane to lane, ragged calls with empty, one-sample and ten-sample channels, NaN behind every channel's count, a
   sentinel behind every channel's outputs, f32 and int16 input, resets with and without a new rate.
2. End to end against the oracle: the three golden recordings, each at seven source rates, through MixedRateReceiver on a
   strict batch -- every event the oracle's on the numpy-resampled stream, every channel's messages its golden text; the same
   through a messages-only batch.
3. The refusals, each with its code and no counter moved."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_RATE = 22050
MIX = [48000, 44100, 22050, 16000, 8000, 11025, 32000]
SENTINEL = -12345.5


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


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    binding.lib()
    return binding


# ------------------------------------------------------------------ 1. the kernels against the reference
def _blank(dtype):
    return np.nan if dtype == np.float32 else 32767


def _noise(rng, n, dtype):
    if dtype == np.int16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.uniform(-32768.0, 32767.0, n).astype(np.float32)


def _call(rs, rng, n_rows, counts, dtype, logs):
    """one call of seeded noise; appends every channel's samples to logs[c]; returns (y rows as numpy, out_counts)"""
    import torch
    C = len(counts)
    x = np.full((n_rows, C), _blank(dtype), dtype)
    for c in range(C):
        v = _noise(rng, int(counts[c]), dtype)
        x[:len(v), c] = v
        logs[c].append(v)
    want, rows = rs.out_counts(counts)
    y = torch.full((rows + 3, C), SENTINEL, dtype=torch.float32, device="cuda")
    _, out = rs.process(torch.from_numpy(x).cuda(), counts, y)
    torch.cuda.synchronize()
    assert np.array_equal(out, want)
    return y.cpu().numpy(), out


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_kernel_equals_the_reference_bit_for_bit(sa, dtype):
    C, n_rows, n_calls = 130, 700, 4
    rates = [MIX[c % 7] for c in range(C)]
    rs = sa.Resampler(rates, OUT_RATE)
    rng = np.random.default_rng(11 if dtype == np.float32 else 12)
    logs = [[] for _ in range(C)]
    got = [[] for _ in range(C)]
    for i in range(n_calls):
        counts = rng.integers(0, n_rows + 1, C).astype(np.uint32)
        counts[[3 + i, 70 + i, 129]] = 0
        counts[[10 + i, 80 + i, 128]] = 1
        counts[[20 + i, 90 + i]] = 10
        counts[[32, 100 + i]] = n_rows                      # (channel 32 is an 8 kHz source)
        y, out = _call(rs, rng, n_rows, counts, dtype, logs)
        for c in range(C):
            got[c].append(y[:out[c], c])
            # rows at or beyond out_counts[c] are never written
            assert np.all(y[out[c]:, c] == np.float32(SENTINEL)), f"call {i} channel {c}"
        if i == 0:
            assert out.max() == 1930 and rates[int(out.argmax())] == 8000          # 700 rows at 8 kHz: across the row blocks
    for c in range(C):
        x = np.concatenate(logs[c])
        ref = rr.resample_f32(x, rates[c], OUT_RATE)
        mine = np.concatenate(got[c])
        assert rs.channel_input_counter(c) == len(x) and rs.channel_output_counter(c) == len(ref) == len(mine)
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), f"channel {c} ({rates[c]} Hz)"
        if rates[c] == OUT_RATE:
            assert np.array_equal(mine.view(np.uint32), x.astype(np.float32).view(np.uint32))

    # resets: five channels with a new source rate, five at their own; the others carry on
    new = {5: 8000, 17: 48000, 64: 22050, 65: 44100, 129: 16000}
    keep = [0, 2, 63, 66, 128]
    rs.reset_channels(list(new), [new[c] for c in new])
    rs.reset_channels(keep)
    for c in list(new) + keep:
        assert rs.channel_input_counter(c) == 0 and rs.channel_output_counter(c) == 0
        rates[c] = new.get(c, rates[c])
        logs[c] = []
    before = [len(np.concatenate(g)) for g in got]
    counts = rng.integers(1, n_rows + 1, C).astype(np.uint32)
    y, out = _call(rs, rng, n_rows, counts, dtype, logs)
    for c in range(C):
        ref = rr.resample_f32(np.concatenate(logs[c]), rates[c], OUT_RATE)
        if c not in new and c not in keep:
            ref = ref[before[c]:]
        assert len(ref) == out[c]
        assert np.array_equal(y[:out[c], c].view(np.uint32), ref.view(np.uint32)), f"after the reset: channel {c} ({rates[c]} Hz)"


# ------------------------------------------------------------------ 2. end to end against the oracle
NAMES = ["npt", "two_and_two", "long_message"]
E2E_RATES = [48000, 44100, 32000, 22050, 16000, 11025, 8000]


def _expected_lines(name):
    with open(os.path.join(GOLDEN, f"{name}.22050.s16le.txt")) as f:
        return [ln for ln in f.read().splitlines() if ln != "+OK"]


@pytest.fixture(scope="module")
def sources():
    """21 channels: each golden recording taken to each source rate by the float64 reference, rounded to int16, zero-padded
    to a whole number of half-second calls that covers the longest recording plus 4 s (the reference's flush).  Per channel:
    (name, rate, int16 source, the numpy-f32-resampled stream a 22.05 kHz receiver is to see)."""
    pcm = {n: np.fromfile(os.path.join(GOLDEN, f"{n}.22050.s16le.bin"), dtype="<i2") for n in NAMES}
    n_calls = -(-max(len(v) for v in pcm.values()) * 2 // OUT_RATE) + 8
    chans = []
    for name in NAMES:
        for rate in E2E_RATES:
            src = np.clip(np.rint(rr.resample_f64(pcm[name], OUT_RATE, rate)), -32768, 32767).astype(np.int16)
            total = n_calls * (rate // 2)
            src = np.concatenate([src, np.zeros(total - len(src), np.int16)])
            chans.append((name, rate, src, rr.resample_f32(src, rate, OUT_RATE)))
    return n_calls, chans


def _feed(sa, sources, **flags):
    import torch
    n_calls, chans = sources
    rates = [ch[1] for ch in chans]
    rx = sa.MixedRateReceiver(sa.SameReceiverBuilder(OUT_RATE).samedec(), rates, **flags)
    counts = np.array([r // 2 for r in rates], np.uint32)
    n_rows = int(counts.max())
    fed = np.zeros(len(chans), np.int64)
    for i in range(n_calls):
        x = np.full((n_rows, len(chans)), 32767, np.int16)
        for c, (_, _, src, _) in enumerate(chans):
            x[:counts[c], c] = src[i * counts[c]:(i + 1) * counts[c]]
        fed += rx.process(torch.from_numpy(x).cuda(), counts)
    rx.sync()
    for c, ch in enumerate(chans):
        assert fed[c] == len(ch[3]) == rx.batch.channel_input_sample_counter(c)
    return rx


def _lines(events):
    out = {}
    for e in events:
        m = e.message()
        if m is not None:
            out.setdefault(int(e.channel), []).append(m)
    return out


def test_mixed_rate_batch_equals_the_oracle_event_for_event(sa, ob, sources):
    rx = _feed(sa, sources)
    events = rx.poll_events()
    got = {}
    for e in events:
        got.setdefault(int(e.channel), []).append((int(e.kind), int(e.sample_counter), int(e.len), e.data()))
    lines = _lines(events)
    n_link = 0
    for c, (name, rate, _, y) in enumerate(sources[1]):
        ref = [(int(e.kind), int(e.sample_counter), int(e.len), e.data()) for e in ob.Receiver(ob.samedec_config()).run(y)]
        n_link += sum(1 for t in ref if t[0] <= 3)
        assert got.get(c, []) == ref, f"channel {c}: {name} at {rate} Hz"
        assert lines.get(c, []) == _expected_lines(name), f"channel {c}: {name} at {rate} Hz"
    assert n_link > 10 * len(sources[1])
    # an event's counter maps back to its source: the start of a message lies where the 22.05 kHz recording has it
    assert abs(rx.source_position(0, 22050 + rx.resampler.delay(0)) - 48000.0) < 1e-6


def test_mixed_rate_messages_only_batch_gives_the_same_messages(sa, sources):
    rx = _feed(sa, sources, messages_only=True)
    lines = _lines(rx.poll_events())
    for c, (name, rate, _, _) in enumerate(sources[1]):
        assert lines.get(c, []) == _expected_lines(name), f"channel {c}: {name} at {rate} Hz"


# ------------------------------------------------------------------ 3. refusals
def test_refusals_move_no_counter(sa):
    import torch
    C, n_rows = 70, 100
    rs = sa.Resampler([MIX[c % 7] for c in range(C)], OUT_RATE)
    x = torch.zeros((n_rows, C), dtype=torch.float32, device="cuda")
    counts = np.full(C, n_rows, np.uint32)
    _, rows = rs.out_counts(counts)
    assert rows == 276                                   # ceil(100 * 441 / 160): the 8 kHz channels

    def counters():
        return [(rs.channel_input_counter(c), rs.channel_output_counter(c)) for c in range(C)]

    zero = counters()
    with pytest.raises(sa.SameError) as e:               # out_rows below the largest output count
        rs.process(x, counts, torch.empty((rows - 1, C), dtype=torch.float32, device="cuda"))
    assert e.value.code == -1 and counters() == zero
    bad = counts.copy()
    bad[69] = n_rows + 1
    with pytest.raises(sa.SameError) as e:               # a count above n_rows
        rs.process(x, bad, torch.empty((rows + 8, C), dtype=torch.float32, device="cuda"))
    assert e.value.code == -1 and counters() == zero
    with pytest.raises(sa.SameError) as e:               # a null pointer
        rs.process_device_ptr(0, n_rows, counts, 0, rows)
    assert e.value.code == -1 and counters() == zero
    rs.process(x, np.zeros(C, np.uint32))                # all zero: a no-op
    assert counters() == zero
    with pytest.raises(sa.SameError) as e:               # 17 distinct ratios
        sa.Resampler([8000 + 100 * i for i in range(17)], OUT_RATE)
    assert e.value.code == -1
    sa.Resampler([8000 + 100 * i for i in range(16)], OUT_RATE)
    with pytest.raises(sa.SameError) as e:               # SAME_ERATE
        sa.Resampler([48000, 192000], OUT_RATE)
    assert e.value.code == -9
    sa.Resampler([96000], OUT_RATE)
    with pytest.raises(sa.SameError) as e:               # a reset to a refused rate resets nothing
        rs.reset_channels([1], [192000])
    assert e.value.code == -9
    y, out = rs.process(x, counts)
    torch.cuda.synchronize()
    assert counters() == [(n_rows, int(k)) for k in out] and y.shape[0] == rows

    builder = sa.SameReceiverBuilder(OUT_RATE)
    for flags in ({"time_parallel": True}, {"call_invariant": True}, {"trace_symbols": True}):
        with pytest.raises(sa.SameError) as e:           # the kinds of batch the ragged call refuses, in the batch's own words
            sa.MixedRateReceiver(builder, [48000] * 64, **flags)
        assert e.value.code == -1 and "ragged calls" in str(e.value)
