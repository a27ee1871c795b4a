"""The tone detector on the device (include/same_tones.h, sameold_amd/csrc/same_tones.hip) against the numpy restatement of its
contract (tests/helpers/tones_reference.py): block values bit for bit, events and counters, through ragged and plain calls,
f32 and int16, both layouts and a mix of all of them on one handle; beside a strict batch on the same tensors and stream; and
the refusals."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
TIME_MAJOR, CHANNEL_MAJOR = 0, 1


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


def _device_input(x_rows, counts, dtype, layout):
    """x_rows: [n_rows, C] integer-valued float64 with the channels' samples in their first counts[c] rows.  NaN (f32) or
    32767 (int16) stands behind every channel's count.  Returns the CUDA tensor in `layout`."""
    import torch
    n_rows, C = x_rows.shape
    x = np.array(x_rows, dtype=dtype, order="C")
    for c in range(C):
        x[counts[c]:, c] = np.nan if dtype == np.float32 else 32767
    if layout == CHANNEL_MAJOR:
        x = np.ascontiguousarray(x.T)
    return torch.from_numpy(x).cuda()


def _by_channel(events, C):
    out = [[] for _ in range(C)]
    for e in events:
        out[int(e["channel"])].append(tuple(int(e[k]) for k in ("channel", "kind", "edge", "reserved", "sample_counter", "duration")))
    return out


# ------------------------------------------------------------------ 1. the kernels against the f32 reference, bit for bit
RATE1, C1, ROWS1, CALLS1 = 8000, 130, 3500, 4
N1 = RATE1 // 25
RESET1 = 60                                   # a 1050 Hz channel that takes every call whole: active from block 25 on


@pytest.fixture(scope="module")
def ragged_case():
    """130 integer-valued streams of 14 000 samples (so that f32 and int16 hold the same values), the counts of four ragged
    calls, and the reference's blocks of every whole stream.  Channel RESET1's reference is cut where it is reset."""
    rng = np.random.default_rng(21)
    length = ROWS1 * CALLS1
    A = 8000.0
    x = np.zeros((C1, length))
    for c in range(C1):
        kind = c % 5
        if kind == 0:
            x[c] = A * tr.tone(tr.WAT, length, RATE1, 1.0, 0.1 * c)
        elif kind == 1:
            x[c, 2 * N1:34 * N1] = A * tr.tone(tr.ATTENTION, 32 * N1, RATE1, 1.0, 0.1 * c)
        elif kind == 2:
            x[c] = 3000.0 * rng.standard_normal(length)
        elif kind == 3:
            x[c] = A * tr.tone(tr.WAT, length, RATE1 * 1.003, 1.0) + A * np.sqrt(0.05) * rng.standard_normal(length)
        else:
            x[c] = A * tr.tone(tr.ATTENTION, length, RATE1, 1.0, 0.1 * c) + 500.0
    x = np.round(x)
    counts = []
    for i in range(CALLS1):
        k = rng.integers(0, ROWS1 + 1, C1).astype(np.uint32)
        k[::4] = ROWS1                                       # every fourth channel takes every call whole: tones get to START
        k[[3 + i, 70 + i, 129]] = 0
        k[[10 + i, 80 + i, 128]] = 1
        k[[20 + i, 90 + i]] = 10
        k[[33 + i, 100 + i]] = N1 - 1
        k[[44 + i, 110 + i]] = N1 + 1
        k[[32, 120, RESET1]] = ROWS1
        counts.append(k)
    whole, whole_E = tr.blocks_f32(x.astype(np.float32), RATE1, True)       # [C, 43, 4], [C, 43]
    reset_at = 3 * ROWS1                                     # RESET1 is reset between calls 2 and 3, counted from 0
    after, after_E = tr.blocks_f32(x[RESET1, reset_at:].astype(np.float32), RATE1, True)
    return x, counts, (whole, whole_E), reset_at, (after, after_E)


VARIANTS = {
    "f32-time": [(np.float32, TIME_MAJOR)] * 4,
    "f32-channel": [(np.float32, CHANNEL_MAJOR)] * 4,
    "i16-time": [(np.int16, TIME_MAJOR)] * 4,
    "i16-channel": [(np.int16, CHANNEL_MAJOR)] * 4,
    "mixed": [(np.float32, CHANNEL_MAJOR), (np.int16, TIME_MAJOR), (np.int16, CHANNEL_MAJOR), (np.float32, TIME_MAJOR)],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernels_equal_the_reference_bit_for_bit(sa, ragged_case, variant):
    import torch
    x, counts, (whole, whole_E), reset_at, (after, after_E) = ragged_case
    td = sa.ToneDetector(C1, RATE1)
    assert td.block_length == N1 and np.array_equal(td.coefficients().view(np.uint32), tr.coefficients(RATE1).view(np.uint32))
    done = np.zeros(C1, np.int64)
    got = [[] for _ in range(C1)]
    events = []
    for i, (dtype, layout) in enumerate(VARIANTS[variant]):
        if i == 3:
            assert any(e["channel"] == RESET1 and e["edge"] == sa.TONE_START for e in events)      # its tone is active
            td.reset_channels([RESET1])
            assert td.channel_sample_counter(RESET1) == 0
        k = counts[i]
        rows = np.zeros((ROWS1, C1))
        for c in range(C1):
            rows[:k[c], c] = x[c, done[c]:done[c] + k[c]]
        want, most = td.block_counts(ROWS1, k)
        pos = done.copy()
        if i == 3:
            pos[RESET1] = 0
        assert np.array_equal(want, (pos % N1 + k) // N1) and most == want.max()
        blocks = torch.full((most + 2, C1, 4), SENTINEL, dtype=torch.float32, device="cuda")
        made = td.process(_device_input(rows, k, dtype, layout), k, layout, blocks)
        td.sync()
        assert np.array_equal(made, want)
        b = blocks.cpu().numpy()
        for c in range(C1):
            got[c].append(b[:want[c], c])
            assert np.all(b[want[c]:, c] == np.float32(SENTINEL)), f"call {i} channel {c}: a row behind its blocks was written"
        ev = td.poll()
        assert np.array_equal(ev["channel"], np.sort(ev["channel"], kind="stable"))                 # inside a call: by channel
        events += list(ev)
        done += k
    per_channel = _by_channel(events, C1)
    n_started = 0
    for c in range(C1):
        mine = np.concatenate(got[c])
        ch = tr.Channel(c, N1)
        if c == RESET1:
            ref = np.concatenate([whole[c, :reset_at // N1], after])
            ref_ev = ch.feed(*tr.qualify_f32(ref[:reset_at // N1], RATE1, whole_E[c, :reset_at // N1]))
            ch.reset()
            ref_ev += ch.feed(*tr.qualify_f32(after, RATE1, after_E))
            assert td.channel_sample_counter(c) == done[c] - reset_at
            assert [(e[1], e[2]) for e in ref_ev] == [(tr.WAT, tr.START)]                           # no END behind the reset
        else:
            ref = whole[c, :done[c] // N1]
            ref_ev = ch.feed(*tr.qualify_f32(ref, RATE1, whole_E[c, :done[c] // N1]))
            assert td.channel_sample_counter(c) == done[c]
        assert mine.shape == ref.shape
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), f"{variant}: channel {c}"
        assert per_channel[c] == ref_ev, f"{variant}: channel {c}"
        n_started += len(ref_ev) > 0
    assert n_started >= 15                                   # (the case has tones that start, and one that ends)
    assert any(e[2] == tr.END for ev in per_channel for e in ev)


# ------------------------------------------------------------------ 2. plain calls
@pytest.mark.parametrize("rate", [22050, 48000])
def test_plain_calls_equal_the_reference_and_the_ragged_call(sa, rate):
    import torch
    C, N = 64, rate // 25
    rows = 5 * N // 2                                        # two calls of 2.5 blocks
    rng = np.random.default_rng(rate)
    x = np.round(2000.0 * rng.standard_normal((C, 2 * rows)) + 6000.0 * tr.tone(tr.WAT, 2 * rows, rate, 1.0)[None, :] * (np.arange(C) % 3 == 0)[:, None])
    ref = tr.blocks_f32(x.astype(np.float32), rate)
    plain, ragged = sa.ToneDetector(C, rate), sa.ToneDetector(C, rate)
    got = {"plain": [], "ragged": []}
    for i in range(2):
        part = x[:, i * rows:(i + 1) * rows].T
        everything = np.full(C, rows, np.uint32)
        n_blocks = (i * rows % N + rows) // N
        for name, td, counts, dtype, layout in (("plain", plain, None, np.float32, TIME_MAJOR),
                                                ("ragged", ragged, everything, np.int16, CHANNEL_MAJOR)):
            blocks = torch.full((n_blocks + 1, C, 4), SENTINEL, dtype=torch.float32, device="cuda")
            made = td.process(_device_input(part, everything, dtype, layout), counts, layout, blocks)
            td.sync()
            assert np.all(made == n_blocks)
            b = blocks.cpu().numpy()
            assert np.all(b[n_blocks:] == np.float32(SENTINEL))
            got[name].append(b[:n_blocks])
    for name, td in (("plain", plain), ("ragged", ragged)):
        mine = np.concatenate(got[name]).transpose(1, 0, 2)
        assert mine.shape == ref.shape == (C, 5, 4)
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), name
        assert all(td.channel_sample_counter(c) == 2 * rows for c in range(C)) and len(td.poll()) == 0


# ------------------------------------------------------------------ 3. beside a batch
def test_beside_a_strict_batch(sa, ob):
    """16 channels of generated messages, fed in 1-s calls to a strict batch and to a ToneDetector from the same tensors on the
    same stream.  The batch's events are those of a batch run without the detector; the tone events are the reference's.

    Where a tone START lies among the batch's events: the reference's assembler emits TRANSPORT_MSG_START when its 1.31-s
    burst timeout runs out behind the third header burst (its sample counter is that moment: 133 624 on a clean channel, 1.41 s
    behind the burst that ends at 102 564), while the generator's tone begins 1 s behind that burst (124 614) and START's
    sample_counter is the tone's first block (124 362).  So a START's sample_counter lies behind the last header burst and
    ahead of TRANSPORT_MSG_END, and the sample at which START was confirmed (25 blocks later) lies between TRANSPORT_MSG_START
    and TRANSPORT_MSG_END: both are asserted, with the figures printed."""
    import torch
    rate, C = 22050, 16
    N = rate // 25
    streams, tone_at = [], []
    for c in range(C):
        noisy = c % 4 == 3
        x, at, _ = tr.message(rate, tr.ATTENTION if c < 8 else tr.WAT, 100 + c, 10.0 if noisy else None, 1.003 if noisy else 1.0,
                              modulate=ob.modulate_afsk)
        streams.append(x)
        tone_at.append(at)
    assert len({len(s) for s in streams}) == 1 and len(set(tone_at)) == 1
    x = np.stack(streams, axis=1)                            # [T, C] float32
    n_calls = -(-x.shape[0] // rate)
    tensors = [torch.from_numpy(np.ascontiguousarray(x[i * rate:(i + 1) * rate])).cuda() for i in range(n_calls)]
    torch.cuda.synchronize()

    def batch_events(with_detector):
        rx = sa.SameReceiverBuilder(rate).samedec().build_batch(C)
        td = sa.ToneDetector(C, rate) if with_detector else None
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for t in tensors:
                rx.process_tensor(t, stream=st.cuda_stream)
                if td is not None:
                    td.process(t, stream=st.cuda_stream)
        rx.sync()
        got = {}
        for e in rx.poll_events():
            got.setdefault(e.channel, []).append(e.as_tuple())
        if td is None:
            return got, None
        td.sync()
        assert all(td.channel_sample_counter(c) == x.shape[0] for c in range(C))
        return got, _by_channel(td.poll(), C)

    alone, _ = batch_events(False)
    beside, tones = batch_events(True)
    assert beside == alone                                   # nothing of the batch's behaviour moved
    for c in range(C):
        ref = tr.events_of_stream(x[:, c], rate, c)
        kind = tr.ATTENTION if c < 8 else tr.WAT
        assert [(e[1], e[2]) for e in ref] == [(kind, tr.START), (kind, tr.END)]
        assert tones[c] == ref, f"channel {c}"
        msg_start = [t[1] for t in beside[c] if t[0] == sa.TRANSPORT_MSG_START]
        msg_end = [t[1] for t in beside[c] if t[0] == sa.TRANSPORT_MSG_END]
        assert len(msg_start) == 1 and len(msg_end) == 1, f"channel {c}: {beside[c]}"
        start = ref[0][4]
        print(f"channel {c}: MSG_START {msg_start[0]}, tone START {start} (confirmed {start + 25 * N}), MSG_END {msg_end[0]}")
        assert tone_at[c] - rate <= start <= msg_end[0]      # behind the third header burst (it ends 1 s before the tone)
        assert abs(start - tone_at[c]) <= N
        assert msg_start[0] <= start + 25 * N <= msg_end[0]


# ------------------------------------------------------------------ 4. refusals
def test_refusals_move_no_counter(sa):
    import torch
    C, n_rows, rate = 70, 1000, 8000
    td = sa.ToneDetector(C, rate)
    x = torch.zeros((n_rows, C), dtype=torch.float32, device="cuda")
    counts = np.full(C, n_rows, np.uint32)
    _, most = td.block_counts(n_rows, counts)
    assert most == 3

    def counters():
        return [td.channel_sample_counter(c) for c in range(C)]

    zero = counters()
    assert zero == [0] * C
    bad = counts.copy()
    bad[69] = n_rows + 1
    with pytest.raises(sa.SameError) as e:                   # a count above n_rows
        td.process(x, bad)
    assert e.value.code == -1 and counters() == zero
    with pytest.raises(sa.SameError) as e:                   # block_rows below the largest block count
        td.process(x, counts, blocks=torch.empty((most - 1, C, 4), dtype=torch.float32, device="cuda"))
    assert e.value.code == -1 and counters() == zero
    with pytest.raises(sa.SameError) as e:                   # a layout that is neither
        td.process_device_ptr(x.data_ptr(), n_rows, counts, layout=2)
    assert e.value.code == -1 and counters() == zero
    with pytest.raises(sa.SameError) as e:                   # a null pointer with samples to read
        td.process_device_ptr(0, n_rows, counts)
    assert e.value.code == -1 and counters() == zero
    td.process(x, np.zeros(C, np.uint32))                    # nothing to read: a no-op
    assert counters() == zero
    td.process(x, counts)
    td.sync()
    assert counters() == [n_rows] * C
    with pytest.raises(sa.SameError) as e:                   # a channel out of range: nothing is reset
        td.reset_channels([0, C])
    assert e.value.code == -1 and counters() == [n_rows] * C
    td.reset_channels([0, C - 1])
    assert counters() == [0] + [n_rows] * (C - 2) + [0]
    for rate in (7999, 96001):
        with pytest.raises(sa.SameError) as e:               # SAME_ERATE
            sa.ToneDetector(C, rate)
        assert e.value.code == -9
    assert len(td.poll()) == 0
