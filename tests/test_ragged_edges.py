"""Ragged calls past one launch and off the defaults ("What the suite holds").

tests/test_ragged_calls.py holds the ragged entry points to the oracle on the default builders, in calls of one launch and one
transpose slab, on device buffers, with counts drawn over the whole call.  This file holds them to the oracle where the code
takes its other paths:

  A1  every block length of demod_ragged_kernel<B, SampleT> (B = 16, 8, 4, 2, 1; f32 and int16) and the ring shapes of the
      rotated store: DL = 1, 2, 5, 8, 11, 23, 32, 50, rings of 16, 32, 64 and 128 slots, DL above and below the ring, the
      equalizer off and at another size -- ragged and plain calls alternating, so each kernel reads the state the other left;
  A2  short and aligned counts: calls of 1, 2, 3, B, DL and ring rows and their neighbours, a wavefront that consumes nothing, a
      wavefront with one lane at n_rows and 63 at 0, lags that are multiples of DL and of the ring;
  A3  a non-zero row offset on device buffers: a channel-major call of two transpose slabs (strict, and messages-only with
      audio capture), a time-major call of two launches;
  A4  the host calls: small, cut by the upload slab, and cut by the upload slab and the transpose slab at once, against the
      oracle and against a twin batch fed the same calls from device buffers.

Every comparison is exact: per channel the events (kind, sample_counter, symbol_count, data) equal the oracle's over the
channel's own consumed samples, channel_input_sample_counter(c) is the channel's consumed count and input_sample_counter()
the sum of the calls' largest counts.  The streams are made on the CPU (oracle.binding.modulate_afsk bursts, three per message,
per-channel offsets, gaps and amplitudes from 300 to 16 000, seeded noise at a twentieth of the amplitude), and every call's
counts come from a seeded generator, so a case's plan -- its streams and its calls -- needs no GPU: the floor every case
asserts (the oracle alone reports a Burst on at least half the channels it is run on) can be checked with the oracle alone.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN
from test_ragged_calls import Feeder, by_channel, oracle_channel, ragged_counts

pytestmark = pytest.mark.gpu


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


TIME, CHANNEL = 0, 1                    # sameold_amd.LAYOUT_TIME_MAJOR, LAYOUT_CHANNEL_MAJOR (asserted in run())
BURST = 3
PREAMBLE = bytes([0xAB] * 16)
HEADERS = [b"ZCZC-WXR-TOR-039173+0030-1591829-KCLE/NWS-", b"ZCZC-EAS-RWT-012057+0015-0381234-WXYZ/FM -",
           b"ZCZC-CIV-EVI-048201+0100-2000915-KPRC/TV -"]
SLAB = 65520                            # rows of one transpose slab (same_batch.cpp: transpose_in_slabs)


# ------------------------------------------------------------------ streams, plans, the oracle
def make_streams(ob, rate, n_streams, length, seed, period=None):
    """-> ([length, n_streams] f32, per stream the [from, to) of its bursts).  Messages of three bursts; the offset of the first
    (up to 0.3 s, or anywhere in the first period), the gaps between bursts (0.25 to 0.5 s) and between messages (0.3 to 0.8 s,
    or one message every `period` samples), the header and the amplitude (log-uniform over 300 .. 16 000) differ per stream;
    Gaussian noise at amplitude / 20."""
    rng = np.random.default_rng(seed)
    amp = np.exp(rng.uniform(np.log(300.0), np.log(16000.0), n_streams))
    x = rng.standard_normal((length, n_streams), dtype=np.float32) * (amp / 20.0).astype(np.float32)[None, :]
    bursts = [ob.modulate_afsk(PREAMBLE + h, rate) for h in HEADERS]
    spans = []
    for c in range(n_streams):
        b = bursts[c % len(bursts)] * np.float32(amp[c])
        sp = []
        start = int(rng.integers(0, period if period else int(0.3 * rate)))
        while start < length:
            t = start
            for _ in range(3):
                e = min(length, t + len(b))
                if t < length:
                    x[t:e, c] += b[:e - t]
                    sp.append((t, e))
                t += len(b) + int(rng.integers(int(0.25 * rate), int(0.5 * rate)))
            start = max(t, start + period) if period else t + int(rng.integers(int(0.3 * rate), int(0.8 * rate)))
        spans.append(sp)
    return x, spans


class PoolFeeder(Feeder):
    """test_ragged_calls.Feeder over a pool of streams: channel c reads column c % pool at its own position (4 096 channels
    need no 4 096 streams), and a channel-major buffer is filled where it lies"""

    def __init__(self, streams, n_ch, dtype="f32"):
        super().__init__(streams, dtype)
        self.pos = np.zeros(n_ch, np.int64)
        self.col = np.arange(n_ch) % streams.shape[1]

    def buffer(self, counts, n_rows, layout_cm):
        n_ch = len(self.pos)
        fill = 0 if self.x.dtype == np.int16 else np.nan
        buf = np.full((n_ch, n_rows) if layout_cm else (n_rows, n_ch), fill, self.x.dtype)
        assert int((self.pos + counts).max()) <= self.x.shape[0], "the streams are too short for this plan"
        for c in range(n_ch):
            k = int(counts[c])
            own = self.x[self.pos[c]:self.pos[c] + k, self.col[c]]
            if layout_cm:
                buf[c, :k] = own
            else:
                buf[:k, c] = own
        self.pos += counts.astype(np.int64)
        return buf

    def own(self, c):
        return self.x[:self.pos[c], self.col[c]]


class Plan:
    """A case without the GPU: the streams and the calls.  A call is (how, n_rows, counts, layout); how[i] says what batch i
    of the case does with it: "device" / "host" (process_ragged / process_host_ragged), "plain" (process_tensor, counts
    all n_rows), None (nothing)."""

    def __init__(self, rate, setters, streams, n_ch, dtype="f32", spans=None):
        self.rate, self.setters, self.streams, self.n_ch, self.dtype, self.spans = rate, setters, streams, n_ch, dtype, spans
        self.calls = []
        self.pos = np.zeros(n_ch, np.int64)           # where every channel stands after the calls so far

    def add(self, how, n_rows, counts, layout=TIME):
        counts = np.asarray(counts).astype(np.uint32)
        assert counts.shape == (self.n_ch,) and int(counts.max()) <= n_rows
        how = (how,) if isinstance(how, str) else tuple(how)
        assert all(h != "plain" or int(counts.min()) == n_rows for h in how)
        self.calls.append((how, int(n_rows), counts, layout))
        self.pos += counts.astype(np.int64)
        assert int(self.pos.max()) <= self.streams.shape[0], "the streams are too short for this plan"

    def plain(self, n_rows, layout=TIME, n_batches=1):
        self.add(("plain",) * n_batches, n_rows, np.full(self.n_ch, n_rows, np.uint32), layout)

    def total(self):
        return sum(int(k.max()) for _, _, k, _ in self.calls)

    def feeder(self):
        return PoolFeeder(self.streams, self.n_ch, self.dtype)


def oracle_config(ob, rate, setters):
    cfg = ob.default_config(rate)
    for name, *args in setters:
        getattr(ob.lib(), "so_config_" + name)(C.byref(cfg), *args)
    return cfg


def builder(sa, rate, setters):
    b = sa.SameReceiverBuilder(rate)
    for name, *args in setters:
        getattr(b, name)(*args)
    return b


def oracle_many(ob, cfg, xs):
    """oracle_channel over every stream of xs (the oracle's calls release the interpreter lock: a thread per core)"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda x: oracle_channel(ob, cfg, x), xs))


def oracle_floor(ob, plan, channels, cfg=None, tail=None):
    """the oracle's events of `channels` over what the plan gives each, and the floor that keeps a case from passing on
    silence: the oracle alone reports at least one Burst on at least half of them"""
    f = plan.feeder()
    f.pos = plan.pos.copy()
    cfg = cfg if cfg is not None else oracle_config(ob, plan.rate, plan.setters)
    xs = [f.own(c) if tail is None else np.concatenate([f.own(c).astype(np.float32), tail]) for c in channels]
    wants = oracle_many(ob, cfg, xs)
    with_burst = sum(any(t[0] == BURST for t in w) for w in wants)
    assert 2 * with_burst >= len(channels), f"only {with_burst} of {len(channels)} channels carry a burst"
    return wants


def run(sa, plan, rxs, after_call=None):
    """the plan's calls on the batches rxs: every call's buffer is built once and handed to each batch as the call says"""
    import torch
    assert (sa.LAYOUT_TIME_MAJOR, sa.LAYOUT_CHANNEL_MAJOR) == (TIME, CHANNEL)
    feeder = plan.feeder()
    for i, (how, n_rows, counts, layout) in enumerate(plan.calls):
        buf = feeder.buffer(counts, n_rows, layout == CHANNEL)
        dev = None
        for rx, h in zip(rxs, how):
            if h is None:
                continue
            if h == "host":
                rx.process_host_ragged(buf, counts, layout=layout)
                continue
            if dev is None:
                dev = torch.from_numpy(buf).cuda()
            if h == "plain":
                rx.process_tensor(dev, layout=layout)
            else:
                rx.process_ragged(dev, counts, layout=layout)
        if after_call:
            after_call(i)
    assert (feeder.pos == plan.pos).all()
    return feeder


def hold_to_oracle(ob, plan, rx, channels):
    """rx, after the plan's calls, against the oracle on `channels` (and the batch's counters on all)"""
    wants = oracle_floor(ob, plan, channels)
    rx.sync()
    got = by_channel(rx.poll_events())
    assert rx.input_sample_counter() == plan.total()
    for c, want in zip(channels, wants):
        assert got.get(c, []) == want, f"channel {c}"
    for c in range(plan.n_ch):
        assert rx.channel_input_sample_counter(c) == plan.pos[c], f"channel {c}"
    return got


def generic_block_length(sa, b):
    """the block length B of the builder's any-configuration kernel, demod_kernel<B> and demod_ragged_kernel<B>, as a generic
    twin of the batch names it"""
    name = b.build_batch(1, generic_kernel=True).kernel_name()
    assert name.startswith("demod_kernel<B=") and name.endswith(">"), name
    return int(name[len("demod_kernel<B="):-1])


# ------------------------------------------------------------------ A1. every block length, both sample types, the ring shapes
DEV = "with_timing_max_deviation"
DC = "with_dc_blocker_length"
# id: rate, builder setters, B, DL, window ring (sameold_amd/csrc/same_config.cpp: derive_params)
A1_ROWS = {
    "22050-dev0.10": (22050, [(DEV, 0.10)], 8, 16, 64),
    "22050-dev0.30": (22050, [(DEV, 0.30)], 4, 16, 64),
    "22050-dev0.40": (22050, [(DEV, 0.40)], 2, 16, 64),
    "22050-dev0.45": (22050, [(DEV, 0.45)], 1, 16, 64),
    "8000": (8000, [], 4, 5, 32),
    "8000-dev0.20": (8000, [(DEV, 0.20)], 2, 5, 16),
    "8000-dev0.30": (8000, [(DEV, 0.30)], 1, 5, 16),
    "11025": (11025, [], 8, 8, 32),
    "16000": (16000, [], 8, 11, 64),
    "32000": (32000, [], 16, 23, 128),
    "44100-dev0.45": (44100, [(DEV, 0.45)], 2, 32, 128),
    "22050-dc0.03": (22050, [(DC, 0.03)], 16, 1, 64),
    "22050-dc0.05": (22050, [(DC, 0.05)], 16, 2, 64),
    "22050-dc1.2": (22050, [(DC, 1.2)], 16, 50, 64),
    "22050-no-eq": (22050, [("without_adaptive_equalizer",)], 16, 16, 64),
    "22050-eq-8-3": (22050, [("with_adaptive_equalizer", 8, 3, 0.2, 1e-5)], 16, 16, 64),
}
# int16 on one row per block length
A1_I16 = ["32000", "22050-dev0.10", "8000", "8000-dev0.20", "22050-dev0.45"]
A1_CASES = [(r, "f32") for r in A1_ROWS] + [(r, "i16") for r in A1_I16]
A1_SHAPE = ["zero", "half", "zero", "plain", "half", "zero", "half", "plain"]


def plan_a1(ob, rate, setters, seed, dtype, hows=("device",) * 6, layout=TIME):
    """130 channels (three wavefronts, the last one partial); six ragged calls of about 0.6 s, "zero" counts (the whole call
    is the ragged kernel's) and "half" counts (a lockstep prefix, then the ragged kernel) in turn, a plain call in the middle
    and one at the end: each kernel reads the state the other left.  hows: how each of the six ragged calls is made"""
    n_ch, n_rows = 130, int(0.6 * rate) + 7
    streams, spans = make_streams(ob, rate, n_ch, n_rows * len(A1_SHAPE), 100 + seed)
    plan = Plan(rate, setters, streams, n_ch, dtype, spans)
    rng = np.random.default_rng(200 + seed)
    hows = list(hows)
    for low in A1_SHAPE:
        if low == "plain":
            plan.plain(n_rows, layout)
        else:
            plan.add(hows.pop(0), n_rows, ragged_counts(rng, n_ch, n_rows, low), layout)
    return plan


def plan_a1_row(ob, row, dtype):
    rate, setters = A1_ROWS[row][:2]
    return plan_a1(ob, rate, setters, 2 * list(A1_ROWS).index(row) + (dtype == "i16"), dtype)


def test_a1_table_covers_every_block_length_with_both_sample_types():
    for dtype in ("f32", "i16"):
        assert {A1_ROWS[r][2] for r, d in A1_CASES if d == dtype} == {16, 8, 4, 2, 1}
    assert {A1_ROWS[r][3] for r, _ in A1_CASES} >= {1, 2, 5, 8, 11, 16, 23, 32, 50}
    assert {A1_ROWS[r][4] for r, _ in A1_CASES} == {16, 32, 64, 128}
    # 64 KiB of LDS per wavefront: (2 DL + ring) x 64 lanes x 4 bytes
    assert all((2 * dl + ring) * 256 < 65536 for _, _, _, dl, ring in A1_ROWS.values())


@pytest.mark.parametrize("row,dtype", A1_CASES, ids=[f"{r}-{d}" for r, d in A1_CASES])
def test_a1_block_lengths_and_ring_shapes(sa, ob, row, dtype):
    rate, setters, block_len, dc_len, ring = A1_ROWS[row]
    b = builder(sa, rate, setters)
    # a row that silently lands on another block length is a failed test
    assert generic_block_length(sa, b) == block_len
    d = ob.derive(oracle_config(ob, rate, setters))
    assert d.dc_len == dc_len and ring >= d.ntaps + block_len - 1
    plan = plan_a1_row(ob, row, dtype)
    rx = b.build_batch(plan.n_ch)
    names = []
    run(sa, plan, [rx], after_call=lambda i: names.append(rx.kernel_name()))
    for name in names:
        # where the batch's own kernel is the any-configuration one, it names the same block length
        assert not name.startswith("demod_kernel<") or name == f"demod_kernel<B={block_len}>", name
    hold_to_oracle(ob, plan, rx, range(plan.n_ch))


# ------------------------------------------------------------------ A2. short and aligned counts
def plan_a2(ob, rate):
    """192 channels (three whole wavefronts) at the default builder.  Ragged calls of 1, 2, 3, B - 1 .. B + 1, DL - 1 .. DL + 1,
    ring - 1 .. ring + 1, 2 ring + 3, 997 and DL ring + 1 rows in turn; in each, one wavefront consumes nothing (kw = 0: no
    loop iteration, the rotated store by n_rows still runs), one has a single lane at n_rows and 63 at 0, and one has lags
    n_rows - k_c from {0, 1, DL, 2 DL, ring, DL ring} as far as they fit, and random lags; the roles move on one wavefront
    per call.  Every tenth call is a plain one of 3 000 rows.  Calls go on until every channel is 0.2 s past its sixth burst."""
    block_len, dc_len, ring = {22050: (16, 16, 64), 8000: (4, 5, 32)}[rate]
    n_ch = 192
    six = 6 * len(ob.modulate_afsk(PREAMBLE + HEADERS[0], rate)) + int((0.3 + 5 * 0.5 + 0.8 + 0.2) * rate)
    streams, spans = make_streams(ob, rate, n_ch, six + 4 * rate, 300 + rate)
    plan = Plan(rate, [], streams, n_ch, "f32", spans)
    target = np.array([sp[5][1] + int(0.2 * rate) for sp in spans])
    sizes = [1, 2, 3, block_len - 1, block_len, block_len + 1, dc_len - 1, dc_len, dc_len + 1, ring - 1, ring, ring + 1,
             2 * ring + 3, 997, dc_len * ring + 1]
    special = [0, 1, dc_len, 2 * dc_len, ring, dc_len * ring]
    rng = np.random.default_rng(400 + rate)
    i = n_ragged = 0
    seen = {"kc": set(), "lag": set()}
    while (plan.pos < target).any():
        i += 1
        if i % 10 == 0:
            plan.plain(3000)
            continue
        n_rows = sizes[n_ragged % len(sizes)]
        n_ragged += 1
        k = np.zeros(n_ch, np.uint32)
        for w in range(3):
            role = (w + i) % 3
            lanes = np.arange(64 * w, 64 * w + 64)
            if role == 1:
                k[lanes[(5 * i) % 64]] = n_rows
            elif role == 2:
                fit = [s for s in special if s <= n_rows]
                lag = rng.integers(0, n_rows + 1, 64)
                lag[:32] = [fit[(j + i) % len(fit)] for j in range(32)]
                k[lanes] = n_rows - np.roll(lag, i)
                seen["lag"].update(int(v) for v in lag)
        seen["kc"].update(int(v) for v in k)
        plan.add("device", n_rows, k)
    # the counts the issue names occur: k_c in {1, B - 1, B, B + 1}, lags that are multiples of DL and of the ring
    assert seen["kc"] >= {0, 1, block_len - 1, block_len, block_len + 1}
    assert seen["lag"] >= set(special)
    return plan


@pytest.mark.parametrize("rate", [22050, 8000])
def test_a2_short_and_aligned_counts(sa, ob, rate):
    plan = plan_a2(ob, rate)
    b = builder(sa, rate, [])
    if rate == 8000:
        assert generic_block_length(sa, b) == 4
    rx = b.build_batch(plan.n_ch)
    run(sa, plan, [rx])
    got = hold_to_oracle(ob, plan, rx, range(plan.n_ch))
    # two full messages everywhere: six bursts per channel
    assert all(sum(t[0] == BURST for t in got.get(c, [])) >= 6 for c in range(plan.n_ch))


# ------------------------------------------------------------------ A3. past the first slab and the first launch
def slab_counts(rng, n_ch, n_rows, cut, late):
    """counts around a cut of the call (a slab's or a launch's last row): late -- all of them beyond the cut, the cut's
    successor and n_rows among them (the piece before the cut is all common prefix; the piece behind it has a prefix AND a
    row offset); else spread over the call, with 0, 1, cut - 1, cut, cut + 1, n_rows - 1 and n_rows among them, a quarter
    of the channels within 16 rows of the cut and a quarter at or just beyond it"""
    if late:
        k = rng.integers(cut + 1, n_rows + 1, n_ch)
        k[rng.choice(n_ch, 4, replace=False)] = [cut + 1, cut + 1, n_rows, n_rows]
        return k.astype(np.uint32)
    k = rng.integers(0, n_rows + 1, n_ch)
    near = rng.choice(n_ch, n_ch // 2, replace=False)
    k[near[:n_ch // 4]] = cut + rng.integers(-16, 17, n_ch // 4)
    k[near[n_ch // 4:]] = rng.integers(cut, n_rows + 1, len(near) - n_ch // 4)
    named = [0, 0, 1, cut - 1, cut, cut + 1, n_rows - 1, n_rows, n_rows]
    k[rng.choice(n_ch, len(named), replace=False)] = named
    return k.astype(np.uint32)


def plan_a3_slabs(ob, dtype, shape):
    """channel-major calls of 70 560 rows at 22.05 kHz: two transpose slabs, the second one with row offset 65 520"""
    rate, n_ch, n_rows = 22050, 96, 70560
    streams, spans = make_streams(ob, rate, n_ch, 3 * n_rows, 500 + (dtype == "i16"))
    plan = Plan(rate, [], streams, n_ch, dtype, spans)
    rng = np.random.default_rng(510 + (dtype == "i16") + 2 * (shape == "prefix-slab"))
    for i in range(3):
        # "prefix-slab": the middle call's first slab lies wholly inside the prefix (m > 65 520)
        plan.add("device", n_rows, slab_counts(rng, n_ch, n_rows, SLAB, shape == "prefix-slab" and i == 1), CHANNEL)
    return plan


@pytest.mark.parametrize("shape", ["spread", "prefix-slab"])
@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_a3_channel_major_two_slabs(sa, ob, dtype, shape):
    plan = plan_a3_slabs(ob, dtype, shape)
    if shape == "prefix-slab":
        assert int(plan.calls[1][2].min()) > SLAB
    for _, n_rows, k, _ in plan.calls:
        assert n_rows > SLAB and (k > SLAB).any() and (k < n_rows).any()
    assert any({0, SLAB, SLAB + 1, n_rows} <= set(int(v) for v in k) for _, n_rows, k, _ in plan.calls)
    rx = builder(sa, plan.rate, []).build_batch(plan.n_ch)
    run(sa, plan, [rx])
    hold_to_oracle(ob, plan, rx, range(plan.n_ch))


RECORDINGS = ["npt", "long_message", "two_and_two"]


def plan_a3_capture(dtype):
    """the streams of test_messages_only_with_audio_capture (every channel a recording behind its own silence) in
    channel-major calls of two slabs, until every stream is consumed"""
    rate, n_ch, n_rows = 22050, 96, 70560
    pcms = [np.fromfile(f"{GOLDEN}/{n}.22050.s16le.bin", dtype="<i2").astype(np.float32) for n in RECORDINGS]
    rng = np.random.default_rng(520 + (dtype == "i16"))
    L = max(len(p) for p in pcms) + 3 * rate
    streams = np.zeros((L, n_ch), np.float32)
    for c in range(n_ch):
        p = pcms[c % len(pcms)]
        off = int(rng.integers(0, L - len(p)))
        streams[off:off + len(p), c] = p
    plan = Plan(rate, [], streams, n_ch, dtype)
    i = 0
    while plan.pos.min() < L:
        k = slab_counts(rng, n_ch, n_rows, SLAB, i % 3 == 1).astype(np.int64)
        plan.add("device", n_rows, np.minimum(k, L - plan.pos), CHANNEL)
        i += 1
    return plan


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_a3_channel_major_two_slabs_messages_only_with_audio_capture(sa, ob, dtype):
    """transport_ragged_kernel and cap::WalkerT<true> with a non-zero row offset: every channel's messages equal the oracle's
    over its own stream, and each message's joined audio is the channel's own samples over [som, next), bit for bit"""
    from test_audio_capture import expected_captures, join
    plan = plan_a3_capture(dtype)
    rate, n_ch, L = plan.rate, plan.n_ch, plan.streams.shape[0]
    assert sum(int(k.max()) > SLAB and int(k.min()) < int(k.max()) for _, _, k, _ in plan.calls) >= 4
    rx = sa.SameReceiverBuilder(rate).samedec().build_batch(n_ch, messages_only=True)
    rx.set_audio_capture(1 << 24)
    chunks = []
    feeder = run(sa, plan, [rx], after_call=lambda i: chunks.extend(rx.poll_audio()))
    assert (feeder.pos == L).all()
    rx.flush()
    rx.sync()
    chunks += rx.poll_audio()
    assert rx.transport_on_device() == 1
    got = by_channel(rx.poll_events())
    cfg = ob.samedec_config(rate)
    zeros = np.zeros(4 * rate, np.float32)
    wants = oracle_many(ob, cfg, [np.concatenate([feeder.own(c).astype(np.float32), zeros]) for c in range(n_ch)])
    assert 2 * sum(any(t[0] == BURST for t in w) for w in wants) >= n_ch
    want_msgs, n_msgs = {}, 0
    for c in range(n_ch):
        want = [t for t in wants[c] if t[0] in (18, 19)]
        assert got.get(c, []) == want, f"channel {c}"
        want_msgs[c] = [(t[0], t[1]) for t in want]
        n_msgs += len(want)
    assert n_msgs >= n_ch
    caps, samples, _ = join(sa, chunks)
    assert caps == expected_captures(want_msgs, flush_at=L)
    for c, a, b, _ in caps:
        assert np.array_equal(samples[(c, a)].view(np.int32), feeder.x[a:b, c].astype(np.float32).view(np.int32)), (c, a, b)


LAUNCH_8K = 360000                      # rows of one launch at 8 kHz (same_batch.cpp: kMaxChunk = min(2^22, 45 s x rate))


def plan_a3_launches(ob, shape):
    """one time-major call of 364 000 rows at 8 kHz -- two launches, the second one with row offset 360 000 -- behind two
    ordinary ragged calls and in front of a plain one; a message every 12 s, so both launches carry bursts"""
    rate, n_ch, n_rows, small = 8000, 64, 364000, 4807
    streams, spans = make_streams(ob, rate, n_ch, n_rows + 3 * small, 530, period=12 * rate)
    plan = Plan(rate, [], streams, n_ch, "f32", spans)
    rng = np.random.default_rng(540 + (shape == "prefix-launch"))
    plan.add("device", small, ragged_counts(rng, n_ch, small, "zero"))
    plan.add("device", small, ragged_counts(rng, n_ch, small, "half"))
    if shape == "prefix-launch":
        # m = 361 000: the first launch is pure prefix, the second has a prefix and a row offset
        k = rng.integers(361000, n_rows + 1, n_ch)
        k[rng.choice(n_ch, 4, replace=False)] = [361000, 361000, n_rows, n_rows]
    else:
        # m = 0: both launches are ragged throughout
        k = slab_counts(rng, n_ch, n_rows, LAUNCH_8K, False)
    plan.add("device", n_rows, k)
    plan.plain(small)
    return plan


@pytest.mark.parametrize("shape", ["ragged-throughout", "prefix-launch"])
def test_a3_time_major_two_launches(sa, ob, shape):
    plan = plan_a3_launches(ob, shape)
    (_, _, k0, _), (_, _, k1, _), (_, n_rows, k, _), _ = plan.calls
    assert n_rows > LAUNCH_8K and int(k.min()) == (0 if shape == "ragged-throughout" else 361000)
    if shape == "ragged-throughout":
        assert {0, LAUNCH_8K - 1, LAUNCH_8K, LAUNCH_8K + 1, n_rows} <= set(int(v) for v in k)
        assert (k < LAUNCH_8K - 16).sum() >= 8 and (k > LAUNCH_8K + 16).sum() >= 8
    # a burst straddles the launches' boundary on a channel that reads past it
    at = k0.astype(np.int64) + k1 + LAUNCH_8K
    assert any(k[c] > LAUNCH_8K and any(a < at[c] < b for a, b in plan.spans[c]) for c in range(plan.n_ch))
    rx = builder(sa, plan.rate, []).build_batch(plan.n_ch)
    run(sa, plan, [rx])
    hold_to_oracle(ob, plan, rx, range(plan.n_ch))


# ------------------------------------------------------------------ A4. the host calls
@pytest.mark.parametrize("layout", [TIME, CHANNEL], ids=["time", "channel"])
@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_a4_host_calls_small(sa, ob, dtype, layout):
    """A1's calls on the default builder through process_host_ragged, every other ragged call through process_ragged on the
    same batch: the host call collects the launches in flight before it reuses the upload buffer"""
    plan = plan_a1(ob, 22050, [], 50 + 2 * layout + (dtype == "i16"), dtype, ["host", "device", "host", "host", "device", "host"], layout)
    rx = builder(sa, plan.rate, []).build_batch(plan.n_ch)
    run(sa, plan, [rx])
    hold_to_oracle(ob, plan, rx, range(plan.n_ch))


def plan_a4_upload_slab(ob):
    """4 096 channels, three time-major host calls of 20 000 rows: the upload slab (256 MiB) is 16 384 rows"""
    rate, n_ch, n_rows, cut = 22050, 4096, 20000, 16384
    assert (256 << 20) // (n_ch * 4) == cut
    streams, spans = make_streams(ob, rate, 128, 3 * n_rows, 550)
    plan = Plan(rate, [], streams, n_ch, "f32", spans)
    rng = np.random.default_rng(551)
    for i in range(3):
        plan.add(("host", "device"), n_rows, slab_counts(rng, n_ch, n_rows, cut, i == 1))
    return plan


def plan_a4_nested(ob):
    """512 channels, two channel-major host calls of 140 000 rows: the upload slab is 131 072 rows, and the transpose slabs
    inside it begin at rows 0, 65 520 and 131 040"""
    rate, n_ch, n_rows, cut = 22050, 512, 140000, 131072
    assert (256 << 20) // (n_ch * 4) == cut
    streams, spans = make_streams(ob, rate, 128, 2 * n_rows, 560)
    plan = Plan(rate, [], streams, n_ch, "f32", spans)
    rng = np.random.default_rng(561)
    k = slab_counts(rng, n_ch, n_rows, cut, False)
    named = [SLAB - 1, SLAB, SLAB + 1, 2 * SLAB - 1, 2 * SLAB, 2 * SLAB + 1, cut - 1, cut, cut + 1]
    k[rng.choice(n_ch, len(named), replace=False)] = named
    plan.add(("host", "device"), n_rows, k, CHANNEL)
    plan.add(("host", "device"), n_rows, slab_counts(rng, n_ch, n_rows, cut, True), CHANNEL)
    return plan


@pytest.mark.parametrize("case,step", [("upload-slab", 7), ("nested", 4)])
def test_a4_host_calls_cut_by_the_upload_slab(sa, ob, case, step):
    """against the oracle on every step-th channel, and on every channel against a twin batch fed the same calls through
    process_ragged on device buffers"""
    plan = plan_a4_upload_slab(ob) if case == "upload-slab" else plan_a4_nested(ob)
    host = builder(sa, plan.rate, []).build_batch(plan.n_ch)
    twin = builder(sa, plan.rate, []).build_batch(plan.n_ch)
    run(sa, plan, [host, twin])
    got = hold_to_oracle(ob, plan, host, range(0, plan.n_ch, step))
    twin.sync()
    assert got == by_channel(twin.poll_events())
    assert twin.input_sample_counter() == host.input_sample_counter()
    assert all(twin.channel_input_sample_counter(c) == plan.pos[c] for c in range(plan.n_ch))
