"""Ragged calls (same_batch_process_*_ragged / SameBatchReceiver.process_ragged) on the GPU.

Each channel of a batch is fed its own number of samples per call.  Strict mode against the oracle, bit for bit: every
channel's events equal an oracle receiver run over that channel's own concatenated samples, with its own sample numbering.
Counts that all equal n_rows make exactly the plain call.  The relaxed mode against ragged strict mode under the relaxed
contract; the forced end of message of a lagging channel at the oracle's sample; resets and flush between ragged calls;
the refusals; the input lifetime."""
import numpy as np
import pytest

from conftest import GOLDEN
from test_time_parallel import assert_contract

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


def tuples(evs):
    return [(int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()) for e in evs]


def by_channel(evs):
    out = {}
    for e in evs:
        out.setdefault(int(e.channel), []).append((int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()))
    return out


def ragged_counts(rng, n_ch, n_rows, low="zero"):
    """random counts in [0, n_rows] with 0 and n_rows among them ("zero": the whole call is the ragged remainder), or in
    [n_rows / 2, n_rows] ("half": a lockstep prefix of at least half the call, then the remainder in the same launch)"""
    if low == "half":
        k = rng.integers(n_rows // 2, n_rows + 1, n_ch).astype(np.uint32)
        k[rng.choice(n_ch, 3, replace=False)] = n_rows
        return k
    k = rng.integers(0, n_rows + 1, n_ch).astype(np.uint32)
    k[rng.choice(n_ch, 3, replace=False)] = 0
    k[rng.choice(n_ch, 3, replace=False)] = n_rows
    return k


class Feeder:
    """Per-channel streams [T, C] (host f32), handed out in ragged calls: channel c's next counts[c] samples."""

    def __init__(self, streams, dtype="f32"):
        self.x = np.clip(np.rint(streams), -32768, 32767).astype(np.int16) if dtype == "i16" else streams
        self.pos = np.zeros(streams.shape[1], np.int64)

    def buffer(self, counts, n_rows, layout_cm):
        C = self.x.shape[1]
        fill = 0 if self.x.dtype == np.int16 else np.nan
        buf = np.full((n_rows, C), fill, self.x.dtype)
        for c in range(C):
            k = int(counts[c])
            buf[:k, c] = self.x[self.pos[c]:self.pos[c] + k, c]
        self.pos += counts.astype(np.int64)
        return np.ascontiguousarray(buf.T if layout_cm else buf)


def ragged_feed(sa, rx, feeder, rng, n_calls, n_rows, layout, between=None, low="zero"):
    import torch
    total = 0
    for i in range(n_calls):
        k = ragged_counts(rng, rx.n_channels, n_rows, low)
        buf = feeder.buffer(k, n_rows, layout == sa.LAYOUT_CHANNEL_MAJOR)
        rx.process_ragged(torch.from_numpy(buf).cuda(), k, layout=layout)
        total += int(k.max())
        if between:
            between(i)
    return total


def oracle_channel(ob, cfg, x):
    return tuples(ob.Receiver(cfg).run(np.ascontiguousarray(x)))


# ------------------------------------------------------------------ 1. strict against the oracle
@pytest.mark.parametrize("low", ["zero", "half"])
@pytest.mark.parametrize("rate", [22050, 48000])
@pytest.mark.parametrize("layout_name,dtype", [("time", "f32"), ("time", "i16"), ("channel", "f32"), ("channel", "i16")])
def test_ragged_strict_equals_the_oracle(sa, ob, rate, layout_name, dtype, low):
    n_ch, n_rows, n_calls = 200, int(rate * 1.3), 5
    layout = sa.LAYOUT_TIME_MAJOR if layout_name == "time" else sa.LAYOUT_CHANNEL_MAJOR
    streams = sa.synth_afsk(n_ch, n_rows * n_calls, rate, seed=21, noise_sigma=0.05).cpu().numpy()
    feeder = Feeder(streams, dtype)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rng = np.random.default_rng(rate + (7 if dtype == "i16" else 0) + (3 if layout_name == "channel" else 0))
    total = ragged_feed(sa, rx, feeder, rng, n_calls, n_rows, layout, low=low)
    if low == "half":
        assert not rx.kernel_name().startswith("demod_kernel<"), rx.kernel_name()   # the prefix ran through a lockstep kernel
    rx.sync()
    got = by_channel(rx.poll_events())
    assert rx.input_sample_counter() == total
    cfg = ob.default_config(rate)
    n_events = 0
    for c in range(n_ch):
        own = feeder.x[:feeder.pos[c], c]
        want = oracle_channel(ob, cfg, own)
        n_events += len(want)
        assert got.get(c, []) == want, f"channel {c}"
        assert rx.channel_input_sample_counter(c) == feeder.pos[c]
    assert n_events > 5 * n_ch


@pytest.mark.parametrize("low,layout_name,dtype", [("zero", "time", "f32"), ("half", "time", "f32"), ("half", "channel", "i16")])
def test_ragged_strict_4096_channels(sa, ob, low, layout_name, dtype):
    rate, n_ch, n_rows, n_calls = 22050, 4096, 22050, 3
    layout = sa.LAYOUT_TIME_MAJOR if layout_name == "time" else sa.LAYOUT_CHANNEL_MAJOR
    streams = sa.synth_afsk(n_ch, n_rows * n_calls, rate, seed=5, noise_sigma=0.05).cpu().numpy()
    feeder = Feeder(streams, dtype)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rng = np.random.default_rng(9)
    total = ragged_feed(sa, rx, feeder, rng, n_calls, n_rows, layout, low=low)
    rx.sync()
    got = by_channel(rx.poll_events())
    assert rx.input_sample_counter() == total
    cfg = ob.default_config(rate)
    for c in range(0, n_ch, 7):
        assert got.get(c, []) == oracle_channel(ob, cfg, feeder.x[:feeder.pos[c], c]), f"channel {c}"
        assert rx.channel_input_sample_counter(c) == feeder.pos[c]


# ------------------------------------------------------------------ 2. degenerate ragged equals plain
@pytest.mark.parametrize("mode", ["strict", "relaxed", "link_only", "messages_only"])
def test_full_counts_equal_the_plain_call(sa, mode):
    import torch
    rate, n_ch, n_rows = 22050, 256, 44100
    kw = {"strict": {}, "relaxed": {"relaxed": True}, "link_only": {"link_only": True}, "messages_only": {"messages_only": True}}[mode]
    a = sa.SameReceiverBuilder(rate).build_batch(n_ch, **kw)
    b = sa.SameReceiverBuilder(rate).build_batch(n_ch, **kw)
    if mode == "messages_only":
        a.set_audio_capture(1 << 22); b.set_audio_capture(1 << 22)
    x = sa.synth_afsk(n_ch, n_rows * 3, rate, seed=4, noise_sigma=0.05)
    k = np.full(n_ch, n_rows, np.uint32)
    for i in range(3):
        piece = x[i * n_rows:(i + 1) * n_rows].contiguous()
        a.process_tensor(piece)
        b.process_ragged(piece, k)
    a.sync(); b.sync()
    assert a.kernel_name() == b.kernel_name()
    assert a.transport_on_device() == b.transport_on_device()
    assert tuples(a.poll_events()) == tuples(b.poll_events())
    if mode == "messages_only":
        ca, cb = a.poll_audio(), b.poll_audio()
        assert [t[:3] for t in ca] == [t[:3] for t in cb]
        assert all(np.array_equal(x[3], y[3]) for x, y in zip(ca, cb))
    assert a.input_sample_counter() == b.input_sample_counter() == 3 * n_rows
    assert all(a.channel_input_sample_counter(c) == b.channel_input_sample_counter(c) for c in range(n_ch))


def test_equal_counts_below_n_rows_are_a_shorter_plain_call(sa, ob):
    import torch
    rate, n_ch, n_rows = 22050, 64, 30000
    x = sa.synth_afsk(n_ch, 2 * n_rows, rate, seed=6).cpu().numpy()
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    k = np.full(n_ch, 20000, np.uint32)
    buf = np.full((n_rows, n_ch), np.nan, np.float32)
    buf[:20000] = x[:20000]
    rx.process_ragged(torch.from_numpy(buf).cuda(), k)
    rx.sync()
    assert rx.input_sample_counter() == 20000
    got = by_channel(rx.poll_events())
    cfg = ob.default_config(rate)
    for c in range(n_ch):
        assert got.get(c, []) == oracle_channel(ob, cfg, x[:20000, c])


# ------------------------------------------------------------------ 3. relaxed
@pytest.mark.parametrize("rate", [22050, 48000])
def test_ragged_relaxed_meets_the_relaxed_contract(sa, rate):
    import torch
    n_ch, n_rows, n_calls = 1024, int(rate * 1.5), 4
    streams = sa.synth_afsk(n_ch, n_rows * n_calls, rate, seed=33).cpu().numpy()
    strict = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rel = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=True)
    fs, fr = Feeder(streams), Feeder(streams)
    rng = np.random.default_rng(rate)
    for i in range(n_calls):
        # a spread of a tenth of the call: the prefix runs through the symbol-paced kernel, the rest through the ragged one
        k = rng.integers(n_rows - n_rows // 10, n_rows + 1, n_ch).astype(np.uint32)
        strict.process_ragged(torch.from_numpy(fs.buffer(k, n_rows, False)).cuda(), k)
        rel.process_ragged(torch.from_numpy(fr.buffer(k, n_rows, False)).cuda(), k)
        assert rel.kernel_name() == "demod_sym_kernel", rel.kernel_name()
    # every channel's last samples (a ragged call too): all streams end at the same own position t_end, where the contract's
    # trimming of the bursts cut by the end of the input applies to every channel alike
    t_end = streams.shape[0]
    k = (t_end - fs.pos).astype(np.uint32)
    last = int(k.max())
    strict.process_ragged(torch.from_numpy(fs.buffer(k, last, False)).cuda(), k)
    rel.process_ragged(torch.from_numpy(fr.buffer(k, last, False)).cuda(), k)
    assert (fs.pos == t_end).all()
    # (the flush's zeros end every burst in both modes)
    strict.flush(); rel.flush()
    strict.sync(); rel.sync()

    def ordered(rx):
        ev = rx.poll_events_np()
        return ev[np.lexsort((np.arange(len(ev)), ev["channel"]))]

    got, ref = ordered(rel), ordered(strict)
    assert len(ref[ref["kind"] == 3]) >= n_ch * 2
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(33, c), exact_bursts=True, what="ragged relaxed",
                    t_end=t_end)
    assert all(rel.channel_input_sample_counter(c) == fr.pos[c] + 4 * rate for c in range(n_ch))


# ------------------------------------------------------------------ 5. forced end of message while lagging
@pytest.mark.parametrize("messages_only", [False, True])
def test_forced_end_of_message_while_lagging(sa, ob, messages_only):
    import torch
    rate, n_ch = 22050, 4
    burst = ob.modulate_afsk(bytes([0xAB] * 16) + b"ZCZC-WXR-TOR-039173+0030-1591829-KCLE/NWS-", rate) * np.float32(16384.0)
    gap = np.zeros(rate, np.float32)
    one = np.concatenate([burst, gap, burst, gap, burst, np.zeros(2 * rate, np.float32), np.zeros(rate * 140, np.float32)])
    streams = np.repeat(one[:, None], n_ch, axis=1).astype(np.float32)
    want = tuples(ob.Receiver(ob.default_config(rate)).run(one))
    msgs = [t for t in want if t[0] in (18, 19)]
    assert [t[0] for t in msgs] == [18, 19]
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, messages_only=messages_only)
    feeder = Feeder(streams)
    n_rows = rate * 5
    rng = np.random.default_rng(2)
    # every channel lags by a different amount: channel c consumes a share (1 - c / 8) of most calls
    while feeder.pos.min() < len(one):
        left = len(one) - feeder.pos
        share = np.array([1.0 - c / 8.0 for c in range(n_ch)]) * rng.uniform(0.6, 1.0, n_ch)
        k = np.minimum(left, np.maximum(1, (n_rows * share).astype(np.int64))).astype(np.uint32)
        k[left == 0] = 0
        rx.process_ragged(torch.from_numpy(feeder.buffer(k, n_rows, False)).cuda(), k)
    rx.sync()
    assert rx.transport_on_device() == (1 if messages_only else 0)
    got = by_channel(rx.poll_events())
    for c in range(n_ch):
        assert rx.channel_input_sample_counter(c) == len(one)
        g = got.get(c, [])
        assert [t for t in g if t[0] in (18, 19)] == msgs, f"channel {c}"
        if not messages_only:
            assert g == want, f"channel {c}"


# ------------------------------------------------------------------ 4. messages-only with audio capture
RECORDINGS = ["npt", "long_message", "two_and_two"]


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_messages_only_with_audio_capture(sa, ob, dtype):
    """every channel a recording behind its own silence, fed in ragged calls: its messages equal the oracle's over its own
    stream, and each message's joined audio is the channel's own samples over [som, next), exactly"""
    import torch
    from test_audio_capture import expected_captures, join
    rate, n_ch = 22050, 96
    pcms = [np.fromfile(f"{GOLDEN}/{n}.22050.s16le.bin", dtype="<i2").astype(np.float32) for n in RECORDINGS]
    rng = np.random.default_rng(31)
    L = max(len(p) for p in pcms) + 3 * rate
    streams = np.zeros((L, n_ch), np.float32)
    for c in range(n_ch):
        p = pcms[c % len(pcms)]
        off = int(rng.integers(0, L - len(p)))
        streams[off:off + len(p), c] = p
    feeder = Feeder(streams, dtype)
    rx = sa.SameReceiverBuilder(rate).samedec().build_batch(n_ch, messages_only=True)
    rx.set_audio_capture(1 << 24)
    n_rows = rate * 3
    chunks = []
    while feeder.pos.min() < L:
        k = ragged_counts(rng, n_ch, n_rows, "half" if rng.uniform() < 0.5 else "zero").astype(np.int64)
        k = np.minimum(k, L - feeder.pos).astype(np.uint32)
        rx.process_ragged(torch.from_numpy(feeder.buffer(k, n_rows, False)).cuda(), k)
        chunks += rx.poll_audio()
    rx.flush()
    rx.sync()
    chunks += rx.poll_audio()
    assert rx.transport_on_device() == 1
    got = by_channel(rx.poll_events())
    cfg = ob.samedec_config(rate)
    zeros = np.zeros(4 * rate, np.float32)
    want_msgs, n_msgs = {}, 0
    for c in range(n_ch):
        own = feeder.x[:, c].astype(np.float32)
        want = [t for t in oracle_channel(ob, cfg, np.concatenate([own, zeros])) if t[0] in (18, 19)]
        assert got.get(c, []) == want, f"channel {c}"
        want_msgs[c] = [(t[0], t[1]) for t in want]
        n_msgs += len(want)
    assert n_msgs >= n_ch
    caps, samples, _ = join(sa, chunks)
    assert caps == expected_captures(want_msgs, flush_at=L)
    for c, a, b, _ in caps:
        assert np.array_equal(samples[(c, a)].view(np.int32), feeder.x[a:b, c].astype(np.float32).view(np.int32)), (c, a, b)


# ------------------------------------------------------------------ 6. resets and flush between ragged calls
def test_resets_and_flush_between_ragged_calls(sa, ob):
    rate, n_ch, n_rows, n_calls = 22050, 200, 30000, 6
    streams = sa.synth_afsk(n_ch, n_rows * n_calls, rate, seed=8, noise_sigma=0.05).cpu().numpy()
    feeder = Feeder(streams)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rng = np.random.default_rng(12)
    first = np.sort(rng.choice(n_ch, n_ch // 3, replace=False))
    second = np.sort(rng.choice(n_ch, n_ch // 5, replace=False))
    marks = {}                 # channel -> own positions of its resets

    def between(i):
        if i == 1:
            rx.reset_channels(first)
            for c in first:
                marks.setdefault(int(c), []).append(int(feeder.pos[c]))
        if i == 3:
            rx.reset_channels(second)
            for c in second:
                marks.setdefault(int(c), []).append(int(feeder.pos[c]))

    ragged_feed(sa, rx, feeder, rng, n_calls, n_rows, sa.LAYOUT_TIME_MAJOR, between)
    rx.flush()
    rx.sync()
    got = by_channel(rx.poll_events())
    cfg = ob.default_config(rate)
    zeros = np.zeros(rate * 4, np.float32)
    for c in range(n_ch):
        own = feeder.x[:feeder.pos[c], c]
        cuts = [0] + marks.get(c, []) + [len(own)]
        r = ob.Receiver(cfg)
        want = []
        for j in range(len(cuts) - 1):
            if j:
                r.reset()
            want += tuples(r.run(np.ascontiguousarray(own[cuts[j]:cuts[j + 1]])))
        want += tuples(r.run(zeros))
        assert got.get(c, []) == want, f"channel {c}"
        last = cuts[-2] if len(cuts) > 2 else 0
        assert rx.channel_input_sample_counter(c) == len(own) - last + len(zeros)


# ------------------------------------------------------------------ 7. refusals
def test_refusals_consume_nothing(sa):
    import torch
    rate, n_ch, n_rows = 22050, 64, 4000
    x = torch.zeros((n_rows, n_ch), dtype=torch.float32, device="cuda")
    good = np.full(n_ch, 100, np.uint32)
    for kw in ({"time_parallel": True}, {"call_invariant": True}, {"trace_symbols": True}):
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, **kw)
        with pytest.raises(sa.SameError) as ei:
            rx.process_ragged(x, good)
        assert ei.value.code == -1, kw
        assert rx.input_sample_counter() == 0
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rx.process_ragged(x, good)
    before = [rx.channel_input_sample_counter(c) for c in range(n_ch)]
    bad = good.copy(); bad[5] = n_rows + 1
    for k in (bad, good[:-1], np.concatenate([good, good[:1]])):
        with pytest.raises(sa.SameError) as ei:
            rx.process_ragged(x, k)
        assert ei.value.code == -1
    # the C entry point itself, with a NULL counts array
    rc = rx._L.same_batch_process_device_ragged(rx._h, x.data_ptr(), n_rows, None, sa.LAYOUT_TIME_MAJOR, None)
    assert rc == -1
    rx.sync()
    assert rx.input_sample_counter() == 100
    assert [rx.channel_input_sample_counter(c) for c in range(n_ch)] == before
    # all counts zero: a no-op
    rx.process_ragged(x, np.zeros(n_ch, np.uint32))
    assert rx.input_sample_counter() == 100


# ------------------------------------------------------------------ 8. input lifetime
def test_dropped_inputs_overwritten_change_nothing(sa):
    import torch
    rate, n_ch, n_rows, n_calls = 22050, 256, 20000, 6
    streams = sa.synth_afsk(n_ch, n_rows * n_calls, rate, seed=17, noise_sigma=0.05).cpu().numpy()
    rng = np.random.default_rng(4)
    counts = [ragged_counts(rng, n_ch, n_rows) for _ in range(n_calls)]

    def run(scribble):
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
        feeder = Feeder(streams)
        for k in counts:
            rx.process_ragged(torch.from_numpy(feeder.buffer(k, n_rows, False)).cuda(), k)
            if scribble:
                # whatever process_ragged's trimming let go of may be handed out again and overwritten at once
                junk = [torch.full((n_rows, n_ch), float("nan"), device="cuda") for _ in range(3)]
                del junk
        rx.sync()
        return tuples(rx.poll_events())

    assert run(True) == run(False)
