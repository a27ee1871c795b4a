"""Messages-only batches (SAME_BATCH_MESSAGES_ONLY, the counterpart of iter_messages()) on the GPU.

The queue must hold exactly the SAME_TRANSPORT_MSG_START / _END events a batch without the flag reports -- every field and
byte -- and nothing else; the transport layer that makes them runs on the device (same_transport.hip) except in
time-parallel batches.  Against the oracle for the recordings and the forced end of message, against a flagless twin fed
the same calls for everything else."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MSG_KINDS = (18, 19)          # SAME_TRANSPORT_MSG_START, SAME_TRANSPORT_MSG_END


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


def messages(ev):
    return ev[np.isin(ev["kind"], MSG_KINDS)]


def assert_same_messages(got, twin):
    """`got` (messages-only queue) equals `twin` (a flagless batch's queue) filtered to messages, record for record"""
    want = messages(twin)
    assert np.all(np.isin(got["kind"], MSG_KINDS)), np.unique(got["kind"])
    assert len(got) == len(want), (len(got), len(want))
    for f in ("kind", "channel", "sample_counter", "symbol_count", "len", "aux", "aux2"):
        assert np.array_equal(got[f], want[f]), f
    assert got.tobytes() == want.tobytes()


def oracle_messages(evs):
    return [(int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()) for e in evs if int(e.kind) in MSG_KINDS]


def load_pcm(name):
    return np.fromfile(os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), dtype="<i2")


def feed_both(rxs, x, cuts, layout=0, between=None):
    """x: torch CUDA tensor [T, C]; every batch of `rxs` gets the calls cuts[i]:cuts[i+1] (channel-major: transposed)"""
    for i in range(len(cuts) - 1):
        piece = x[cuts[i]:cuts[i + 1]]
        if layout == 1:
            piece = piece.t()
        piece = piece.contiguous()
        for rx in rxs:
            rx.process_tensor(piece, layout=layout)
        if between:
            between(i)
    for rx in rxs:
        rx.sync()


# ------------------------------------------------------------------ a. the recordings, against the oracle
@pytest.mark.parametrize("name", ["npt", "two_and_two", "long_message"])
def test_recordings_equal_the_oracles_messages(sa, ob, name):
    rate = 22050
    pcm = load_pcm(name).astype(np.float32)
    rx = sa.SameReceiverBuilder(rate).samedec().build_batch(1, messages_only=True)
    for off in range(0, len(pcm), rate * 2):
        rx.process_host(pcm[off:off + rate * 2])
    assert rx.transport_on_device() == 1
    rx.flush()
    rx.sync()
    got = [(int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()) for e in rx.poll_events()]
    tape = np.concatenate([pcm, np.zeros(4 * rate, np.float32)])
    want = oracle_messages(ob.Receiver(ob.samedec_config(rate)).run(tape))
    assert got == want
    assert any(k == 18 for k, _, _, _ in got)


# ------------------------------------------------------------------ b. full size, against a flagless twin
@pytest.mark.parametrize("rate,n_ch,seconds,relaxed,call_s,repeat", [
    (22050, 4096, 10.0, False, 2.0, 1),
    # the shard: one 2-s buffer streamed as six calls back to back, as bench.py streams it (a single 2 s holds no whole message)
    (22050, 32768, 2.0, True, 2.0, 6),
    (48000, 16384, 10.0, True, 2.5, 1),
])
def test_full_size_equals_the_flagless_twin(sa, rate, n_ch, seconds, relaxed, call_s, repeat):
    import torch
    n, step = int(rate * seconds), int(rate * call_s)
    x = sa.synth_afsk(n_ch, n, rate, seed=7, noise_sigma=0.05)
    twin = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=relaxed)
    mo = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=relaxed, messages_only=True)
    for _ in range(repeat):
        feed_both([twin, mo], x, list(range(0, n, step)) + [n])
    assert mo.transport_on_device() == 1 and twin.transport_on_device() == 0
    got, ref = mo.poll_events_np(1 << 24), twin.poll_events_np(1 << 24)
    del x
    torch.cuda.empty_cache()
    assert len(messages(ref)) >= 20
    assert np.all(got["kind"] >= 16), "a link event was queued"
    assert_same_messages(got, ref)
    assert mo.pack_bursts_np().shape[0] == 0


# ------------------------------------------------------------------ c. the forced end of message, against the oracle
def test_forced_end_of_message_across_calls(sa, ob):
    rate = 22050
    burst = ob.modulate_afsk(bytes([0xAB] * 16) + b"ZCZC-WXR-TOR-039173+0030-1591829-KCLE/NWS-", rate) * np.float32(16384.0)
    gap = np.zeros(rate, np.float32)
    x = np.concatenate([burst, gap, burst, gap, burst, np.zeros(2 * rate, np.float32), np.zeros(rate * 140, np.float32)])
    want = oracle_messages(ob.Receiver(ob.default_config(rate)).run(x))
    assert [k for k, _, _, _ in want] == [18, 19]
    rx = sa.SameReceiverBuilder(rate).build_batch(1, messages_only=True)
    # several calls: the instant is armed on the device between launches, as in streaming use
    for off in range(0, len(x), rate * 20):
        rx.process_host(x[off:off + rate * 20])
    got = [(int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()) for e in rx.poll_events()]
    assert got == want


# ------------------------------------------------------------------ d. resets and flush, against the twin
def test_resets_and_flush_equal_the_twin(sa):
    rate, n_ch = 22050, 256
    n, step = int(rate * 8.0), int(rate * 2.0)
    rng = np.random.default_rng(3)
    first = np.sort(rng.choice(n_ch, n_ch // 3, replace=False))
    second = np.sort(rng.choice(n_ch, n_ch // 5, replace=False))
    twin = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    mo = sa.SameReceiverBuilder(rate).build_batch(n_ch, messages_only=True)

    def between(i):
        # (no sync: the reset is queued behind the launches in flight)
        if i == 0:
            twin.reset_channels(first); mo.reset_channels(first)
        if i == 2:
            twin.reset_channels(second); mo.reset_channels(second)

    x = sa.synth_afsk(n_ch, n, rate, seed=11, noise_sigma=0.05)
    feed_both([twin, mo], x, list(range(0, n, step)) + [n], between=between)
    twin.flush(); mo.flush()
    twin.sync(); mo.sync()
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert len(messages(ref)) >= 20
    assert_same_messages(got, ref)
    # reset() of the whole batch, then a new stream
    twin.reset(); mo.reset()
    x = sa.synth_afsk(n_ch, n, rate, seed=12, noise_sigma=0.05)
    feed_both([twin, mo], x, [0, 3 * step // 2, n])
    twin.flush(); mo.flush()
    twin.sync(); mo.sync()
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert len(messages(ref)) >= 20
    assert_same_messages(got, ref)


# ------------------------------------------------------------------ e. other input forms and modes, against the twin
@pytest.mark.parametrize("form", ["i16", "channel_major", "call_invariant_relaxed"])
def test_input_forms_equal_the_twin(sa, form):
    import torch
    rate, n_ch = 22050, 128
    n = int(rate * 7.0)
    cuts = [0, 30011, 30011 + 44100, 100000, n]
    kw = {"relaxed": True, "call_invariant": True} if form == "call_invariant_relaxed" else {}
    twin = sa.SameReceiverBuilder(rate).build_batch(n_ch, **kw)
    mo = sa.SameReceiverBuilder(rate).build_batch(n_ch, messages_only=True, **kw)
    x = sa.synth_afsk(n_ch, n, rate, seed=17, noise_sigma=0.05)
    if form == "i16":
        x = torch.clamp(torch.round(x), -32768, 32767).to(torch.int16)
    feed_both([twin, mo], x, cuts, layout=1 if form == "channel_major" else 0)
    twin.flush(); mo.flush()
    twin.sync(); mo.sync()
    assert mo.transport_on_device() == 1
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert len(messages(ref)) >= 20
    assert_same_messages(got, ref)


# ------------------------------------------------------------------ f. time-parallel: transport layer on the host
def test_time_parallel_equals_the_twin(sa):
    rate, n_ch = 22050, 128
    n = rate * 10
    twin = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    mo = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True, messages_only=True)
    for rx in (twin, mo):
        rx.time_parallel_config(max_chunks=4)
    x = sa.synth_afsk(n_ch, n, rate, seed=19, noise_sigma=0.05)
    feed_both([twin, mo], x, [0, n // 2, n])
    assert mo.time_parallel_chunks() == 4
    assert mo.transport_on_device() == 0
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert len(messages(ref)) >= 20
    assert_same_messages(got, ref)


# ------------------------------------------------------------------ g. flags
def test_link_only_and_messages_only_are_refused(sa):
    with pytest.raises(sa.SameError) as err:
        sa.SameReceiverBuilder(22050).build_batch(64, link_only=True, messages_only=True)
    assert err.value.code == -1          # SAME_EINVAL
