"""Per-channel reset of a batched receiver (same_batch_reset_channels / SameBatchReceiver.reset_channels) on the GPU.

Strict mode against the oracle, bit for bit: a channel reset between two calls equals an oracle receiver that ran the samples
before, was reset(), then ran the rest (counters from 0); every other channel equals the oracle over the whole stream.  The
fast modes against strict mode's events for the same stream and resets, under their existing contracts; call-invariant mode
against itself, cut into two different call lists."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

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


def by_channel(evs):
    out = {}
    for e in evs:
        out.setdefault(int(e.channel), []).append((int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()))
    return out


def oracle_tuples(evs):
    return [(int(e.kind), int(e.sample_counter), int(e.symbol_count), e.data()) for e in evs]


def reset_set(n_ch, seed=5):
    """a scattered third of the channels"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n_ch, n_ch // 3, replace=False))


def synth(sa, n_ch, n, rate, seed, noise):
    return sa.synth_afsk(n_ch, n, rate, seed=seed, noise_sigma=noise).cpu().numpy()


def feed(rx, x, cuts, layout, dtype, between=None):
    """x [T, C] f32 host array, fed as torch device tensors in the calls cuts[i]:cuts[i+1]; `between(i)` runs after call i"""
    import torch
    import sameold_amd as sa
    xd = np.clip(np.rint(x), -32768, 32767).astype(np.int16) if dtype == "i16" else x
    for i in range(len(cuts) - 1):
        piece = xd[cuts[i]:cuts[i + 1]]
        if layout == sa.LAYOUT_CHANNEL_MAJOR:
            piece = piece.T
        rx.process_tensor(torch.from_numpy(np.ascontiguousarray(piece)).cuda(), layout=layout)
        if between:
            between(i)


RATES = [22050, 48000]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("layout_name,dtype", [("time", "f32"), ("time", "i16"), ("channel", "f32"), ("channel", "i16")])
def test_mid_stream_reset_strict_equals_the_oracle(sa, ob, rate, layout_name, dtype):
    n_ch = 256
    n = int(rate * 5.2)
    cuts = [0, n // 5, n // 2, (3 * n) // 4, n]           # reset behind call 2 of 4
    split = cuts[2]
    x = synth(sa, n_ch, n, rate, seed=11, noise=0.15)
    if dtype == "i16":
        x = np.clip(np.rint(x), -32768, 32767).astype(np.int16).astype(np.float32)
    layout = sa.LAYOUT_TIME_MAJOR if layout_name == "time" else sa.LAYOUT_CHANNEL_MAJOR
    chans = reset_set(n_ch)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)

    def between(i):
        if i == 1:
            assert rx.input_sample_counter() == split
            rx.reset_channels(chans)
            assert rx.channel_input_sample_counter(int(chans[0])) == 0
            assert rx.input_sample_counter() == split        # the batch's own counter does not move

    feed(rx, x, cuts, layout, dtype, between=between)
    rx.sync()
    assert rx.channel_input_sample_counter(int(chans[0])) == n - split
    untouched = int(np.setdiff1d(np.arange(n_ch), chans)[0])
    assert rx.channel_input_sample_counter(untouched) == n
    got = by_channel(rx.poll_events())
    cfg = ob.default_config(rate)
    in_burst = 0
    is_reset = np.zeros(n_ch, bool); is_reset[chans] = True
    for c in range(n_ch):
        col = np.ascontiguousarray(x[:, c])
        ref = ob.Receiver(cfg)
        if is_reset[c]:
            pre = oracle_tuples(ref.run(col[:split]))
            link = [k for k, *_ in pre if k < 16]
            in_burst += bool(link) and link[-1] in (sa.LINK_SEARCHING, sa.LINK_READING)
            ref.reset()
            want = pre + oracle_tuples(ref.run(col[split:]))
        else:
            want = oracle_tuples(ref.run(col))
        assert got.get(c, []) == want, f"channel {c} ({'reset' if is_reset[c] else 'untouched'})"
    assert in_burst >= 3, f"only {in_burst} channels were reset in the middle of a burst"


def test_reset_does_not_wait_for_the_launch_in_flight(sa, ob):
    """Two calls, a reset, a third call: the second call's launch is still in flight (its events are not on the host yet) when
    reset_channels returns, and they keep the old numbering when they arrive."""
    import torch
    rate, n_ch = 22050, 64
    n1 = n2 = n3 = int(rate * 1.7)
    x = synth(sa, n_ch, n1 + n2 + n3, rate, seed=3, noise=0.1)
    chans = np.arange(0, n_ch, 2)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    xd = torch.from_numpy(x).cuda()
    rx.process_tensor(xd[:n1].contiguous())
    rx.process_tensor(xd[n1:n1 + n2].contiguous())
    before = rx.pending_events()
    rx.reset_channels(torch.from_numpy(chans.astype(np.int64)))       # a CPU tensor
    assert rx.pending_events() == before, "reset_channels collected the launch in flight"
    rx.process_tensor(xd[n1 + n2:].contiguous())
    rx.sync()
    got = by_channel(rx.poll_events())
    cfg = ob.default_config(rate)
    late = 0
    for c in range(n_ch):
        col = np.ascontiguousarray(x[:, c])
        ref = ob.Receiver(cfg)
        if c % 2 == 0:
            pre = oracle_tuples(ref.run(col[:n1 + n2]))
            late += sum(1 for e in pre if e[1] >= n1)
            ref.reset()
            want = pre + oracle_tuples(ref.run(col[n1 + n2:]))
        else:
            want = oracle_tuples(ref.run(col))
        assert got.get(c, []) == want, f"channel {c}"
    assert late > 0      # (the second launch did carry events of reset channels)


def test_out_of_range_channel_resets_nothing(sa, ob):
    rate, n_ch = 22050, 64
    n = int(rate * 3.0)
    x = synth(sa, n_ch, n, rate, seed=9, noise=0.1)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    rx.process_host(x[: n // 2])
    with pytest.raises(sa.SameError) as e:
        rx.reset_channels([3, n_ch])
    assert e.value.code == -1
    with pytest.raises(sa.SameError):
        rx.reset_channels(np.array([1 << 31], dtype=np.uint32))
    rx.reset_channels([])                    # an empty list is allowed
    assert rx.channel_input_sample_counter(3) == n // 2
    rx.process_host(x[n // 2:])
    got = by_channel(rx.poll_events())
    cfg = ob.default_config(rate)
    for c in range(n_ch):
        assert got.get(c, []) == oracle_tuples(ob.Receiver(cfg).run(np.ascontiguousarray(x[:, c]))), f"channel {c}"


def test_duplicates_equal_a_single_reset(sa):
    rate, n_ch = 22050, 64
    x = synth(sa, n_ch, int(rate * 3.0), rate, seed=4, noise=0.05)
    out = []
    for lst in ([5, 9, 5, 9, 9], [9, 5]):
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch)
        rx.process_host(x[:30000])
        rx.reset_channels(lst)
        rx.process_host(x[30000:])
        out.append(by_channel(rx.poll_events()))
    assert out[0] == out[1]


def load_pcm(name):
    return np.fromfile(os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), dtype="<i2")


def test_decode_recordings(sa, ob):
    rate = 22050
    names = ["npt", "two_and_two", "long_message"]
    recs = [load_pcm(nm) for nm in names]
    syn = synth(sa, 3, int(rate * 9.0), rate, seed=21, noise=0.05)
    recs += [np.ascontiguousarray(syn[: int(rate * s), i]) for i, s in enumerate((3.1, 9.0, 5.55))]
    got = sa.decode_recordings(recs, rate, 2, builder=sa.SameReceiverBuilder(rate).samedec(), max_call_samples=rate)
    assert len(got) == len(recs) and all(got)
    # a channel that takes the next recording has been reset(), not rebuilt (AGC gain 1.0, equalizer and timing loop keep their
    # state): the oracle of a recording is its channel's receiver after the recordings before it, reset
    chan = [int(evs[0].channel) for evs in got]
    assert all(all(int(e.channel) == c for e in evs) for c, evs in zip(chan, got))
    assert chan[:2] == [0, 1] and set(chan) == {0, 1}
    cfg = ob.samedec_config(rate)
    refs = {0: ob.Receiver(cfg), 1: ob.Receiver(cfg)}
    for i, (rec, evs) in enumerate(zip(recs, got)):
        tape = np.concatenate([rec.astype(np.float32), np.zeros(4 * rate, np.float32)])
        ref = refs[chan[i]]
        want = oracle_tuples(ref.run(tape))
        ref.reset()
        assert [t for t in oracle_tuples(evs) if t[0] < 16] == [t for t in want if t[0] < 16], f"recording {i}: link events"
        if i < len(names):
            txt = open(os.path.join(GOLDEN, f"{names[i]}.22050.s16le.txt")).read().splitlines()
            headers = [e.data().decode() for e in evs if e.kind == sa.TRANSPORT_MSG_START]
            assert headers == [l for l in txt if l.startswith("ZCZC")], f"{names[i]}: headers"


# ------------------------------------------------------------------ fast modes, against strict mode with the same resets
def quiet_reset_set(sa, ev_strict_pre, n_ch, split, rate, seed=5):
    """A scattered third of the channels, leaving out those with a link event within 12 symbols before the reset: a burst
    finishing right at the reset is reported or not depending on the few symbols the fast modes' events may be late"""
    sps = rate / 520.83
    busy = set(int(e.channel) for e in ev_strict_pre if e.kind < 16 and split - 12 * sps <= e.sample_counter)
    rng = np.random.default_rng(seed)
    cand = np.array([c for c in range(n_ch) if c not in busy])
    return np.sort(rng.choice(cand, min(len(cand), n_ch // 3), replace=False))


def stitched(pre, post, chans, split):
    """one channel-ordered event array: what was delivered before the reset, then after it, a reset channel's counters after
    the reset moved back onto the stream's"""
    post = post.copy()
    post["sample_counter"][np.isin(post["channel"], chans)] += split
    ev = np.concatenate([pre, post])
    return ev[np.argsort(ev["channel"], kind="stable")]


def run_with_reset(sa, rate, x, cuts, chans, layout, **kw):
    rx = sa.SameReceiverBuilder(rate).build_batch(x.shape[1], **kw)
    if kw.get("time_parallel"):
        rx.time_parallel_config(max_chunks=4)
    pre = []

    def between(i):
        if i == 1:
            rx.sync()
            pre.append(rx.poll_events_np())
            rx.reset_channels(chans)

    feed(rx, x, cuts, layout, "f32", between=between)
    rx.sync()
    return pre[0], rx.poll_events_np(), rx


@pytest.mark.parametrize("mode", ["relaxed", "time_parallel"])
def test_mid_stream_reset_fast_modes_meet_the_contract(sa, mode):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_time_parallel import assert_contract
    if mode == "relaxed":
        rate, n_ch, n, layout, kw = 44100, 256, int(44100 * 6.0), sa.LAYOUT_TIME_MAJOR, {"relaxed": True}
    else:
        rate, n_ch, n, layout, kw = 22050, 256, 4 * 66000, sa.LAYOUT_CHANNEL_MAJOR, {"time_parallel": True}
    cuts = [0, n // 4, n // 2, (3 * n) // 4, n]
    split = cuts[2]
    seed = 13
    x = synth(sa, n_ch, n, rate, seed=seed, noise=0.0)
    probe = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    probe.process_host(x[:split])
    chans = quiet_reset_set(sa, probe.poll_events(), n_ch, split, rate)
    del probe
    pre_s, post_s, _ = run_with_reset(sa, rate, x, cuts, chans, layout)
    pre_f, post_f, rxf = run_with_reset(sa, rate, x, cuts, chans, layout, **kw)
    if mode == "time_parallel":
        assert rxf.time_parallel_chunks() > 1
    ref = stitched(pre_s, post_s, chans, split)
    got = stitched(pre_f, post_f, chans, split)
    # (t_end: a burst cut by the end of the input is decoded differently by the two arithmetics; stitched() puts every
    # channel's events on the stream's time, so the end of the input is n for all of them)
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(seed, c), what=mode, t_end=n)


def test_call_invariant_with_resets(sa):
    """The same samples and resets cut into two different call lists -- one with calls shorter than a window around the
    reset -- give identical events."""
    rate, n_ch = 22050, 128
    n = int(rate * 6.0)
    x = synth(sa, n_ch, n, rate, seed=17, noise=0.05)
    chans = reset_set(n_ch, seed=2)
    split = 61234
    lists = [[0, 30000, split, 100000, n], [0, 12345, 41000, 55000, split, 62000, 64500, 90000, n]]
    outs = []
    for cuts in lists:
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=True, call_invariant=True)
        i_split = cuts.index(split) - 1

        def between(i, rx=rx, i_split=i_split):
            if i == i_split:
                rx.reset_channels(chans)
                assert rx.channel_input_sample_counter(int(chans[0])) == 0

        feed(rx, x, cuts, sa.LAYOUT_TIME_MAJOR, "f32", between=between)
        rx.flush()
        rx.sync()
        ev = rx.poll_events_np()
        outs.append(ev[np.argsort(ev["channel"], kind="stable")])
    a, b = outs
    assert len(a) == len(b) and len(a) > 100
    for f in ("kind", "channel", "sample_counter", "symbol_count", "len", "bytes"):
        assert np.array_equal(a[f], b[f]), f
