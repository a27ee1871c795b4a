"""Alert audio per message (same_batch_set_audio_capture) on the GPU: the capture of a message is the channel's samples
x[som.sample_counter, next.sample_counter) -- what samedec hands its alert command -- and nothing else.

Against the oracle's messages and against samedec_gpu's children for the recordings; against the input and the batch's own queued
messages at full size, in every mode, layout and sample type whose transport layer runs on the device; call invariance,
resets, flush, overflow, refusals and the input-lifetime contract."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_input_lifetime import gate_cycles  # noqa: F401  (the calibrated gate of the input-lifetime tests, a module fixture)

pytestmark = pytest.mark.gpu

MSG_START, MSG_END = 18, 19
END_MESSAGE, END_FLUSH, END_RESET, FIRST, TRUNCATED = 2, 4, 8, 1, 16


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


def load_pcm(name):
    return np.fromfile(os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), dtype="<i2")


def expected_captures(msgs, flush_at=None, resets=()):
    """The rule (include/same_rx.h) over one stream in batch counters.  msgs: {channel: [(kind, counter)]} in time order;
    flush_at: where the flush's zeros begin; resets: [(position, set of channels)].  -> sorted [(channel, from, to, end)]"""
    out = []
    for c, lst in msgs.items():
        ev = [(m, 0, k) for k, m in lst] + [(r, 1, 0) for r, chans in resets if c in chans]
        if flush_at is not None:
            ev.append((flush_at, 2, 0))
        ev.sort(key=lambda e: (e[0], e[1]))
        open_from = None
        for pos, typ, kind in ev:
            if typ:
                if open_from is not None:
                    out.append((c, open_from, pos, END_RESET if typ == 1 else END_FLUSH))
                open_from = None
            elif flush_at is not None and pos > flush_at:
                if kind == MSG_START:
                    out.append((c, pos, pos, END_FLUSH))
            else:
                if open_from is not None:
                    out.append((c, open_from, pos, END_MESSAGE))
                open_from = pos if kind == MSG_START else None
        assert open_from is None or flush_at is None
    return sorted(out)


def join(sa, chunks, base=None):
    """chunks -> sorted [(channel, from, to, end)] and {(channel, from): samples}; base(channel, i): what to add to the
    counter of chunks[i] (rebased channel counters -> batch counters)"""
    j = sa.AudioJoiner()
    done = []
    for i, (c, counter, flags, s) in enumerate(chunks):
        done += j.feed([(c, counter + (base(c, i) if base else 0), flags, s)])
    assert not j.open, f"{len(j.open)} captures still open"
    caps = sorted((d["channel"], d["sample_counter"], d["sample_counter"] + len(d["samples"]), d["end"]) for d in done)
    return caps, {(d["channel"], d["sample_counter"]): d["samples"] for d in done}, done


def join_lengths(chunks):
    """join() for chunks whose samples were checked already: (channel, counter, flags, n_samples) -> sorted captures"""
    ends = END_MESSAGE | END_FLUSH | END_RESET
    open_, caps = {}, []
    for c, k, f, n in chunks:
        if f & FIRST:
            assert c not in open_, (c, k)
            open_[c] = [k, k]
        cur = open_[c]
        assert k == cur[1], (c, k, cur)
        cur[1] = k + n
        if f & ends:
            caps.append((c, cur[0], cur[1], f & ends))
            del open_[c]
    assert not open_
    return sorted(caps)


def queued_messages(ev, base=None):
    msgs = {}
    for i, e in enumerate(ev):
        if int(e["kind"]) in (MSG_START, MSG_END):
            c = int(e["channel"])
            msgs.setdefault(c, []).append((int(e["kind"]), int(e["sample_counter"]) + (base(c, i) if base else 0)))
    return msgs


def verify_on_device(x, caps, samples):
    """every capture (c, a, b) equals the stream's x[a:b, c], bit for bit; x: CUDA tensor [T, C] (f32 or int16).  Gathered on
    the device in groups."""
    import torch
    group, n = [], 0

    def flush_group():
        if not group:
            return
        rows = np.concatenate([np.arange(a, b, dtype=np.int64) for c, a, b in group])
        cols = np.concatenate([np.full(b - a, c, dtype=np.int64) for c, a, b in group])
        want = x[torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()].float()
        got = torch.from_numpy(np.concatenate([samples[(c, a)] for c, a, b in group])).cuda()
        assert torch.equal(want.view(torch.int32), got.view(torch.int32)), "captured samples differ from the input"
        group.clear()

    for c, a, b, _ in caps:
        if b > a:
            group.append((c, a, b))
            n += b - a
            if n >= 1 << 25:
                flush_group()
                n = 0
    flush_group()


def oracle_captures(ob, pcm, rate=22050):
    """(som, next, end) of every message of the oracle over pcm + the flush's zeros"""
    tape = np.concatenate([pcm.astype(np.float32), np.zeros(4 * rate, np.float32)])
    evs = [(int(e.kind), int(e.sample_counter)) for e in ob.Receiver(ob.samedec_config(rate)).run(tape) if int(e.kind) in (MSG_START, MSG_END)]
    return expected_captures({0: evs}, flush_at=len(pcm))


def run_recording(sa, pcm, calls, rate=22050, i16=False):
    rx = sa.SameReceiverBuilder(rate).samedec().build_batch(1, messages_only=True)
    rx.set_audio_capture(1 << 22)
    x = pcm if i16 else pcm.astype(np.float32)
    chunks, off = [], 0
    for k in calls:
        rx.process_host(x[off:off + k])
        chunks += rx.poll_audio()
        off += k
    if off < len(x):
        rx.process_host(x[off:])
    rx.flush()
    rx.sync()
    return chunks + rx.poll_audio()


# ------------------------------------------------------------------ 1. the recordings, against the oracle
@pytest.mark.parametrize("name", ["npt", "two_and_two", "long_message"])
def test_recordings_equal_the_oracles_spans(sa, ob, name):
    pcm = load_pcm(name)
    chunks = run_recording(sa, pcm, [44100, 30011, 44100, 12345, 44100], i16=name == "two_and_two")
    caps, samples, _ = join(sa, chunks)
    want = oracle_captures(ob, pcm)
    assert caps == want
    # (long_message's one header is only produced by the flush: its capture is empty)
    assert any(b > a for _, a, b, _ in caps) == (name != "long_message")
    pcmf = pcm.astype(np.float32)
    for c, a, b, end in caps:
        assert samples[(c, a)].tobytes() == pcmf[a:b].tobytes()
    # FIRST on exactly one chunk per capture, an END_* flag on exactly its last
    assert sum(1 for ch in chunks if ch[2] & FIRST) == len(caps)
    assert sum(1 for ch in chunks if ch[2] & (END_MESSAGE | END_FLUSH | END_RESET)) == len(caps)
    assert not any(ch[2] & TRUNCATED for ch in chunks)


# ------------------------------------------------------------------ 2. against samedec_gpu's alert command
@pytest.mark.parametrize("name", ["npt", "two_and_two", "long_message"])
def test_samedec_children_get_the_captures(sa, name, tmp_path):
    from sameold_amd import build as sbuild
    out = tmp_path / "children"
    out.mkdir()
    p = subprocess.run([sbuild.SAMEDEC, "--rate", "22050", "--file", os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), "--",
                        sys.executable, os.path.join(ROOT, "tests", "helpers", "samedec_child_dump.py"), str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    children = [open(f, "rb").read() for f in sorted(glob.glob(str(out / "*.s16le")))]
    pcm = load_pcm(name)
    _, _, done = join(sa, run_recording(sa, pcm, [44100] * (len(pcm) // 44100)))
    caps = [d["samples"].astype(np.int16).tobytes() for d in done]
    assert [c for c in children if c] == [c for c in caps if c]
    if name == "long_message":
        assert children == caps == [b""]
    else:
        assert any(children)


# ------------------------------------------------------------------ 3. at scale, against the input and the batch's own messages
def feed(sa, rxs, x, cuts, layout, dtype, host=False, between=None):
    import torch
    polls = [[] for _ in rxs]
    for i in range(len(cuts) - 1):
        piece = x[cuts[i]:cuts[i + 1]]
        if dtype == "i16":
            piece = piece.round().clamp(-32768, 32767).to(torch.int16)
        if layout == 1:
            piece = piece.t()
        piece = piece.contiguous()
        for rx, pl in zip(rxs, polls):
            if host:
                rx.process_host(piece.cpu().numpy(), layout=layout)
            else:
                rx.process_tensor(piece, layout=layout)
            pl.append(rx.poll_audio() if rx is rxs[0] else [])
        if between:
            between(i)
    return polls


SCALE = [
    # name, rate, channels, seconds, relaxed, dtype, layout, host
    ("strict_4096x10s", 22050, 4096, 10.0, False, "f32", 0, False),
    ("relaxed_shard", 22050, 32768, 8.0, True, "f32", 0, False),
    ("relaxed_48k", 48000, 4096, 12.0, True, "f32", 0, False),
    ("i16_time_major", 22050, 256, 8.0, False, "i16", 0, False),
    ("f32_channel_major", 22050, 256, 8.0, False, "f32", 1, False),
    ("i16_channel_major_relaxed", 22050, 256, 8.0, True, "i16", 1, False),
    ("host_f32", 22050, 256, 8.0, False, "f32", 0, True),
    ("host_i16_channel_major", 22050, 256, 8.0, False, "i16", 1, True),
]


@pytest.mark.parametrize("name,rate,n_ch,seconds,relaxed,dtype,layout,host", SCALE, ids=[s[0] for s in SCALE])
def test_captures_equal_the_input_at_the_batchs_messages(sa, name, rate, n_ch, seconds, relaxed, dtype, layout, host):
    import torch
    n = int(rate * seconds)
    x = sa.synth_afsk(n_ch, n, rate, seed=23, noise_sigma=0.05)
    if dtype == "i16":
        x = x.round().clamp(-32768, 32767).to(torch.int16)
    rng = np.random.default_rng(sum(name.encode()))
    if n_ch == 32768:
        cuts = list(range(0, n + 1, 2 * rate))      # the shard: 2-s calls
    else:
        cuts = [0] + sorted(rng.choice(np.arange(1, n), 4, replace=False).tolist()) + [n]
    max_call = max(b - a for a, b in zip(cuts, cuts[1:]))
    mo = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=relaxed, messages_only=True)
    twin = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=relaxed, messages_only=True)
    mo.set_audio_capture(max_call * n_ch)
    chunks = []

    def keep(pl):
        # the samples are checked against the input as they arrive, by chunk (a chunk's channel counter is the batch's here);
        # only their lengths are kept
        verify_on_device(x, [(c, k, k + len(a), 0) for c, k, f, a in pl], {(c, k): a for c, k, f, a in pl})
        chunks.extend((c, k, f, len(a)) for c, k, f, a in pl)

    for pl in feed(sa, [mo, twin], x, cuts, layout, "f32", host=host)[0]:
        keep(pl)
    for rx in (mo, twin):
        rx.flush()
        rx.sync()
    keep(mo.poll_audio())
    ev, ev_twin = mo.poll_events_np(1 << 24), twin.poll_events_np(1 << 24)
    assert ev.tobytes() == ev_twin.tobytes(), "capture changed the event queue"
    assert twin.poll_audio() == []
    want = expected_captures(queued_messages(ev), flush_at=n)
    assert sum(1 for w in want if w[2] > w[1]) >= n_ch // 16, "too few messages to say anything"
    caps = join_lengths(chunks)
    assert caps == want
    assert sum(n for _, _, _, n in chunks) == sum(b - a for _, a, b, _ in want), "a sample outside a capture was delivered"
    assert not any(ch[2] & TRUNCATED for ch in chunks)


# ------------------------------------------------------------------ 4. call invariance
def test_call_invariant_chunks_do_not_depend_on_the_calls(sa):
    import torch
    rate, n_ch = 22050, 128
    n = int(rate * 7.0)
    x = sa.synth_afsk(n_ch, n, rate, seed=29, noise_sigma=0.05)
    lists = [[0, n], [0, 30011, 30011 + 44100, 100000, n], [0, 3, 18432, 18433, 60000, n - 5, n],
             list(range(0, n, 7001)) + [n]]
    streams = []
    for cuts in lists:
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=True, call_invariant=True, messages_only=True)
        rx.set_audio_capture(1 << 22)
        chunks = []
        for pl in feed(sa, [rx], x, cuts, 0, "f32")[0]:
            chunks += pl
        rx.flush()
        rx.sync()
        chunks += rx.poll_audio()
        streams.append([(c, k, f, s.tobytes()) for c, k, f, s in chunks])
        ev = rx.poll_events_np()
    for s in streams[1:]:
        assert s == streams[0]
    caps, samples, _ = join(sa, [(c, k, f, np.frombuffer(b, np.float32)) for c, k, f, b in streams[0]])
    assert caps == expected_captures(queued_messages(ev), flush_at=n)
    assert sum(1 for w in caps if w[2] > w[1]) >= 20
    verify_on_device(x, caps, samples)


# ------------------------------------------------------------------ 5. resets and flush
def test_resets_end_captures_and_flush_zeros_are_never_captured(sa):
    rate, n_ch = 22050, 128
    step = int(rate * 3.0)
    n_calls = 6
    n = n_calls * step
    rng = np.random.default_rng(31)
    first = set(rng.choice(n_ch, n_ch // 2, replace=False).tolist())
    second = set(rng.choice(n_ch, n_ch // 3, replace=False).tolist())
    x = sa.synth_afsk(n_ch, n, rate, seed=37, noise_sigma=0.05)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, messages_only=True)
    rx.set_audio_capture(step * n_ch)
    # one launch per call; a call's poll brings in the launch before it (the one of the previous call)
    tagged, ev_tagged = [], []

    def poll(launch):
        tagged.extend((launch, ch) for ch in rx.poll_audio())
        ev_tagged.extend((launch, e) for e in rx.poll_events_np())

    R1, R2 = 3 * step, 4 * step
    for i in range(n_calls):
        rx.process_tensor(x[i * step:(i + 1) * step].contiguous())
        poll(i - 1)
        if i == 2:
            rx.reset_channels(sorted(first))     # behind the launch in flight: applied at its harvest
        if i == 3:
            rx.sync()
            poll(3)
            rx.reset_channels(sorted(second))    # nothing in flight: the open captures end now
            poll(3)
    rx.flush()
    rx.sync()
    poll(n_calls - 1)

    def base(c, launch):
        b = 0
        if c in first and launch * step >= R1:
            b = R1
        if c in second and launch * step >= R2:
            b = R2
        return b

    chunks = [ch for _, ch in tagged]
    caps, samples, done = join(sa, chunks, base=lambda c, i: base(c, tagged[i][0]))
    ev = [e for _, e in ev_tagged]
    msgs = queued_messages(ev, base=lambda c, i: base(c, ev_tagged[i][0]))
    resets = [(R1, first), (R2, second)]
    want = expected_captures(msgs, flush_at=n, resets=resets)
    assert caps == want
    verify_on_device(x, caps, samples)
    # END_RESET chunks: empty, at the reset position in the channel's counters before the reset
    ends = [(c, k) for _, (c, k, f, s) in tagged if f & END_RESET]
    assert len(ends) >= 10 and all(len(s) == 0 for _, (c, k, f, s) in tagged if f & END_RESET)
    assert sorted(ends) == sorted((c, b - (R1 if (c in first and b == R2) else 0)) for c, a, b, e in want if e == END_RESET)
    # captures that began after a reset count from it (their samples were checked at counter + reset position above)
    assert any(f & FIRST and c in second and launch >= 4 for launch, (c, k, f, s) in tagged)
    # no flush zero is captured: every capture with samples ends at or before the flush position (a message the flush itself
    # yields has an empty one)
    assert all(b <= n for _, a, b, _ in caps if b > a)
    assert all(e == END_FLUSH for _, a, b, e in caps if b > n)
    assert any(e == END_FLUSH for *_, e in caps)
    # reset() empties the audio queue
    rx.process_tensor(x[:step].contiguous())
    rx.process_tensor(x[step:2 * step].contiguous())
    rx.reset()
    assert rx.poll_audio() == []


# ------------------------------------------------------------------ 6. a pool that overflows
def test_a_full_pool_truncates_marks_and_recovers(sa):
    import torch
    rate, n_ch = 22050, 64
    big, small = rate * 8, 4096
    x = sa.synth_afsk(n_ch, big + 40 * small, rate, seed=41, noise_sigma=0.05)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, messages_only=True)
    rx.set_audio_capture(small * n_ch)         # far less than the first call keeps inside messages
    tagged = []
    rx.process_tensor(x[:big].contiguous())
    for i in range(40):
        rx.process_tensor(x[big + i * small:big + (i + 1) * small].contiguous())
        tagged += [(i, ch) for ch in rx.poll_audio()]     # poll i: launch i - 1 (launch -1: the big call)
    with pytest.raises(sa.SameError) as err:
        rx.sync()
    assert err.value.code == -7                # SAME_EOVERFLOW
    tagged += [(40, ch) for ch in rx.poll_audio()]
    trunc = [ch for i, ch in tagged if ch[2] & TRUNCATED]
    assert trunc and all(i == 0 for i, ch in tagged if ch[2] & TRUNCATED), "only the big launch overflows"
    # what was delivered is the input at its counters
    xs = x.cpu().numpy()
    for _, (c, k, f, s) in tagged:
        assert s.tobytes() == xs[k:k + len(s), c].tobytes()
    # the later launches capture normally: their chunks join up with nothing missing
    later = [(i, ch) for i, ch in tagged if i >= 2]
    assert later and not any(ch[2] & TRUNCATED for _, ch in later)
    assert sum(len(ch[3]) for _, ch in later) > 0


# ------------------------------------------------------------------ 7. refusals
def test_capture_is_refused_where_the_input_is_gone(sa):
    b = sa.SameReceiverBuilder(22050)
    for kw in ({}, {"messages_only": True, "time_parallel": True}):
        rx = b.build_batch(64, **kw)
        with pytest.raises(sa.SameError) as err:
            rx.set_audio_capture(1 << 20)
        assert err.value.code == -1
    rx = b.build_batch(64, messages_only=True)
    rx.process_host(np.zeros((100, 64), np.float32))
    with pytest.raises(sa.SameError) as err:
        rx.set_audio_capture(1 << 20)
    assert err.value.code == -1
    rx.reset()
    rx.set_audio_capture(1 << 20)
    rx.set_audio_capture(0)


# ------------------------------------------------------------------ 8. the input-lifetime contract
@pytest.mark.parametrize("mode", ["strict", "call_invariant"])
def test_released_inputs_do_not_reach_the_audio(sa, gate_cycles, stream_x, mode):
    import torch
    from test_input_lifetime import (CALLS, N_CH, RATE, WINDOW, assert_gate_pending, assert_overwrites_run_ahead, gate_on,
                                     overwrite_stream, pieces, scribble)
    CALLS = CALLS * 3                # (15 s: the synthetic workload's first messages come after about 5 s)
    kw = {"relaxed": True, "call_invariant": True} if mode == "call_invariant" else {}

    def make():
        rx = sa.SameReceiverBuilder(RATE).build_batch(N_CH, messages_only=True, **kw)
        if mode == "call_invariant":
            rx.set_call_window(WINDOW)
        rx.set_audio_capture(max(CALLS) * N_CH)
        return rx

    twin = make()
    chunks_twin = []
    for b in pieces(stream_x, CALLS, "f32", False):
        twin.process_tensor(b)
        chunks_twin += twin.poll_audio()
    twin.flush(); twin.sync()
    chunks_twin += twin.poll_audio()
    assert sum(len(c[3]) for c in chunks_twin) > 0

    rx = make()
    bufs = pieces(stream_x, CALLS, "f32", False)
    side, ow = torch.cuda.Stream(), overwrite_stream()
    gate = gate_on(side, gate_cycles)
    rx.order_after(side.cuda_stream)
    assert_overwrites_run_ahead(ow, gate)
    chunks = []
    for k in range(len(bufs)):
        rx.process_tensor(bufs[k])
        if k == 0:
            assert_gate_pending(gate)
        chunks += rx.poll_audio()
        if k >= 2:
            with torch.cuda.stream(ow):
                scribble(bufs[k - 2])
            ow.synchronize()
            bufs[k - 2] = None
    rx.flush(); rx.sync()
    with torch.cuda.stream(ow):
        for b in bufs[-2:]:
            scribble(b)
    ow.synchronize()
    chunks += rx.poll_audio()
    key = lambda cs: sorted((c, k, f, s.tobytes()) for c, k, f, s in cs)
    assert key(chunks) == key(chunks_twin)


@pytest.fixture(scope="module")
def stream_x(sa):
    import torch
    from test_input_lifetime import N, N_CH, RATE
    x = sa.synth_afsk(N_CH, 3 * N, RATE, seed=5151)
    torch.cuda.synchronize()
    return x
