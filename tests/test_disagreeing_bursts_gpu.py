"""The transport layer on the GPU against the oracle on messages whose bursts disagree (tests/helpers/disagreeing_bursts.py).

Everywhere else the GPU suite shows the transport layer three identical bursts.  Here 21 classes x 8 channels carry bursts
with flipped bits (one, two, the same one twice, three in one byte, the high bit), bursts that are cut, missing, late, a
fourth one or another message's, and end-of-message bursts that are corrupted, single or absent; a second batch carries two
messages back to back.  With such bursts a START is not delivered at a burst but at a deadline poll: the device reports that
poll as a wake-up tick, and on a messages-only batch transport_kernel (same_transport.hip over same_transport_dev.h) turns
it into the message.  The audio is clean, so every comparison is exact; tests/test_disagreeing_bursts_cpu.py shows on the
oracle alone that the batches do what they are built for.

  a. a strict batch without the flag equals the oracle on every channel in EVERY event: link events and transport events
     16 .. 20, sample counter, symbol count, length, aux, aux2, bytes (the host replay and the tick machinery)
  b. a strict messages-only batch: its queue equals the oracle's START / END in every field and the flagless twin's byte
     for byte, and the transport layer ran on the device
  c. the same under odd call lengths (with STARTs that fall into a launch behind the last burst's which holds no link
     event of the channel), int16, channel-major, a ragged call, per-channel resets, flush(), the forced end of message
  d. relaxed arithmetic: messages-only equals its flagless twin byte for byte; kind, channel and text equal strict mode's
     on the classes whose bursts are whole
  e. time-parallel messages-only (transport layer on the host): kind, channel and text equal strict mode's on those classes

Every case prints one "DISAGREE" line with what it compared.
"""
import numpy as np
import pytest

from helpers import disagreeing_bursts as db
from helpers import impairments as im

pytestmark = pytest.mark.gpu

SEED = 2027
START, END = 18, 19
MSG_KINDS = (START, END)


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


@pytest.fixture(autouse=True)
def default_kernels(monkeypatch):
    for k in ("SAME_RELAXED_KERNEL", "SAME_SYM", "SAME_RELAXED", "SAME_PIPE", "SAME_PIPE_LANES", "SAME_TP_KERNEL"):
        monkeypatch.delenv(k, raising=False)


_BATCHES, _ORACLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_batches():
    """the batches and the oracle's events are shared by the cases of this module and dropped with it"""
    yield
    _BATCHES.clear()
    _ORACLE.clear()


def the_batch(name, rate, width=None):
    """"batch": 21 classes x 8 channels at 22.05 kHz (168: the transport kernel's last wavefront is partly filled), x 3 at
    48 kHz (63); "two_messages": 8 channels; "open": the classes that leave a message open (and one that ends it), 3 channels
    each, for the forced end of message.  width: the batch widened to that many channels by repeating its first ones -- the
    wavefront pipeline, the symbol-paced pipeline and the time-parallel mode take whole groups of 16 / 64 channels only."""
    key = (name, rate)
    if key not in _BATCHES:
        if name == "batch":
            _BATCHES[key] = db.batch(rate, SEED, 8 if rate == 22050 else 3)
        elif name == "two_messages":
            _BATCHES[key] = db.two_message_batch(rate, SEED)
        else:
            _BATCHES[key] = db.batch(rate, SEED, 3, classes=("unanimous", "eom_nnzz", "eom_single", "eom_none"))
    b = _BATCHES[key]
    n_ch = b["x"].shape[1]
    if width is None or width == n_ch:
        return b
    key = (name, rate, width)
    if key not in _BATCHES:
        _BATCHES[key] = dict(b, x=np.ascontiguousarray(np.concatenate([b["x"], b["x"][:, :width - n_ch]], axis=1)),
                             cls=b["cls"] + b["cls"][:width - n_ch])
    return _BATCHES[key]


def widened(events, width):
    """the oracle's events of a batch widened by the_batch(width=...)"""
    return events + events[:width - len(events)]


def the_oracle(ob, key, rate, make_x, **kw):
    """the oracle's events per channel for the samples make_x() returns, computed once per module run and never changed"""
    if key not in _ORACLE:
        _ORACLE[key] = db.oracle_events(ob, ob.default_config(rate), make_x(), **kw)
    return _ORACLE[key]


def by_channel(ev, n_ch):
    """a polled queue (numpy EVENT_DTYPE) as per-channel lists of (kind, sample_counter, symbol_count, len, aux, aux2, bytes),
    in queue order: launches come in order and a launch's events are ordered by channel, then time"""
    out = [[] for _ in range(n_ch)]
    for r in ev:
        n = min(int(r["len"]), 288)
        out[int(r["channel"])].append((int(r["kind"]), int(r["sample_counter"]), int(r["symbol_count"]), int(r["len"]),
                                       int(r["aux"]), int(r["aux2"]), r["bytes"][:n].tobytes()))
    return out


def only_messages(events):
    return [[e for e in ev if e[0] in MSG_KINDS] for ev in events]


def whole_channels(b):
    """the channels of the classes whose bursts are all whole"""
    return [c for c, name in enumerate(b["cls"]) if name in db.WHOLE]


def kind_and_text(events, channels):
    return {int(c): [(e[0], e[6]) for e in events[c] if e[0] in MSG_KINDS] for c in channels}


def assert_same_messages(got, twin):
    """`got` (a messages-only queue) equals `twin` (a flagless batch's queue) filtered to messages, record for record"""
    want = twin[np.isin(twin["kind"], MSG_KINDS)]
    assert np.all(np.isin(got["kind"], MSG_KINDS)), np.unique(got["kind"])
    assert len(got) == len(want), (len(got), len(want))
    for f in ("kind", "channel", "sample_counter", "symbol_count", "len", "aux", "aux2"):
        assert np.array_equal(got[f], want[f]), f
    assert got.tobytes() == want.tobytes()


def assert_channels_equal(got, want, b, what):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: channel {c} ({b['cls'][c]}):\n device {g}\n oracle {w}"


def build(sa, monkeypatch, rate, n_ch, family=None, **kw):
    """a batch of the strict kernel family named (None: the library's own choice), or of the relaxed / time-parallel mode in kw"""
    if family in ("fast", "pipe"):
        monkeypatch.setenv("SAME_PIPE", "1" if family == "pipe" else "0")          # read when the batch is created
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, generic_kernel=(family == "generic"), **kw)
    if family is not None:
        name = rx.kernel_name()
        assert name.startswith("demod_kernel<") if family == "generic" else name == f"demod_{family}_kernel", name
    return rx


def feed(rxs, x, cuts, layout=0):
    """x: torch CUDA tensor [T, C]; every batch of `rxs` gets the calls cuts[i]:cuts[i+1] (channel-major: transposed)"""
    for a, z in zip(cuts[:-1], cuts[1:]):
        piece = x[a:z]
        piece = (piece.t() if layout == 1 else piece).contiguous()
        for rx in rxs:
            rx.process_tensor(piece, layout=layout)
    for rx in rxs:
        rx.sync()


def even_cuts(T, step):
    return list(range(0, T, step)) + [T]


def count(events):
    return sum(len(e) for e in events)


# (name, rate, width, strict kernel family): 168 and 63 channels run the one-wavefront kernels, 192 and 64 the wavefront pipeline,
# which keeps a launch's deadline ring in registers
CASES = [("batch", 22050, 168, "fast"), ("batch", 22050, 168, "generic"), ("batch", 22050, 192, "pipe"), ("batch", 48000, 63, "fast"),
         ("batch", 48000, 64, "pipe"), ("two_messages", 22050, 8, None)]
CASE_IDS = [f"{n}-{r}-{w}-{f or 'default'}" for n, r, w, f in CASES]


# ------------------------------------------------------------------ a. flagless, strict: every event
@pytest.mark.parametrize("name,rate,width,family", CASES, ids=CASE_IDS)
def test_strict_batch_equals_the_oracle_in_every_event(sa, ob, monkeypatch, name, rate, width, family):
    import torch
    b = the_batch(name, rate, width)
    T, n_ch = b["x"].shape
    want = widened(the_oracle(ob, (name, rate), rate, lambda: the_batch(name, rate)["x"]), width)
    rx = build(sa, monkeypatch, rate, n_ch, family)
    feed([rx], torch.from_numpy(b["x"]).cuda(), even_cuts(T, 2 * rate + 77))
    assert rx.transport_on_device() == 0
    got = by_channel(rx.poll_events_np(), n_ch)
    assert_channels_equal(got, want, b, f"strict {rx.kernel_name()} {rate} Hz")
    n_tr = sum(e[0] >= 16 for ev in want for e in ev)
    assert n_tr >= 3 * n_ch
    print(f"DISAGREE a. strict {rx.kernel_name()} {name} {rate} Hz: {n_ch} channels, {count(want)} events "
          f"({count(want) - n_tr} link, {n_tr} transport, {count(only_messages(want))} START / END) equal the oracle's")


# ------------------------------------------------------------------ b. messages-only, strict
@pytest.mark.parametrize("name,rate,width,family", CASES, ids=CASE_IDS)
def test_messages_only_batch_equals_the_oracle_and_the_twin(sa, ob, monkeypatch, name, rate, width, family):
    import torch
    b = the_batch(name, rate, width)
    T, n_ch = b["x"].shape
    want = only_messages(widened(the_oracle(ob, (name, rate), rate, lambda: the_batch(name, rate)["x"]), width))
    twin = build(sa, monkeypatch, rate, n_ch, family)
    mo = build(sa, monkeypatch, rate, n_ch, family, messages_only=True)
    feed([twin, mo], torch.from_numpy(b["x"]).cuda(), even_cuts(T, 2 * rate + 77))
    assert mo.transport_on_device() == 1 and twin.transport_on_device() == 0
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert_channels_equal(by_channel(got, n_ch), want, b, f"messages-only {mo.kernel_name()} {rate} Hz")
    assert_same_messages(got, ref)
    assert count(want) >= n_ch
    print(f"DISAGREE b. messages-only {mo.kernel_name()} {name} {rate} Hz: {n_ch} channels, {count(want)} START / END equal "
          f"the oracle's and the flagless twin's")


# ------------------------------------------------------------------ c. calls and forms, messages-only against the oracle
ODD_CALL = 9973          # 0.45 s at 22.05 kHz: shorter than the silence in which a deadline falls


def late_starts(events, cuts):
    """the channels on which a START comes at a deadline poll in a launch (call) behind the one of the last burst before it,
    and that launch holds no link event of the channel at all"""
    cuts = np.asarray(cuts)
    launch = lambda s: int(np.searchsorted(cuts, s, side="left")) - 1          # sample counter s counts the samples up to and with its own
    out = []
    for c, ev in enumerate(events):
        for e in db.deadline_starts(ev):
            bursts = [q[1] for q in ev if q[0] == 3 and q[1] < e[1]]
            k = launch(e[1])
            if bursts and launch(bursts[-1]) < k and not any(q[0] < 16 and launch(q[1]) == k for q in ev):
                out.append(c)
                break
    return out


@pytest.mark.parametrize("width,family", [(168, "fast"), (192, "pipe")])
def test_odd_calls_deliver_starts_in_launches_without_link_events(sa, ob, monkeypatch, width, family):
    import torch
    rate = 22050
    b = the_batch("batch", rate, width)
    T, n_ch = b["x"].shape
    events = widened(the_oracle(ob, ("batch", rate), rate, lambda: the_batch("batch", rate)["x"]), width)
    cuts = even_cuts(T, ODD_CALL)
    late = late_starts(events, cuts)
    assert len(late) >= 10, f"only {len(late)} channels get their START in a launch of its own"
    mo = build(sa, monkeypatch, rate, n_ch, family, messages_only=True)
    feed([mo], torch.from_numpy(b["x"]).cuda(), cuts)
    assert mo.transport_on_device() == 1
    want = only_messages(events)
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, f"{len(cuts) - 1} calls of {ODD_CALL}")
    print(f"DISAGREE c. odd calls {mo.kernel_name()}: {len(cuts) - 1} calls of {ODD_CALL} samples, {n_ch} channels, {count(want)} START / END equal the oracle's; "
          f"on {len(late)} channels the START arrived at a deadline in a launch without link events of the channel")


@pytest.mark.parametrize("form", ["i16", "channel_major"])
def test_input_forms_equal_the_oracle(sa, ob, monkeypatch, form):
    import torch
    rate = 22050
    b = the_batch("batch", rate)
    T, n_ch = b["x"].shape
    if form == "i16":
        host = im.to_int16(b["x"])
        want = only_messages(the_oracle(ob, ("batch", rate, "i16"), rate, lambda: host))          # the oracle on the same int16 samples
    else:
        host = b["x"]
        want = only_messages(the_oracle(ob, ("batch", rate), rate, lambda: host))
    mo = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feed([mo], torch.from_numpy(host).cuda(), [0, 70001, 150002, T], layout=1 if form == "channel_major" else 0)
    assert mo.transport_on_device() == 1
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, form)
    print(f"DISAGREE c. {form}: {n_ch} channels, {count(want)} START / END equal the oracle's")


def test_ragged_calls_equal_the_oracle(sa, ob, monkeypatch):
    """The first call leaves every other channel behind by a count of its own (501, 538, ... samples); the lag stays until the
    last call, in which only the lagging channels still have samples.  Each channel's events are the oracle's on the
    channel's own stream, in its own sample numbering."""
    import torch
    from test_ragged_calls import Feeder
    rate, n_rows = 22050, 30011
    b = the_batch("batch", rate)
    T, n_ch = b["x"].shape
    want = only_messages(the_oracle(ob, ("batch", rate), rate, lambda: b["x"]))
    lag = np.zeros(n_ch, np.int64)
    lag[1::2] = 501 + 37 * np.arange(len(lag[1::2]))
    assert len(set(lag[1::2])) == n_ch // 2 and lag.max() < n_rows
    mo = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feeder = Feeder(b["x"])
    counts = (n_rows - lag).astype(np.uint32)
    n_calls = 0
    while True:
        mo.process_ragged(torch.from_numpy(feeder.buffer(counts, int(counts.max()), False)).cuda(), counts)
        n_calls += 1
        left = T - feeder.pos
        if not left.any():
            break
        counts = np.minimum(left, n_rows).astype(np.uint32)
    mo.sync()
    assert mo.transport_on_device() == 1
    assert all(mo.channel_input_sample_counter(c) == T for c in range(0, n_ch, 5))
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, "ragged")
    print(f"DISAGREE c. ragged: {n_calls} calls, {n_ch // 2} channels lagging by {lag[1]} .. {lag.max()} samples, {n_ch} channels, "
          f"{count(want)} START / END equal the oracle's")


def test_channel_resets_between_the_bursts_equal_the_oracle(sa, ob, monkeypatch):
    """reset_channels of every other channel 3.8 s into the stream: behind burst 2 and in front of burst 3 on every channel,
    so the two bursts in the assembler and the message they have pending are gone, and burst 3 stands alone.  The oracle is
    reset at the same sample; a reset channel counts from 0 again."""
    import torch
    rate = 22050
    b = the_batch("batch", rate)
    T, n_ch = b["x"].shape
    at = int(3.8 * rate) + 1
    chans = np.arange(0, n_ch, 2)
    resets = [at if c % 2 == 0 else None for c in range(n_ch)]
    events = the_oracle(ob, ("batch", rate, "reset"), rate, lambda: b["x"], resets=resets)
    plain = the_oracle(ob, ("batch", rate), rate, lambda: b["x"])
    for c in chans:                                             # the reset falls into silence, behind at most two bursts
        before = [e for e in plain[c] if e[0] < 16 and e[1] < at]
        assert before[-1][0] == 0 and sum(e[0] == 3 for e in before) <= 2, c
        if b["cls"][c] in ("unanimous", "one_flip", "four_bursts", "late_third"):
            assert sum(e[0] == 3 for e in before) == 2, c
    want = only_messages(events)
    assert sum(want[c] != only_messages(plain)[c] for c in chans) >= len(chans) // 2          # (the reset changed the outcome)
    mo = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    x = torch.from_numpy(b["x"]).cuda()
    feed([mo], x, [0, 40003, at])
    mo.reset_channels(chans)
    feed([mo], x, [at, at + 60001, T])
    assert mo.transport_on_device() == 1
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, "reset")
    print(f"DISAGREE c. resets: {len(chans)} of {n_ch} channels reset at sample {at}, {count(want)} START / END equal the oracle's")


@pytest.mark.parametrize("cut_s", [6.6, 11.2])
def test_flush_in_place_of_silence_equals_the_oracle(sa, ob, monkeypatch, cut_s):
    """flush() where the input stops: 11.2 s, in the silence behind the last burst; and 6.6 s, behind the header bursts and in
    front of every end-of-message burst, where most STARTs are still pending and their deadlines pass inside the flush."""
    import torch
    rate = 22050
    b = the_batch("batch", rate)
    n_ch = b["x"].shape[1]
    cut = int(cut_s * rate) + 3
    tape = lambda: np.concatenate([b["x"][:cut], np.zeros((4 * rate, n_ch), np.float32)])
    events = the_oracle(ob, ("batch", rate, "flush", cut), rate, tape)
    want = only_messages(events)
    in_flush = sum(e[0] == START and e[1] > cut for ev in want for e in ev)
    if cut_s < 7.0:
        assert in_flush >= n_ch // 2
    mo = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feed([mo], torch.from_numpy(b["x"][:cut]).cuda(), [0, 80001, cut])
    mo.flush()
    mo.sync()
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, f"flush at {cut}")
    print(f"DISAGREE c. flush at {cut_s} s: {n_ch} channels, {count(want)} START / END equal the oracle's, {in_flush} STARTs inside the flush")


def test_forced_end_of_message_where_none_was_sent(sa, ob, monkeypatch):
    """The classes whose message is never ended (NNZZ, one NNNN, none), and one that is, followed by 136 s of silence: the
    oracle ends an open message at the first poll 135 s behind its START.  On the device that instant is armed by
    transport_kernel between launches (State::wake_sample) and comes back as a wake-up tick."""
    import torch
    rate = 22050
    b = the_batch("open", rate)
    T, n_ch = b["x"].shape
    n_zero, step = 136 * rate, 20 * rate + 11
    tape = lambda: np.concatenate([b["x"], np.zeros((n_zero, n_ch), np.float32)])
    want = only_messages(the_oracle(ob, ("open", rate), rate, tape))
    forced = [c for c in range(n_ch) if b["cls"][c] != "unanimous"]
    for c in forced:
        assert [e[0] for e in want[c]] == [START, END] and want[c][1][1] > want[c][0][1] + 135 * rate, c
    mo = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feed([mo], torch.from_numpy(b["x"]).cuda(), [0, T])
    zeros = torch.zeros((step, n_ch), dtype=torch.float32, device="cuda")
    for off in range(0, n_zero, step):
        mo.process_tensor(zeros[:min(step, n_zero - off)])
    mo.sync()
    assert mo.transport_on_device() == 1
    assert_channels_equal(by_channel(mo.poll_events_np(), n_ch), want, b, "forced end of message")
    print(f"DISAGREE c. forced end of message: {n_ch} channels, {count(want)} START / END equal the oracle's, {len(forced)} ENDs forced")


# ------------------------------------------------------------------ d. relaxed arithmetic
RELAXED_KERNEL = {"sym": "demod_sym_kernel", "fastmath": "demod_pipe_kernel<fastmath>", "wave": "demod_relaxed_kernel"}


@pytest.mark.parametrize("rate,width,family", [(22050, 192, "sym"), (22050, 192, "fastmath"), (22050, 168, "wave"), (48000, 64, "sym")])
def test_relaxed_messages_only_equals_its_twin_and_strict_mode(sa, monkeypatch, rate, width, family):
    """Byte for byte against the relaxed flagless twin on every class, the truncated ones included; against strict mode in
    kind, channel and text on the classes whose bursts are whole (aux, aux2 and sample counters are not promised across
    arithmetics).  168 channels, not whole groups of 64, run the one- / two-wavefront relaxed kernel."""
    import torch
    if family == "fastmath":
        monkeypatch.setenv("SAME_SYM", "0")
    b = the_batch("batch", rate, width)
    T, n_ch = b["x"].shape
    x = torch.from_numpy(b["x"]).cuda()
    twin = build(sa, monkeypatch, rate, n_ch, relaxed=True)
    mo = build(sa, monkeypatch, rate, n_ch, relaxed=True, messages_only=True)
    strict = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feed([twin, mo, strict], x, even_cuts(T, 2 * rate + 77))
    assert mo.kernel_name() == twin.kernel_name() == RELAXED_KERNEL[family], mo.kernel_name()
    assert mo.transport_on_device() == 1
    got, ref = mo.poll_events_np(), twin.poll_events_np()
    assert_same_messages(got, ref)
    whole = whole_channels(b)
    mine, theirs = kind_and_text(by_channel(got, n_ch), whole), kind_and_text(by_channel(strict.poll_events_np(), n_ch), whole)
    for c in whole:
        assert mine[int(c)] == theirs[int(c)], f"channel {c} ({b['cls'][c]}): relaxed {mine[int(c)]}, strict {theirs[int(c)]}"
    n = sum(len(v) for v in theirs.values())
    assert n >= len(whole)
    print(f"DISAGREE d. relaxed {mo.kernel_name()} {rate} Hz: {len(got)} START / END on {n_ch} channels equal the relaxed twin's byte for byte; "
          f"{n} on {len(whole)} whole-burst channels equal strict mode's in kind, channel and text")


# ------------------------------------------------------------------ e. time-parallel: transport layer on the host
@pytest.mark.parametrize("layout", ["time_major", "channel_major"])
def test_time_parallel_messages_only_equals_strict_mode(sa, monkeypatch, layout):
    import torch
    rate = 22050
    b = the_batch("batch", rate, 192)
    T, n_ch = b["x"].shape
    x = torch.from_numpy(b["x"]).cuda()
    strict = build(sa, monkeypatch, rate, n_ch, messages_only=True)
    feed([strict], x, [0, T])
    tp = build(sa, monkeypatch, rate, n_ch, time_parallel=True, messages_only=True)
    tp.time_parallel_config(max_chunks=4)
    feed([tp], x, [0, T // 2 + 5, T], layout=1 if layout == "channel_major" else 0)
    assert tp.time_parallel_chunks() >= 2
    assert tp.transport_on_device() == 0
    got = tp.poll_events_np()
    assert np.all(np.isin(got["kind"], MSG_KINDS))
    whole = whole_channels(b)
    mine, theirs = kind_and_text(by_channel(got, n_ch), whole), kind_and_text(by_channel(strict.poll_events_np(), n_ch), whole)
    for c in whole:
        assert mine[int(c)] == theirs[int(c)], f"channel {c} ({b['cls'][c]}): time-parallel {mine[int(c)]}, strict {theirs[int(c)]}"
    n = sum(len(v) for v in theirs.values())
    assert n >= len(whole)
    print(f"DISAGREE e. time-parallel {layout} {tp.time_parallel_chunks()} chunks: {n} START / END on {len(whole)} whole-burst channels "
          f"equal strict mode's in kind, channel and text")
