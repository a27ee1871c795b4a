"""The input-lifetime contract (include/same_rx.h, same_batch_process_device): a caller may overwrite or release a call's input
buffer once same_batch_sync returns, or once the second-next process call on the handle returns -- in every batch mode, the
call-invariant one included.  SameBatchReceiver.process_tensor relies on it when it drops its reference two calls later.

Each case queues the library's work behind a long, harmless gate kernel, so that everything the library does with an input is
still pending when the contract releases it.  The test then overwrites the released buffer from a stream that is not gated and
drops its reference.  A library that kept its promise delivers, bit for bit, what an ungated twin fed the same calls without
overwrites delivers (a batch is deterministic for a given call list); one that read a released buffer decodes garbage.  The
gate checks itself: right after the first call returns, an event behind the gate must still be pending."""
import numpy as np
import pytest

from helpers.oracle_compare import assert_every_channel_matches_oracle

pytestmark = pytest.mark.gpu

RATE = 22050
N_CH = 64
WINDOW = 18432                      # call-invariant window: several per stream
GATE_MS = 250.0                     # how long the gate kernel is to hold the library's stream
MSG_KINDS = (18, 19)
FIELDS = ("kind", "channel", "sample_counter", "symbol_count", "len", "bytes")

# Calls longer than a window (whole windows launched in place from the caller's buffer, the tail copied into the waiting
# buffer), calls shorter than one (only appended), odd lengths.  The first three calls launch once at most, so in a
# call-invariant batch nothing waits for the gate until x_0 has been released.
CALLS = [WINDOW + 3001, 4001, 2999, 5003, 2 * WINDOW + 777, 1111, 3, WINDOW - 5, 333]
N = RATE * 5
CALLS.append(N - sum(CALLS))

MODES = {
    "strict": {},
    "relaxed": {"relaxed": True},
    "time_parallel": {"time_parallel": True},
    "messages_only": {"messages_only": True},
    "ci_strict": {"call_invariant": True},
    "ci_relaxed": {"call_invariant": True, "relaxed": True},
    "ci_time_parallel": {"call_invariant": True, "time_parallel": True},
}
WINDOWED = ["ci_strict", "ci_relaxed", "ci_time_parallel"]


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


@pytest.fixture(scope="module")
def gate_cycles():
    """torch.cuda._sleep's argument for a gate of about GATE_MS: its clock is measured here, not assumed (a few bounded
    single-thread sleeps of at most ~0.1 s)."""
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles, ms = 1 << 20, 0.0
    for _ in range(5):
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 20.0:
            break
        cycles *= 8
    assert ms > 0.0, "torch.cuda._sleep did not take measurable time"
    want = int(cycles * GATE_MS / ms)
    with torch.cuda.stream(s):
        e0.record()
        torch.cuda._sleep(want)
        e1.record()
    e1.synchronize()
    print(f"\n[input-lifetime] gate: {want} cycles of torch.cuda._sleep measured {e0.elapsed_time(e1):.1f} ms")
    return want


@pytest.fixture(scope="module")
def stream_x(sa):
    import torch
    x = sa.synth_afsk(N_CH, N, RATE, seed=5151)
    torch.cuda.synchronize()
    return x


def ordered(ev):
    return ev[np.lexsort((np.arange(len(ev)), ev["channel"]))]


def make_batch(sa, mode):
    rx = sa.SameReceiverBuilder(RATE).build_batch(N_CH, **MODES[mode])
    if mode in WINDOWED:
        rx.set_call_window(WINDOW)
    return rx


def pieces(x, calls, dtype, layout_cm):
    """one buffer of its own per call"""
    import torch
    out, off = [], 0
    for k in calls:
        p = x[off:off + k]
        if dtype == "i16":
            p = p.round().to(torch.int16)
        out.append((p.t() if layout_cm else p).clone(memory_format=torch.contiguous_format))      # (a copy, never a view of x)
        off += k
    assert off == x.shape[0]
    torch.cuda.synchronize()
    return out


def scribble(buf):
    """overwrite a released input (on the current stream, which is not gated)"""
    import torch
    if buf.dtype == torch.int16:
        flat = buf.view(-1)
        flat[0::2] = 32767
        flat[1::2] = -32768
    else:
        buf.fill_(1.0e9)


def overwrite_stream():
    """The stream the overwrites come from.  HIP multiplexes streams onto a few hardware queues, and a queue that carries a
    gated stream's wait holds everything behind it: a stream of its own priority level gets a queue the gated ones do not
    share (assert_overwrites_run_ahead checks it)."""
    import torch
    lo, hi = torch.cuda.Stream.priority_range()
    return torch.cuda.Stream(priority=hi)


def assert_overwrites_run_ahead(ow, gate):
    """an overwrite queued on `ow` lands while the gate still holds the library's stream"""
    import torch
    probe = torch.empty(1024, device="cuda")
    with torch.cuda.stream(ow):
        probe.fill_(1.0)
    ow.synchronize()
    assert not gate.query(), "the overwrite stream waited for the gate: this case could not see a released buffer being read"


def gate_on(stream, cycles):
    """queue the gate kernel on `stream`; returns an event behind it"""
    import torch
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev.record()
    return ev


def assert_gate_pending(gate):
    assert not gate.query(), (f"the gate (about {GATE_MS} ms of torch.cuda._sleep) was over before the first call returned: it is "
                              "too short to hold the library's reads, and this case would pass whatever the library does")


def feed(sa, rx, bufs, layout, streams, gate=None, overwrite=None):
    """process bufs[k] on streams[k % len(streams)] (None: the library's own stream).  With `overwrite`, a stream that is not
    gated: once call k + 2 has returned, x_k is overwritten there and the test drops its reference."""
    import torch
    for k, b in enumerate(bufs):
        rx.process_device_ptr(b.data_ptr(), b.shape[0] if layout == sa.LAYOUT_TIME_MAJOR else b.shape[1], layout,
                              streams[k % len(streams)], b.dtype == torch.int16)
        if k == 0 and gate is not None:
            assert_gate_pending(gate)
        if overwrite is not None and k >= 2:
            with torch.cuda.stream(overwrite):
                scribble(bufs[k - 2])
            overwrite.synchronize()
            bufs[k - 2] = None
    rx.flush()
    rx.sync()
    if overwrite is not None:
        with torch.cuda.stream(overwrite):
            for b in bufs:
                if b is not None:
                    scribble(b)
        overwrite.synchronize()
    return ordered(rx.poll_events_np())


def assert_equal_runs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def assert_enough_events(sa, ev, mode, what):
    if mode == "messages_only":
        assert np.isin(ev["kind"], MSG_KINDS).sum() >= N_CH, what
    else:
        assert (ev["kind"] <= 3).sum() >= N_CH, what


def check_against_oracle(ob, x, ev, dtype):
    import torch
    xs = x.round() if dtype == "i16" else x
    xs = torch.cat([xs, torch.zeros(4 * RATE, N_CH, device=x.device)])
    assert assert_every_channel_matches_oracle(ob, ob.default_config(RATE), xs, ev) >= N_CH


@pytest.mark.parametrize("layout", ["time_major", "channel_major"])
@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_process_tensor_inputs_may_be_released_two_calls_later(sa, ob, gate_cycles, stream_x, mode, dtype, layout):
    """process_tensor on the library's own stream, which drops its reference to x_k after call k + 2; the test overwrites
    x_k then too."""
    import torch
    cm = layout == "channel_major"
    lay = sa.LAYOUT_CHANNEL_MAJOR if cm else sa.LAYOUT_TIME_MAJOR
    what = (mode, dtype, layout)

    twin = make_batch(sa, mode)
    for b in pieces(stream_x, CALLS, dtype, cm):
        twin.process_tensor(b, layout=lay)
    twin.flush(); twin.sync()
    want = ordered(twin.poll_events_np())
    assert_enough_events(sa, want, mode, what)

    rx = make_batch(sa, mode)
    bufs = pieces(stream_x, CALLS, dtype, cm)
    side, ow = torch.cuda.Stream(), overwrite_stream()
    gate = gate_on(side, gate_cycles)
    rx.order_after(side.cuda_stream)
    assert_overwrites_run_ahead(ow, gate)
    for k in range(len(bufs)):
        rx.process_tensor(bufs[k], layout=lay)
        if k == 0:
            assert_gate_pending(gate)
        if k >= 2:
            with torch.cuda.stream(ow):
                scribble(bufs[k - 2])
            ow.synchronize()
            bufs[k - 2] = None               # (process_tensor has dropped its own reference by now)
    rx.flush(); rx.sync()
    with torch.cuda.stream(ow):
        for b in bufs[-2:]:
            scribble(b)
    ow.synchronize()
    got = ordered(rx.poll_events_np())
    assert_equal_runs(got, want, what)
    if mode in ("strict", "ci_strict"):
        check_against_oracle(ob, stream_x, got, dtype)


@pytest.mark.parametrize("mode", list(MODES))
def test_caller_stream_inputs_may_be_released_two_calls_later(sa, ob, gate_cycles, stream_x, mode):
    """process_device_ptr on a stream of the caller's, gated itself; the overwrites come from a third stream."""
    import torch
    lay = sa.LAYOUT_TIME_MAJOR
    s = torch.cuda.Stream()
    twin = make_batch(sa, mode)
    want = feed(sa, twin, pieces(stream_x, CALLS, "f32", False), lay, [s.cuda_stream])
    assert_enough_events(sa, want, mode, mode)
    rx = make_batch(sa, mode)
    bufs = pieces(stream_x, CALLS, "f32", False)
    gate, ow = gate_on(s, gate_cycles), overwrite_stream()
    assert_overwrites_run_ahead(ow, gate)
    got = feed(sa, rx, bufs, lay, [s.cuda_stream], gate=gate, overwrite=ow)
    assert_equal_runs(got, want, mode)
    if mode in ("strict", "ci_strict"):
        check_against_oracle(ob, stream_x, got, "f32")


@pytest.mark.parametrize("layout", ["time_major", "channel_major"])
@pytest.mark.parametrize("mode", ["strict", "relaxed"] + WINDOWED)
def test_inputs_may_be_released_two_calls_later_when_the_calls_alternate_streams(sa, gate_cycles, stream_x, mode, layout):
    """Calls handed alternately to the library's own stream and to two streams of the caller, all gated."""
    import torch
    cm = layout == "channel_major"
    lay = sa.LAYOUT_CHANNEL_MAJOR if cm else sa.LAYOUT_TIME_MAJOR
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    order = [None, a.cuda_stream, b.cuda_stream, None, b.cuda_stream, a.cuda_stream]
    twin = make_batch(sa, mode)
    want = feed(sa, twin, pieces(stream_x, CALLS, "f32", cm), lay, order)
    assert_enough_events(sa, want, mode, (mode, layout))
    rx = make_batch(sa, mode)
    bufs = pieces(stream_x, CALLS, "f32", cm)
    side = torch.cuda.Stream()
    gate = gate_on(side, gate_cycles)
    a.wait_stream(side); b.wait_stream(side); rx.order_after(side.cuda_stream)
    ow = overwrite_stream()
    assert_overwrites_run_ahead(ow, gate)
    got = feed(sa, rx, bufs, lay, order, gate=gate, overwrite=ow)
    assert_equal_runs(got, want, (mode, layout))


SYNC_WINDOW = 6 * WINDOW
# 4.5 s in two calls, shorter than SYNC_WINDOW: both only append, and neither is the call after the previous one of another, so
# nothing but sync() waits for their copies.  (The longer one first: a channel-major call's staging buffers never grow.)
SYNC_CALLS = [60011, 39214]


@pytest.mark.parametrize("form", ["f32", "i16", "channel_major"])
@pytest.mark.parametrize("mode", WINDOWED)
def test_inputs_may_be_released_once_sync_returns(sa, gate_cycles, stream_x, mode, form):
    """Calls that only copy their samples into the waiting buffer, then sync(): every input is released at once.  The gate
    is still pending when sync() is called, so it is sync() that must wait for the copies; the samples are demodulated by the
    flush behind the overwrites."""
    import torch
    cm = form == "channel_major"
    lay = sa.LAYOUT_CHANNEL_MAJOR if cm else sa.LAYOUT_TIME_MAJOR
    dtype = "i16" if form == "i16" else "f32"
    x = stream_x[:sum(SYNC_CALLS)]

    def run(gated):
        rx = sa.SameReceiverBuilder(RATE).build_batch(N_CH, **MODES[mode])
        rx.set_call_window(SYNC_WINDOW)
        bufs = pieces(x, SYNC_CALLS, dtype, cm)
        side, ow = torch.cuda.Stream(), overwrite_stream()
        gate = gate_on(side, gate_cycles) if gated else None
        if gated:
            rx.order_after(side.cuda_stream)
            assert_overwrites_run_ahead(ow, gate)
        for b in bufs:
            rx.process_tensor(b, layout=lay)
        if gated:
            assert_gate_pending(gate)
        rx.sync()
        if gated:
            assert gate.query(), "sync() returned before the copies of the calls' samples, queued behind the gate, had run"
            with torch.cuda.stream(ow):
                for b in bufs:
                    scribble(b)
            ow.synchronize()
        del bufs
        rx.flush(); rx.sync()
        return ordered(rx.poll_events_np())

    want = run(False)
    assert_enough_events(sa, want, mode, (mode, form))
    assert_equal_runs(run(True), want, (mode, form))


# 4.5 s, every call shorter than a window; the longest first, so that the upload buffer is never reallocated (a hipFree waits for
# the whole device, and would make the second call wait for the gate whatever the library does)
HOST_CALLS = [17001, 3001, 14001, 2999, 15003, 777, 11, 1111, 16099, 12345, 16877]


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("mode", ["strict"] + WINDOWED)
def test_host_calls_behind_a_busy_stream(sa, gate_cycles, stream_x, mode, dtype):
    """process_host uploads each call into one device buffer of the batch's and processes it from there; in a call-invariant
    batch a short call is only appended to the waiting buffer, asynchronously, so the next upload must wait for that copy.
    (A call longer than the 256 MB upload slab goes through the same upload-and-process step once per slab, so short calls
    exercise the same ordering.)  A batch without windows synchronises every call: the gate is over when the first call
    returns.  In a call-invariant batch the first call returns with its copy still behind the gate, and the second call's
    upload must wait for that copy, so the gate is over when the second call returns.  The upload is a blocking copy on the
    legacy default stream; where the runtime queues it behind the gated stream (streams share a few hardware queues), the
    first call cannot return before the gate either, no upload can overtake a copy, and the case is skipped as unable to
    see the hazard."""
    import torch
    n = sum(HOST_CALLS)
    xh = stream_x[:n]
    xh = (xh.round().to(torch.int16) if dtype == "i16" else xh).cpu().numpy()

    def run(gated):
        rx = sa.SameReceiverBuilder(RATE).build_batch(N_CH, **MODES[mode])
        if mode in WINDOWED:
            rx.set_call_window(SYNC_WINDOW)
        side = torch.cuda.Stream()
        gate = gate_on(side, gate_cycles) if gated else None
        if gated:
            rx.order_after(side.cuda_stream)
        off = 0
        for i, k in enumerate(HOST_CALLS):
            rx.process_host(xh[off:off + k].copy())
            off += k
            if gated and i == 0:
                if mode in WINDOWED:
                    if gate.query():
                        rx.sync()
                        pytest.skip("the runtime queued the first upload behind the gated stream: an upload cannot overtake "
                                    "the copy of the call before here")
                else:
                    assert gate.query(), "process_host returned before its launch, queued behind the gate, had run"
            if gated and i == 1 and mode in WINDOWED:
                assert gate.query(), "the second upload did not wait for the copy of the first call's samples out of the upload buffer"
        rx.flush(); rx.sync()
        return ordered(rx.poll_events_np())

    want = run(False)
    assert_enough_events(sa, want, mode, (mode, dtype))
    assert_equal_runs(run(True), want, (mode, dtype))
