"""Every kernel family against the oracle on distorted and broken signals (tests/helpers/impairments.py).

Elsewhere the GPU tests decode textbook bursts.  Here one batch of 16 classes x 16 channels per rate carries clock skew, detuned
tones, DC offsets and steps, mains hum, an in-band tone, echoes, clipping, fades, level steps, near-silent and very loud
carriers, bursts that are cut, interrupted, missing their preamble or their header, run into a second preamble, or carry
bytes the framer rejects, and echoes on which the oracle's equalizer decides transmitted bytes (eq_echo: the class that holds
the relaxed kernels' NLMS update; the echoes of gain up to 0.5 do not).
tests/test_impairments_cpu.py shows on the oracle alone that these batches leave its trivial regime,
that it decodes the distortion classes with a margin of 1.5, and which channels it decides the same way under a perturbation
of 1 % of the carrier (the stability mask, recomputed here the same way).

  strict    generic, fast and pipe kernels: tolerance zero on every channel of every class -- all link events, burst bytes
            included, and on four channels per class the symbol trace bit for bit; int16, channel-major, odd call lengths, a
            ragged call that ends inside the bursts; samedec's gain limits; a longer equalizer with the timing clamp narrowed
            to 1 % skew (the default clamp lies beyond what the oracle decodes: test_impairments_cpu.py); headers of more than 288 bytes
  relaxed   sym, pipe-fastmath and wave-relaxed kernels against strict mode under include/same_rx.h's contract as
            tests/test_time_parallel.py::assert_contract states it, nothing looser: burst bytes equal, link events within 2
            symbols, on the stable channels of the 15 classes that met the cap of a quarter unstable (impairments.ADMITTED); soft
            symbols within 0.05 with equal sign up to impairments.SOFT_LIMIT; unstable channels must complete with ordered events
  time-parallel   the 22.05 kHz workload of synth_afsk with DC, hum, echo, clipping, a fade and a level step, both layouts

The module's name sorts behind every other GPU test module on purpose.  It builds some 150 batches, each with streams of its
own, and the HIP runtime hands hardware queues to streams in the order they are made: run earlier in the same process it moved
the queue that tests/test_input_lifetime.py's gated stream shares with the legacy default stream, and one of that module's
cases then skipped as unable to see its hazard.  Run last it changes nothing for any other module.

Every case prints one "IMPAIRED" line per class with what it compared and the worst differences it saw
(profiles/r09_impaired_vs_oracle.txt is made of them).
"""
import ctypes as C

import numpy as np
import pytest

from helpers import impairments as im
from helpers.oracle_compare import assert_every_channel_matches_oracle
from test_time_parallel import SOFT_SYMBOL_TOLERANCE, assert_contract, split, strict_events

pytestmark = pytest.mark.gpu

SEED = 2026
TRACE_FIELDS = ("sample_counter", "zero", "sym", "err", "next")
TRACED_PER_CLASS = (0, 5, 10, 15)          # mild ... the test level


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


_BATCHES, _MASKS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_batches():
    """the batches and masks are shared by the cases of this module and dropped with it"""
    yield
    _BATCHES.clear()
    _MASKS.clear()


def the_batch(rate):
    if rate not in _BATCHES:
        _BATCHES[rate] = im.batch(rate, SEED)
    return _BATCHES[rate]


def the_mask(ob, rate, form="f32", narrow=False):
    """the stability mask of the batch as the kernels get it (float32, or int16 after the saturating rounding), for the default
    configuration or the one with the narrowed timing clamp: computed once per module run, never stored"""
    key = (rate, form, narrow)
    if key not in _MASKS:
        b = the_batch(rate)
        _MASKS[key] = im.stability_mask(ob, config(ob, rate, "narrow" if narrow else "default")[1], b["x64"], b["amplitude"], SEED,
                                        quantize=im.to_int16 if form == "i16" else None)
    return _MASKS[key]


def config(ob, rate, name, sa=None):
    """(builder or None, oracle configuration) by name"""
    L = ob.lib()
    b = sa.SameReceiverBuilder(rate) if sa is not None else None
    if name == "samedec":
        cfg = ob.samedec_config(rate)
        if b is not None:
            b.samedec()
        return b, cfg
    cfg = ob.default_config(rate)
    if name in ("narrow", "long_equalizer"):
        L.so_config_with_timing_max_deviation(C.byref(cfg), im.NARROW_CLAMP)
        if b is not None:
            b.with_timing_max_deviation(im.NARROW_CLAMP)
    if name == "long_equalizer":
        L.so_config_with_adaptive_equalizer(C.byref(cfg), 8, 3, 0.05, 1.0e-6)
        if b is not None:
            b.with_adaptive_equalizer(8, 3, 0.05, 1.0e-6)
    return b, cfg


def ordered(ev):
    return ev[np.lexsort((np.arange(len(ev)), ev["channel"]))]          # events come per launch: (channel, time) order


def assert_traces_equal_the_oracle(ob, cfg, rx, x_host, channels, what):
    for c in channels:
        ref = ob.Receiver(cfg)
        ref.enable_trace(4096)
        ref.run(np.ascontiguousarray(x_host[:, c]))
        want, got = ref.trace(), rx.read_trace(c, cap=4096)
        assert len(got) == len(want) > 0, f"{what} channel {c}: {len(got)} traced symbols, oracle {len(want)}"
        for f in TRACE_FIELDS:
            same = np.array_equal(got[f], want[f]) if f == "sample_counter" else np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32))
            assert same, f"{what} channel {c}: trace field {f} differs from the oracle's"


def traced_channels(b):
    return [r[i] for name in b["classes"] for r in [im.class_channels(b, name)] for i in TRACED_PER_CLASS]


# ------------------------------------------------------------------ strict: tolerance zero
STRICT = [("generic", 22050), ("generic", 44100), ("generic", 48000), ("generic", 16000),
          ("fast", 22050), ("fast", 44100), ("fast", 48000), ("pipe", 22050), ("pipe", 44100), ("pipe", 48000)]


def strict_batch(sa, monkeypatch, family, builder, n_ch, **kw):
    if family != "generic":
        monkeypatch.setenv("SAME_PIPE", "1" if family == "pipe" else "0")          # read when the batch is created
    rx = builder.build_batch(n_ch, generic_kernel=(family == "generic"), **kw)
    name = rx.kernel_name()
    assert name.startswith("demod_kernel<") if family == "generic" else name == f"demod_{family}_kernel", name
    return rx


@pytest.mark.parametrize("family,rate", STRICT)
def test_strict_kernels_equal_the_oracle_on_every_channel(sa, ob, monkeypatch, family, rate):
    """All 256 channels, every class, stable or not, broken or not: every link event and burst byte, and the symbol trace of
    four channels per class bit for bit in all five fields."""
    import torch
    b = the_batch(rate)
    x = torch.from_numpy(b["x"]).cuda()
    cfg = ob.default_config(rate)
    rx = strict_batch(sa, monkeypatch, family, sa.SameReceiverBuilder(rate), x.shape[1], trace_symbols=True)
    rx.process_tensor(x)
    rx.sync()
    ev = rx.poll_events_np()
    n = assert_every_channel_matches_oracle(ob, cfg, x, ev)
    assert n > 3 * x.shape[1]                                           # (the stubs deliver little)
    assert_traces_equal_the_oracle(ob, cfg, rx, b["x"], traced_channels(b), f"{family} {rate}")
    print(f"IMPAIRED strict {rx.kernel_name()} {rate} Hz: {x.shape[1]} channels, {n} link events and {len(traced_channels(b))} traces equal the oracle's")


@pytest.mark.parametrize("form", ["i16", "channel_major", "odd_calls", "ragged"])
@pytest.mark.parametrize("family,rate", [("pipe", 22050), ("fast", 22050), ("generic", 48000), ("pipe", 48000)])
def test_strict_input_forms_equal_the_oracle(sa, ob, monkeypatch, family, rate, form):
    """The same batch as int16 after the saturating rounding (hum and DC of several carriers saturate), channel-major, in
    calls of 25 013 samples that cut through the bursts, and as two ragged calls the first of which ends inside the bursts:
    all equal the oracle fed the same samples."""
    import torch
    from test_ragged_calls import Feeder
    b = the_batch(rate)
    host = im.to_int16(b["x64"]) if form == "i16" else b["x"]
    T, n_ch = host.shape
    rx = strict_batch(sa, monkeypatch, family, sa.SameReceiverBuilder(rate), n_ch, trace_symbols=(form != "ragged"))
    if form == "i16":
        rx.process_tensor(torch.from_numpy(host).cuda())
    elif form == "channel_major":
        rx.process_tensor(torch.from_numpy(np.ascontiguousarray(host.T)).cuda(), layout=sa.LAYOUT_CHANNEL_MAJOR)
    elif form == "odd_calls":
        for off in range(0, T, 25013):
            rx.process_tensor(torch.from_numpy(host[off:off + 25013]).cuda())
    else:
        rng = np.random.default_rng(rate)
        first = rng.integers(int(0.2 * T), int(0.5 * T), n_ch).astype(np.uint32)      # the bursts span 0.12 .. 0.53 T
        feeder = Feeder(host)
        for counts in (first, (T - first).astype(np.uint32)):
            rows = int(counts.max())
            rx.process_ragged(torch.from_numpy(feeder.buffer(counts, rows, False)).cuda(), counts)
        assert all(rx.channel_input_sample_counter(c) == T for c in range(0, n_ch, 17))
    rx.sync()
    ev = ordered(rx.poll_events_np())
    as_f32 = torch.from_numpy(host.astype(np.float32)).cuda()
    cfg = ob.default_config(rate)
    n = assert_every_channel_matches_oracle(ob, cfg, as_f32, ev)
    if form != "ragged":
        assert_traces_equal_the_oracle(ob, cfg, rx, host.astype(np.float32), traced_channels(b)[::2], f"{family} {rate} {form}")
    print(f"IMPAIRED strict {rx.kernel_name()} {rate} Hz {form}: {n_ch} channels, {n} link events equal the oracle's")


@pytest.mark.parametrize("rate", [22050, 48000])
@pytest.mark.parametrize("name", ["samedec", "long_equalizer"])
def test_strict_other_configurations_equal_the_oracle(sa, ob, name, rate):
    """samedec's configuration (AGC gain between 1 / 32 767 and 1 / 200: the near-silent carriers hold the gain at its upper
    limit, the loud ones at its lower) and an equalizer of 8 + 3 taps with the timing clamp narrowed to 1 % skew (the channels
    of the skew class beyond it sit on the clamp: test_impairments_cpu.py) on the skew, echo, eq_echo and level classes."""
    import torch
    b = im.batch(rate, SEED, classes=("skew", "echo", "eq_echo", "level"))
    x = torch.from_numpy(b["x"]).cuda()
    builder, cfg = config(ob, rate, name, sa)
    rx = builder.build_batch(x.shape[1], trace_symbols=True)
    assert rx.kernel_name().startswith("demod_") and "relaxed" not in rx.kernel_name() and "sym" not in rx.kernel_name()
    if name == "long_equalizer":
        assert rx.kernel_name().startswith("demod_kernel<")
    rx.process_tensor(x)
    rx.sync()
    n = assert_every_channel_matches_oracle(ob, cfg, x, rx.poll_events_np())
    assert_traces_equal_the_oracle(ob, cfg, rx, b["x"], traced_channels(b), f"{name} {rate}")
    print(f"IMPAIRED strict {rx.kernel_name()} {rate} Hz {name}: {x.shape[1]} channels, {n} link events equal the oracle's")


@pytest.mark.parametrize("family", ["generic", "fast", "pipe"])
def test_strict_headers_longer_than_an_event(sa, ob, monkeypatch, family):
    """Headers of 289 .. 300 bytes: the burst's length is the true one and its first 288 bytes are kept, as the oracle has it."""
    import torch
    rate = 22050
    o = im.overlong_batch(rate, SEED)
    x = torch.from_numpy(o["x"]).cuda()
    rx = strict_batch(sa, monkeypatch, family, sa.SameReceiverBuilder(rate), x.shape[1])
    rx.process_tensor(x)
    rx.sync()
    ev = rx.poll_events_np()
    assert_every_channel_matches_oracle(ob, ob.default_config(rate), x, ev)
    bursts = ev[ev["kind"] == 3]
    assert len(bursts) == x.shape[1] and sorted(set(int(v) for v in bursts["len"]))[0] > im.EVENT_MAX_BYTES
    for r in bursts:
        assert r["bytes"].tobytes() == o["sent"][int(r["channel"])][:im.EVENT_MAX_BYTES]


# ------------------------------------------------------------------ relaxed: the existing contract on the stable channels
def only(ev, channels, n_ch):
    """the events of `channels`, renumbered 0 .. len(channels) - 1"""
    remap = np.full(n_ch, -1, dtype=np.int64)
    remap[channels] = np.arange(len(channels))
    e = ev[np.isin(ev["channel"], channels)].copy()
    e["channel"] = remap[e["channel"]].astype(np.uint32)
    return e


class Renumbered:
    """a receiver seen through a list of its channels (what test_relaxed.soft_symbol_differences reads of one)"""

    def __init__(self, rx, events, channels, n_ch, until=None):
        self.rx, self.events, self.channels, self.n_ch, self.until = rx, events, channels, n_ch, until

    def poll_events_np(self):
        return only(self.events, self.channels, self.n_ch)

    def read_trace(self, c, cap=4096):
        tr = self.rx.read_trace(int(self.channels[c]), cap=cap)
        return tr if self.until is None else tr[tr["sample_counter"] < self.until[int(self.channels[c])]]


def assert_relaxed_contract(sa, b, mask, got, ref, rate, n_ch, what, full=None, rel=None, classes=None, soft_limit=None):
    """Per admitted class: at least three quarters of its channels are stable and meet assert_contract(exact_bursts=True,
    garbled_per_mille=0) against strict mode; the unstable ones, and the class held by the strict tests only
    (impairments.STRICT_ONLY), must complete with ordered events.  full, rel: the strict and the relaxed receiver with symbol
    traces, for the soft symbols of the distortion classes -- while the carrier is there (up to a symbol before it stops: what
    follows is decoded from the hum or the tone alone) and up to impairments.SOFT_LIMIT (soft_limit: other limits for this
    case); beyond it the figure is printed."""
    from test_relaxed import soft_symbol_differences
    until = b["carrier_end"] - rate / im.BAUD
    for name in (classes or b["classes"]):
        ch = np.array([c for c in im.class_channels(b, name) if c < n_ch], dtype=np.int64)
        good = mask[ch] & (name in im.ADMITTED)
        stable, unstable = ch[good], ch[~good]
        if name in im.ADMITTED:
            assert 4 * len(stable) >= 3 * len(ch), f"{what} {name}: only {len(stable)} of {len(ch)} channels are stable"
        worst = assert_contract(sa, only(got, stable, n_ch), only(ref, stable, n_ch), rate, len(stable), lambda i: b["payload"][int(stable[i])],
                                exact_bursts=True, garbled_per_mille=0, what=f"{what} {name}")
        for c in unstable:
            t = got[got["channel"] == c]["sample_counter"].astype(np.int64)
            assert np.all(np.diff(t) >= 0), f"{what} {name} channel {c}: events out of order"
        soft = ""
        limits = dict(im.SOFT_LIMIT, **(soft_limit or {}))
        if full is not None and name in limits and len(stable):
            within = np.array([(b["amplitude"][c] >= im.SOFT_QUIET) if name == "level" else (b["severity"][c] <= limits[name] + 1e-9) for c in stable])
            for part, sel in (("", stable[within]), (" beyond the soft-symbol precondition (not asserted)", stable[~within])):
                if len(sel) == 0:
                    continue
                dt, err, flips, checked = soft_symbol_differences(Renumbered(full, ref, sel, n_ch, until), Renumbered(rel, got, sel, n_ch, until), len(sel), rate, every=1)
                soft += f", soft symbols of {checked} bursts{part}: worst |diff| {err.max():.4f}, {flips} sign differences, instants {dt.max()} samples apart"
                if not part:
                    assert checked >= len(sel) and flips == 0 and err.max() <= SOFT_SYMBOL_TOLERANCE, f"{what} {name}{soft}"
        print(f"IMPAIRED relaxed {what} {name}: compared {len(stable)} of {len(ch)} channels (unstable share {len(unstable) / len(ch):.3f}), "
              f"worst event-instant difference {max(worst.values())} samples {worst}{soft}")


def relaxed_pair(sa, x, rate, n_ch, builder_of, kernel, feed=None):
    """strict and relaxed receivers with symbol traces on the same input; returns (full, rel, ref events, got events)"""
    out = []
    for relaxed in (False, True):
        rx = builder_of().build_batch(n_ch, trace_symbols=True, relaxed=relaxed)
        (feed or (lambda r: r.process_tensor(x)))(rx)
        rx.sync()
        out.append((rx, ordered(rx.poll_events_np())))
    (full, ref), (rel, got) = out
    assert rel.kernel_name() == kernel, rel.kernel_name()
    assert "sym" not in full.kernel_name() and "relaxed" not in full.kernel_name() and "fastmath" not in full.kernel_name()
    return full, rel, ref, got


RELAXED = [("sym", 22050, 256), ("sym", 44100, 256), ("sym", 48000, 256),
           ("fastmath", 22050, 256), ("fastmath", 44100, 256), ("fastmath", 48000, 256),
           ("solo", 22050, 250), ("duo", 22050, 250)]            # 250: the last group of 64 is partly filled
RELAXED_KERNEL = {"sym": "demod_sym_kernel", "fastmath": "demod_pipe_kernel<fastmath>", "solo": "demod_relaxed_kernel", "duo": "demod_relaxed_kernel"}


def select_relaxed(monkeypatch, family):
    if family == "fastmath":
        monkeypatch.setenv("SAME_SYM", "0")
    elif family in ("solo", "duo"):
        monkeypatch.setenv("SAME_RELAXED_KERNEL", family)


@pytest.mark.parametrize("family,rate,n_ch", RELAXED)
def test_relaxed_kernels_meet_the_contract_on_the_stable_channels(sa, ob, monkeypatch, family, rate, n_ch):
    """The comparison is against strict mode on the same batch, which this test first holds to the oracle on every channel."""
    import torch
    select_relaxed(monkeypatch, family)
    b = the_batch(rate)
    x = torch.from_numpy(np.ascontiguousarray(b["x"][:, :n_ch])).cuda()
    full, rel, ref, got = relaxed_pair(sa, x, rate, n_ch, lambda: sa.SameReceiverBuilder(rate), RELAXED_KERNEL[family])
    assert_every_channel_matches_oracle(ob, ob.default_config(rate), x, ref)
    assert_relaxed_contract(sa, b, the_mask(ob, rate), got, ref, rate, n_ch, f"{rel.kernel_name()} {family} {rate} Hz", full, rel)


@pytest.mark.parametrize("family,rate,form", [("sym", 22050, "i16"), ("sym", 48000, "calls"), ("fastmath", 48000, "i16"), ("solo", 22050, "calls")])
def test_relaxed_input_forms_meet_the_contract(sa, ob, monkeypatch, family, rate, form):
    """int16 (the batch with the channels that would saturate -- DC and hum of several carriers -- scaled down to fit, so that
    every channel keeps its whole carrier; its own stability mask: the oracle on the rounded samples; the saturating form is
    held by the strict cases) and a split into calls that cut through the bursts."""
    import torch
    select_relaxed(monkeypatch, family)
    b = the_batch(rate)
    n_ch = b["x"].shape[1]
    if form == "i16":
        key = (rate, "fitted i16")
        if key not in _MASKS:
            fitted, amp = im.fit_int16(b["x64"], b["amplitude"])
            _MASKS[key] = (im.to_int16(fitted), im.stability_mask(ob, ob.default_config(rate), fitted, amp, SEED, quantize=im.to_int16))
        host, mask = _MASKS[key]
        assert np.abs(host.astype(np.int32)).max() < 32767
        x = torch.from_numpy(host).cuda()
        feed = None
    else:
        host = b["x"]
        x = torch.from_numpy(host).cuda()
        T = host.shape[0]
        cuts = [0, int(0.37 * T) + 11, int(0.37 * T) + 88, int(0.61 * T) + 5, T]
        feed = lambda r: [r.process_tensor(x[a:z].contiguous()) for a, z in zip(cuts[:-1], cuts[1:])]
        mask = the_mask(ob, rate)
    full, rel, ref, got = relaxed_pair(sa, x, rate, n_ch, lambda: sa.SameReceiverBuilder(rate), RELAXED_KERNEL[family], feed)
    assert_every_channel_matches_oracle(ob, ob.default_config(rate), torch.from_numpy(host.astype(np.float32)).cuda(), ref)
    assert_relaxed_contract(sa, b, mask, got, ref, rate, n_ch, f"{rel.kernel_name()} {family} {rate} Hz {form}", full, rel)


@pytest.mark.parametrize("family,rate", [("sym", 22050), ("sym", 48000), ("fastmath", 44100), ("solo", 22050)])
def test_relaxed_kernels_at_the_timing_clamp(sa, ob, monkeypatch, family, rate):
    """with_timing_max_deviation(0.005): the timing loop's averaged period is clamped at 1 % skew, and the skew class runs to
    1.5 %, so its upper channels sit on the clamp for dozens of symbols of their header (test_impairments_cpu.py); the detune,
    echo and tone classes ride along.  The stability mask is the oracle's under this configuration.  Bursts and link events
    are held on the whole skew class; its soft symbols up to 0.94 % skew (impairments.SOFT_SKEW_NARROW): measured, they stay
    within 0.05 up to 1.41 % and reach 0.16 at 1.5 %, where the loop cannot follow the clock any more, so no level with the
    1.5 x margin lies beyond the clamp.  The clamp itself is therefore held only indirectly in relaxed arithmetic: by the
    bytes and the +/- 2 symbols of the channels that sit on it."""
    import torch
    select_relaxed(monkeypatch, family)
    b = the_batch(rate)
    n_ch = b["x"].shape[1]
    x = torch.from_numpy(b["x"]).cuda()
    cfg = config(ob, rate, "narrow")[1]
    full, rel, ref, got = relaxed_pair(sa, x, rate, n_ch, lambda: config(ob, rate, "narrow", sa)[0], RELAXED_KERNEL[family])
    assert_every_channel_matches_oracle(ob, cfg, x, ref)
    assert_relaxed_contract(sa, b, the_mask(ob, rate, narrow=True), got, ref, rate, n_ch, f"{rel.kernel_name()} {family} {rate} Hz narrow clamp", full, rel,
                            classes=("skew", "detune", "echo", "tone"), soft_limit={"skew": im.SOFT_SKEW_NARROW})


# ------------------------------------------------------------------ time-parallel
TP_BLOCKS = ("dc", "hum", "echo", "clip", "fade", "level_step")


def distorted_workload(sa, n_ch, n, rate, seed):
    """synth_afsk's workload brought to the host and distorted by channel block at the classes' test levels, the severity
    spread over each block; the carrier of a channel is the largest sample of its clean stream"""
    x = sa.synth_afsk(n_ch, n, rate, seed=seed).cpu().numpy().astype(np.float64)
    amp = np.abs(x).max(axis=0)
    rng = np.random.default_rng([SEED, seed])
    per = -(-n_ch // len(TP_BLOCKS))
    for k, name in enumerate(TP_BLOCKS):
        ch = np.arange(k * per, min((k + 1) * per, n_ch))
        m = len(ch)
        sev = (np.arange(m) + 1.0) / m * im.LEVELS[name]
        sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
        frac = rng.uniform(0.0, 1.0, m)
        xb = x[:, ch]
        if name == "dc":
            xb = im.dc_step(xb, sev * amp[ch] * sign, np.where(np.arange(m) % 2 == 0, 0.0, (0.2 + 0.6 * frac) * n))
        elif name == "hum":
            xb = im.hum(xb, rate, np.where(np.arange(m) % 2 == 0, 50.0, 60.0), sev * amp[ch], 2.0 * np.pi * frac)
        elif name == "echo":
            xb = im.echo(xb, np.maximum(np.rint((0.25e-3 + 0.8e-3 * frac) * rate), 1), sev * sign)
        elif name == "clip":
            xb = im.clip(xb, amp[ch] / (1.0 + sev))
        elif name == "fade":
            xb = im.fade(xb, rate, sev, 3.0, 2.0 * np.pi * frac)
        else:
            xb = im.level_step(xb, 2.0 ** (sev * sign), (0.2 + 0.6 * frac) * n)
        x[:, ch] = xb
    return x.astype(np.float32)


@pytest.mark.parametrize("layout", ["channel_major", "time_major"])
def test_time_parallel_on_a_distorted_workload(sa, ob, monkeypatch, layout):
    """256 channels x 8 s at 22.05 kHz with DC offsets and steps, hum, echoes, clipping, fades and level steps, cut into at least
    four chunks per channel: does a chunk that starts one warm-up before its samples settle under hum and offset?  Strict mode
    is held to the oracle on every channel, the time-parallel receiver to strict mode under the contract, as
    test_time_parallel_meets_the_contract does."""
    import torch
    monkeypatch.setenv("SAME_PIPE_LANES", "64")          # (small test batches would otherwise get 16-channel workgroups)
    rate, n_ch, seed = 22050, 256, 4242
    n = 8 * rate
    n -= n % 1260
    x = torch.from_numpy(distorted_workload(sa, n_ch, n, rate, seed)).cuda()
    ref = strict_events(sa, x, rate)
    assert_every_channel_matches_oracle(ob, ob.default_config(rate), x, ref)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=6)
    if layout == "channel_major":
        rx.process_tensor(x.t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
    else:
        rx.process_tensor(x)
    rx.sync()
    assert rx.time_parallel_chunks() >= 4 and rx.kernel_name() == "demod_sym_kernel"
    got = ordered(rx.poll_events_np())
    assert len(ref[ref["kind"] == 3]) >= n_ch
    host = x.cpu().numpy()
    amp = np.abs(sa.synth_afsk(n_ch, n, rate, seed=seed).cpu().numpy()).max(axis=0)
    key = ("time-parallel", seed)
    if key not in _MASKS:
        _MASKS[key] = im.stability_mask(ob, ob.default_config(rate), host, amp, SEED)
    per = -(-n_ch // len(TP_BLOCKS))
    for k, name in enumerate(TP_BLOCKS):
        block = np.arange(k * per, min((k + 1) * per, n_ch))
        ch = block[_MASKS[key][block]]
        if name not in im.STRICT_ONLY:
            assert 4 * len(ch) >= 3 * len(block), f"time-parallel {name}: only {len(ch)} of {len(block)} channels are stable"
        worst = assert_contract(sa, only(got, ch, n_ch), only(ref, ch, n_ch), rate, len(ch), lambda i: sa.synth_payload(seed, int(ch[i])),
                                exact_bursts=True, garbled_per_mille=0, what=f"time-parallel {layout} {name}", t_end=n)
        print(f"IMPAIRED time-parallel {rx.kernel_name()} {layout} {rx.time_parallel_chunks()} chunks {name}: compared {len(ch)} of {len(block)} channels, "
              f"worst event-instant difference {max(worst.values())} samples {worst}")
