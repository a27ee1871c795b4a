"""The distorted and broken batches of tests/helpers/impairments.py, on the oracle alone (no GPU).

tests/test_under_impairments_gpu.py holds every kernel family to the oracle on these batches.  That only means something if the oracle
itself copes with them, decides them the same way when the samples move a little, and is driven out of its trivial regime by
them; this module measures all three at 22.05, 44.1 and 48 kHz for the committed seed:

  (a) decode margin     every distortion class decodes to the transmitted header on all of its channels at its test level and
                        at 1.5 times it;
  (b) stability mask    at most a quarter of a class's channels change their bursts under three perturbations of 1 % of the
                        carrier (fifteen classes meet the cap, broken ones included, and are admitted to the relaxed tests;
                        level_step does not and is held by the strict tests only);
  (c) each class bites  see test_each_class_reaches_its_stage; what the oracle does NOT do is written there too;
  (d) determinism       the same arguments give the same bits, and float32 rounding happens once, at the end.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import impairments as im

SEED = 2026
RATES = (22050, 44100, 48000)


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    binding.lib()
    return binding


_WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def release_worlds():
    """the batches are shared by the tests of this module and dropped with it"""
    yield
    _WORLDS.clear()


@pytest.fixture(params=RATES)
def world(request, ob):
    """per rate, computed once: the batch, the same bursts undistorted, and the oracle's events on both"""
    rate = request.param
    if rate not in _WORLDS:
        cfg = ob.default_config(rate)
        b = im.batch(rate, SEED)
        clean = im.batch(rate, SEED, distorted=False)
        _WORLDS[rate] = dict(rate=rate, cfg=cfg, b=b, clean=clean, ev=im.oracle_bursts(ob, cfg, b["x"]),
                             ev_clean=im.oracle_bursts(ob, cfg, clean["x"]))
    return _WORLDS[rate]


def delivered(events, payload):
    bursts = im.bursts_of(events)
    return len(payload) > 0 and len(bursts) >= 1 and bursts[0][:len(payload)] == payload


def test_decode_margin(world, ob):
    """(a) At the test level and at MARGIN times it the oracle delivers the whole header on every channel of every
    distortion class (and exactly one burst: nothing is split in two)."""
    b, rate = world["b"], world["rate"]
    hard = im.batch(rate, SEED, scale=im.MARGIN, classes=im.DISTORTIONS)
    ev_hard = im.oracle_bursts(ob, world["cfg"], hard["x"])
    for name in im.DISTORTIONS:
        lost = [c for c in im.class_channels(b, name) if not delivered(world["ev"][c], b["payload"][c]) or len(im.bursts_of(world["ev"][c])) != 1]
        assert not lost, f"{rate} Hz, {name} at its test level: channels {lost}"
        lost = [c for c in im.class_channels(hard, name) if not delivered(ev_hard[c], hard["payload"][c])]
        assert not lost, f"{rate} Hz, {name} at {im.MARGIN} x its test level: channels {lost}"
        assert [hard["payload"][c] for c in im.class_channels(hard, name)] == [b["payload"][c] for c in im.class_channels(b, name)]


def test_stability_mask(world, ob):
    """(b) The cap is a condition on the classes' parameters: at most MAX_UNSTABLE_SHARE of a class may change its bursts, or
    move the instants of their link events by more than a symbol, under the perturbations (tuned until the oracle alone met
    it: dropouts of at least three bytes, cuts away from the byte edges, equalizer-decided echoes that survived nine
    perturbations when they were searched for).  level_step could not be tuned to it (impairments.STRICT_ONLY: 19 .. 37 %
    unstable) and is held by the strict tests only.  Printed per class, since the GPU
    tests' coverage follows from it."""
    b, rate = world["b"], world["rate"]
    mask = im.stability_mask(ob, world["cfg"], b["x64"], b["amplitude"], SEED, base=world["ev"])
    share = {name: 1.0 - float(np.mean(mask[list(im.class_channels(b, name))])) for name in im.CLASSES}
    print(f"{rate} Hz, unstable share per class:", {k: round(v, 3) for k, v in share.items()})
    for name in im.ADMITTED:
        assert share[name] <= im.MAX_UNSTABLE_SHARE, f"{rate} Hz, {name}: {share[name]:.2f} of the channels are unstable"
    assert set(im.STRICT_ONLY) | set(im.ADMITTED) == set(im.CLASSES) and im.STRICT_ONLY == ("level_step",)
    # the mask is a function of the samples and the seed
    if rate == RATES[0]:
        assert np.array_equal(im.stability_mask(ob, world["cfg"], b["x64"], b["amplitude"], SEED, base=world["ev"]), mask)


def period_avg_at_clamp(ob, cfg, x):
    """Symbols between Reading and Burst at which the timing loop's averaged period sits on its clamp.  The trace has
    next = period_avg + alpha err + offset at every symbol; the offset is what the two waits since the previous symbol left
    over: 2 next[k-1] less the samples that passed (rx/symsync.rs advance: the TED between two symbols adds its own
    remainder to the same period).  Returns (symbols at the clamp, symbols looked at, header delivered?)."""
    d = ob.derive(cfg)
    rx = ob.Receiver(cfg)
    rx.enable_trace(4096)
    ev = [e.as_tuple() for e in rx.run(np.ascontiguousarray(x))]
    tr = rx.trace()
    t_read = [t for k, t, _ in ev if k == 2]
    t_burst = [t for k, t, _ in ev if k == 3]
    if not t_read or not t_burst:
        return 0, 0, ev
    idx = np.flatnonzero((tr["sample_counter"] > t_read[0]) & (tr["sample_counter"] < t_burst[0]))
    nxt, err, sc = tr["next"].astype(np.float64), tr["err"].astype(np.float64), tr["sample_counter"].astype(np.int64)
    avg = nxt[idx] - d.alpha_locked * err[idx] - (2.0 * nxt[idx - 1] - (sc[idx] - sc[idx - 1]))
    at = (np.abs(avg - d.period_max) < 1e-3) | (np.abs(avg - d.period_min) < 1e-3)
    return int(at.sum()), len(idx), ev


def test_each_class_reaches_its_stage(world, ob):
    """(c) What each class does to the oracle, so that "the kernel equals the oracle" is a statement about the stage the class
    is aimed at.

    Every class: the event sample counters differ from those of the same bursts undistorted on at least three quarters of
    the channels (the mildest channels of a block may leave them where they were).
    cut, dropout: the burst is shorter than the header.  back_to_back: an extra NoCarrier and a second burst.
    invalid_bytes: the channels with seven bad bytes end their burst at the sixth; those with up to five deliver all of them.
    stub: no burst at all.  level: the near-silent carriers (5 .. 40 against the usual 2 000 .. 30 000) are decoded -- no
    more than that: the default AGC has no gain limit within reach (it climbs from 0 by its bandwidth per sample towards 1e6), so
    nothing here shows an AGC at a limit; only the samedec() case of the GPU tests, with gains held between 1 / 32 767 and
    1 / 200, exercises the AGC's gain limits.
    skew: measured, not assumed -- the clamp of the DEFAULT configuration (timing_max_deviation 0.01 of a symbol, which is
    2 % of the half-symbol period the loop steers) is never reached: the oracle loses headers from 2.4 .. 2.85 % skew on at
    44.1 / 48 kHz, so no level with a 1.5 x margin gets there, and the averaged period stays inside its limits on every
    channel.  With the clamp narrowed to 1 % (with_timing_max_deviation(0.005)) the channels beyond 1.2 % skew sit on it for
    at least 16 symbols of their header -- not in one run: the loop bounces off the limit -- and still decode; that
    configuration is what the GPU tests use to hold the clamp.
    echo: measured as well -- at no echo level with a 1.5 x margin does the oracle with its equalizer disabled lose a header
    the default keeps; what the equalizer changes there is the bytes decoded behind the carrier (with it disabled the
    delivered bursts differ on at least three quarters of the channels), so its taps have moved.
    eq_echo: the class where the equalizer decides TRANSMITTED bytes -- on every channel that has an entry in
    impairments.EQ_ECHOES (at least twelve of the sixteen per rate) the default configuration delivers the whole header and
    the oracle with the equalizer disabled does not.  About two in a hundred strong echoes are of that kind and a fraction of
    those is stable; the entries were searched for, channel by channel, among 1 200 .. 4 800 candidates."""
    b, rate, ev, ev0 = world["b"], world["rate"], world["ev"], world["ev_clean"]
    n = b["n_per_class"]
    for name in im.CLASSES:
        moved = [c for c in im.class_channels(b, name) if [t for _, t, _ in ev[c]] != [t for _, t, _ in ev0[c]]]
        assert len(moved) >= 3 * n // 4, f"{rate} Hz, {name}: the event instants moved on {len(moved)} channels only"
    for c in im.class_channels(b, "stub"):
        assert not im.bursts_of(ev[c]) and len(im.bursts_of(ev0[c])) == 1
    for name in ("cut", "dropout"):
        for c in im.class_channels(b, name):
            bursts = im.bursts_of(ev[c])
            assert len(bursts) == 1 and len(bursts[0]) < len(b["sent"][c]) and delivered(ev[c], b["payload"][c]), (name, c)
    for c in im.class_channels(b, "back_to_back"):
        assert len(im.bursts_of(ev[c])) == 2 and sum(k == 0 for k, _, _ in ev[c]) == sum(k == 0 for k, _, _ in ev0[c]) + 1
        assert delivered(ev[c], b["payload"][c])
    first = im.class_channels(b, "invalid_bytes")[0]
    for c in im.class_channels(b, "invalid_bytes"):
        burst = im.bursts_of(ev[c])[0]
        if (c - first) % 4 == 3:
            assert burst == b["payload"][c] and len(burst) < len(b["sent"][c]), c          # ended by the framer, nothing behind it
        else:
            assert burst[:len(b["sent"][c])] == b["sent"][c], c
    level = list(im.class_channels(b, "level"))
    for c in level[:n // 2]:
        assert b["amplitude"][c] <= 40.0 and delivered(ev[c], b["payload"][c])
    assert max(b["amplitude"][level]) == im.LOUD

    skew = list(im.class_channels(b, "skew"))
    for c in skew:
        assert period_avg_at_clamp(ob, world["cfg"], b["x"][:, c])[0] == 0, c
    narrow = ob.default_config(rate)
    ob.lib().so_config_with_timing_max_deviation(C.byref(narrow), im.NARROW_CLAMP)
    for c in skew:
        at, looked, e = period_avg_at_clamp(ob, narrow, b["x"][:, c])
        assert delivered(e, b["payload"][c]), c
        if b["severity"][c] * im.LEVELS["skew"] >= 0.012:
            assert looked > 300 and at >= 16, f"{rate} Hz, channel {c}: {at} of {looked} symbols at the clamp"

    without = ob.default_config(rate)
    ob.lib().so_config_without_adaptive_equalizer(C.byref(without))
    ch = list(im.class_channels(b, "echo"))
    ev_w = im.oracle_bursts(ob, without, b["x"][:, ch])
    assert all(delivered(ev[c], b["payload"][c]) and delivered(ev_w[i], b["payload"][c]) for i, c in enumerate(ch))
    assert sum(im.bursts_of(ev_w[i]) != im.bursts_of(ev[c]) for i, c in enumerate(ch)) >= 3 * n // 4
    ch = list(im.class_channels(b, "eq_echo"))
    ev_w = im.oracle_bursts(ob, without, b["x"][:, ch])
    table = im.EQ_ECHOES[(rate, SEED)]
    decided = [c for i, c in enumerate(ch) if table[i] is not None]
    assert len(decided) >= 3 * n // 4
    for i, c in enumerate(ch):
        if table[i] is not None:
            assert delivered(ev[c], b["payload"][c]) and len(im.bursts_of(ev[c])) == 1, f"{rate} Hz eq_echo channel {i}: the default configuration loses the header"
            assert not delivered(ev_w[i], b["payload"][c]), f"{rate} Hz eq_echo channel {i}: the header survives without the equalizer"


def test_what_an_error_in_the_equalizer_update_can_show(world, ob):
    """How wrong the NLMS update has to be before the REFERENCE's transmitted bytes change, on the two echo classes: with the
    relaxation at half or twice its value (0.05) the oracle delivers the same payload on every stable channel -- an update
    that is off by such a factor is invisible to any contract stated in bytes, in the oracle as in a kernel --, with the
    update dead (relaxation 0) it loses at least half of the eq_echo class, and with eight times the relaxation at least
    a quarter of it.  The eq_echo class is what holds the relaxed kernels' equalizer, against errors of that size."""
    b, rate = world["b"], world["rate"]
    ch = list(im.class_channels(b, "echo")) + list(im.class_channels(b, "eq_echo"))
    x64, amp = b["x64"][:, ch], b["amplitude"][ch]
    base = im.oracle_bursts(ob, world["cfg"], x64.astype(np.float32))
    assert [e for e in base] == [world["ev"][c] for c in ch]
    stable = im.stability_mask(ob, world["cfg"], x64, amp, SEED, base=base)
    changed = {}
    for factor in (0.0, 0.5, 2.0, 8.0):
        cfg = ob.default_config(rate)
        ob.lib().so_config_with_adaptive_equalizer(C.byref(cfg), 6, 4, 0.05 * factor, 1.0e-6)
        ev = im.oracle_bursts(ob, cfg, x64.astype(np.float32))
        changed[factor] = [i for i, c in enumerate(ch) if stable[i] and delivered(ev[i], b["payload"][c]) != delivered(base[i], b["payload"][c])]
    print(f"{rate} Hz, stable echo channels whose payload changes with the relaxation:", {k: len(v) for k, v in changed.items()})
    assert not changed[0.5] and not changed[2.0]
    assert all(i >= 16 for i in changed[0.0] + changed[8.0])                   # the echo class with a margin never reacts
    assert len(changed[0.0]) >= 8 and len(changed[8.0]) >= 4


def test_the_helper_is_deterministic_and_rounds_once(world):
    """(d) Same arguments, same bits; x is the float32 rounding of x64 and of nothing else; a class's channels do not depend on
    which other classes are in the batch; int16 rounding saturates."""
    b, rate = world["b"], world["rate"]
    again = im.batch(rate, SEED)
    assert np.array_equal(again["x64"], b["x64"]) and again["x"].dtype == np.float32
    assert np.array_equal(b["x"], b["x64"].astype(np.float32))
    assert again["payload"] == b["payload"] and again["cls"] == b["cls"] and np.array_equal(again["severity"], b["severity"])
    assert b["x"].shape == (im.n_samples(rate), im.N_CLASSES * 16) and b["x"].shape[1] % 64 == 0
    alone = im.batch(rate, SEED, classes=("echo", "cut"))
    assert np.array_equal(alone["x64"][:, :16], b["x64"][:, list(im.class_channels(b, "echo"))])
    assert np.array_equal(alone["x64"][:, 16:], b["x64"][:, list(im.class_channels(b, "cut"))])
    assert not np.array_equal(im.batch(rate, SEED + 1, classes=("echo",))["x64"], alone["x64"][:, :16])
    for name in im.CLASSES:
        sev = b["severity"][list(im.class_channels(b, name))]
        assert np.allclose(sev, (np.arange(16) + 1) / 16.0)                # mild to the test level
    i16 = im.to_int16(b["x64"])
    assert i16.dtype == np.int16 and i16.max() == 32767 and i16.min() == -32768          # (hum and DC of several carriers)
    inside = np.abs(b["x64"]) < 32767.0
    assert np.array_equal(i16[inside], np.rint(b["x64"][inside]).astype(np.int16))


def test_the_modulator_against_its_definition():
    """An independent look at modulate(): tone frequencies by counting zero crossings over whole bytes of ones and of zeros,
    the symbol clock from the burst's length, continuity of the phase, skew and detune as the stated factors."""
    rate, T = 48000, 48000
    for data, hz in ((b"\xff" * 20, im.MARK_HZ), (b"\x00" * 20, im.SPACE_HZ)):
        for detune in (0.0, 0.04):
            x = im.modulate(data, rate, T, 1.0, detune=detune, lead=0.1, preamble=False)
            on = np.flatnonzero(x != 0.0)
            seconds = (on[-1] - on[0]) / rate
            crossings = np.sum(np.signbit(x[on[0]:on[-1]][1:]) != np.signbit(x[on[0]:on[-1]][:-1]))
            assert abs(crossings / (2.0 * seconds) - hz * (1.0 + detune)) < 2.0 / seconds, (hz, detune)
            assert abs(seconds - 160 / im.BAUD) < 2.0 / rate
    for skew in (-0.02, 0.0, 0.02):
        x = im.modulate(b"ZCZC-TEST", rate, T, 1000.0, skew=skew, lead=0.1)
        on = np.flatnonzero(x != 0.0)
        assert abs((on[-1] - on[0]) / rate - 8 * 25 / (im.BAUD * (1.0 + skew))) < 3.0 / rate
        # continuous phase: no sample-to-sample jump larger than the faster tone can make
        assert np.abs(np.diff(x[on[0]:on[-1] + 1])).max() <= 1000.0 * 2.0 * np.pi * im.MARK_HZ / rate * 1.001
    # least significant bit first: 0x01 is one mark symbol followed by seven space symbols
    x = im.modulate(b"\x01", rate, T, 1.0, lead=0.1, preamble=False)
    sps = im.samples_per_symbol(rate)
    first = int(0.1 * rate)
    spectrum = lambda seg, hz: abs(np.sum(seg * np.exp(-2j * np.pi * hz / rate * np.arange(len(seg)))))
    one, rest = x[first + 2:first + int(sps) - 2], x[first + int(sps) + 2:first + int(8 * sps) - 2]
    assert spectrum(one, im.MARK_HZ) > 3 * spectrum(one, im.SPACE_HZ) and spectrum(rest, im.SPACE_HZ) > 3 * spectrum(rest, im.MARK_HZ)


def test_the_distortions_do_what_they_say():
    rate = 22050
    x = np.stack([im.modulate(b"ZCZC", rate, 8000, 1000.0, lead=0.05), im.modulate(b"NNNN", rate, 8000, 500.0, lead=0.06)], axis=1)
    assert np.allclose(im.dc_offset(x, [10.0, -5.0]) - x, np.broadcast_to([10.0, -5.0], x.shape), atol=1e-9, rtol=0)
    step = im.dc_step(np.zeros_like(x), [7.0, 9.0], [100, 4000])
    assert step[99, 0] == 0.0 and step[100, 0] == 7.0 and step[3999, 1] == 0.0 and step[4000, 1] == 9.0
    h = im.hum(np.zeros((rate, 2)), rate, [50.0, 60.0], [2.0, 3.0])
    assert abs(np.abs(h[:, 0]).max() - 2.0) < 1e-3 and abs(np.abs(h[:, 1]).max() - 3.0) < 1e-3
    assert np.sum(np.signbit(h[1:, 0]) != np.signbit(h[:-1, 0])) in (99, 100) and np.sum(np.signbit(h[1:, 1]) != np.signbit(h[:-1, 1])) in (119, 120)
    e = im.echo(x, [3, 11], [0.5, -0.7])
    assert np.allclose(e[3:, 0], x[3:, 0] + 0.5 * x[:-3, 0]) and np.allclose(e[11:, 1], x[11:, 1] - 0.7 * x[:-11, 1]) and np.array_equal(e[:3, 0], x[:3, 0])
    c = im.clip(x, [300.0, 100.0])
    assert c[:, 0].max() == 300.0 and c[:, 0].min() == -300.0 and c[:, 1].max() == 100.0 and np.array_equal(c[np.abs(x) < 100.0], x[np.abs(x) < 100.0])
    assert np.array_equal(im.to_int16(np.array([0.5, 1.5, -0.5, 2.5, 40000.0, -40000.0, 32767.4, -32768.6])), np.array([0, 2, 0, 2, 32767, -32768, 32767, -32768], np.int16))
    f = im.fade(np.ones((rate, 1)), rate, 0.6, freq=3.0)
    assert abs(f.max() - 1.0) < 1e-6 and abs(f.min() - 0.4) < 1e-4
    s = im.level_step(x, [4.0, 0.25], [2000, 3000])
    assert np.array_equal(s[:2000, 0], x[:2000, 0]) and np.array_equal(s[2000:, 0], 4.0 * x[2000:, 0]) and np.array_equal(s[3000:, 1], 0.25 * x[3000:, 1])
    k = im.cut(x, [2500.5, 0.0])
    assert np.array_equal(k[:2501, 0], x[:2501, 0]) and not k[2501:, 0].any() and not k[:, 1].any()
    d = im.dropout(x, [2000, 3000], [100, 50])
    assert not d[2000:2100, 0].any() and np.array_equal(d[2100:, 0], x[2100:, 0]) and np.array_equal(d[:2000, 0], x[:2000, 0]) and not d[3000:3050, 1].any()


def test_overlong_headers(ob):
    """Headers of 289 .. 300 bytes: the oracle reports the burst's true length and keeps its first 288 bytes."""
    rate = 22050
    o = im.overlong_batch(rate, SEED, n_channels=12)
    ev = im.oracle_bursts(ob, ob.default_config(rate), o["x"])
    for c in range(12):
        assert 289 <= len(o["sent"][c]) <= 300 and len(set(len(s) for s in o["sent"])) == 12
        bursts = im.bursts_of(ev[c])
        assert len(bursts) == 1 and bursts[0] == o["sent"][c][:im.EVENT_MAX_BYTES], c
