"""Time-parallel ("fast") mode, SAME_BATCH_TIME_PARALLEL: the parity contract of include/same_rx.h.

The mode approximates the state a chunk starts from (a freshly built receiver one warm-up before the samples it
owns) and, by default, runs the chunks in relaxed arithmetic (the pipeline's FASTMATH build: fused multiply-add
partial sums in the matched filters, f32 square root, two-operation AGC chain, SAME_BATCH_RELAXED's contract);
SAME_RELAXED=0 keeps every chunk's arithmetic strict.  EVERY test of this module runs both ways (the `arith`
fixture).  Against the oracle on the same samples:
  * bursts: their number and order per channel and every transmitted byte (the header, or NNNN): EQUAL.
    The up to frame_max_invalid + 1 bytes a burst carries after them are decoded from the silence that
    follows the carrier and depend on the symbol clock's phase to the sample; they are not compared
    (the transport layer never votes on them either: rx/combiner.rs truncates at the header's end);
  * transport messages (header text, end-of-message), their number and order: EQUAL;
  * link events of every delivered burst -- Reading, Burst, the NoCarrier after it -- within
    TP_EVENT_TOLERANCE_SYMBOLS symbols of the reference's sample counter, its Searching anywhere inside
    the preamble.  Acquisitions that never reach Reading (a Searching / NoCarrier pair) may differ;
  * soft symbols of an open squelch: instants within SOFT_INSTANT_TOLERANCE samples, values within
    SOFT_SYMBOL_TOLERANCE with equal sign;
  * noisy input, where the reference itself drops a burst now and then and which one is chaotic: bursts
    both deliver are equal as above, the number of unmatched bursts is bounded, BER tallies are
    statistically equal.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SOFT_SYMBOL_TOLERANCE = 0.05
SOFT_INSTANT_TOLERANCE = 8       # samples (a fifth of a symbol at 22.05 kHz; measured: max 6, mean 0.9)


@pytest.fixture(autouse=True, params=["fastmath", "strict"])
def arith(request, monkeypatch):
    """The arithmetic inside the chunks: the default (relaxed: the pipeline's FASTMATH build wherever the batch is
    whole 64-channel workgroups at 22.05 / 44.1 / 48 kHz) or strict (SAME_RELAXED=0); read when a batch is created."""
    if request.param == "strict":
        monkeypatch.setenv("SAME_RELAXED", "0")
    else:
        monkeypatch.delenv("SAME_RELAXED", raising=False)
    return request.param


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


def split(ev, n_ch):
    first = np.searchsorted(ev["channel"], np.arange(n_ch + 1))
    return [ev[first[c]:first[c + 1]] for c in range(n_ch)]


def burst_list(e):
    b = e[e["kind"] == 3]
    return [r["bytes"][: min(int(r["len"]), 288)].tobytes() for r in b]


def message_list(e):
    m = e[e["kind"] >= 18]
    return [(int(r["kind"]), r["bytes"][: min(int(r["len"]), 288)].tobytes()) for r in m]


def burst_records(e):
    """Per delivered burst: (t_searching, t_reading, t_burst, t_no_carrier_after, bytes) -- the acquisition
    that led to it (last Searching before its Reading), leaving failed acquisitions out."""
    out, t_s, t_r = [], None, None
    link = e[e["kind"] <= 3]
    for i, r in enumerate(link):
        k, t = int(r["kind"]), int(r["sample_counter"])
        if k == 1:
            t_s = t
        elif k == 2:
            t_r = t
        elif k == 3:
            t_n = int(link[i + 1]["sample_counter"]) if i + 1 < len(link) and link[i + 1]["kind"] == 0 else None
            out.append((t_s, t_r, t, t_n, r["bytes"][: min(int(r["len"]), 288)].tobytes()))
            t_s = t_r = None
    return out


def payload_len(burst, payload):
    """Bytes of a burst that were transmitted: the header (or NNNN).  What follows is decoded from the
    silence after the carrier stops -- up to frame_max_invalid + 1 bytes -- and depends on the symbol
    clock's phase to the sample."""
    return len(payload) if burst[:4] == payload[:4] else 4


def assert_contract(sa, got, ref, rate, n_ch, payload_of, exact_bursts=True, what="", t_end=None, garbled_per_mille=0):
    """got / ref: event arrays (kind, channel, sample_counter, len, bytes) ordered by channel then time;
    ref from the oracle or from a strict batch.  payload_of(c) = what channel c transmits.
    garbled_per_mille: bursts per thousand (at least one) whose transmitted bytes may differ -- 0 except for relaxed
    arithmetic on NOISY input, where a marginal acquisition now and then goes the other way (measured: 1-2 in 22 000 bursts
    at noise sigma 0.05-0.1, tools/noise_probe.py; strict mode loses 2-10 bursts in the same runs)."""
    sps = rate / 520.83
    tol = sa.receiver.TP_EVENT_TOLERANCE_SYMBOLS * sps
    g, r = split(got, n_ch), split(ref, n_ch)
    worst = {"reading": 0, "burst": 0, "no_carrier": 0, "searching": 0}
    n_bursts = n_missing = n_garbled = 0
    for c in range(n_ch):
        pay = payload_of(c)
        bg, br = burst_records(g[c]), burst_records(r[c])
        if t_end is not None:
            # a burst that ends within the event tolerance of the end of the input is reported by one mode in this call
            # and by the other in the next
            bg = [x for x in bg if x[2] <= t_end - 2 * tol]
            br = [x for x in br if x[2] <= t_end - 2 * tol]
            # (... and one within the tolerance of THAT limit may fall on either side of it in the two modes)
            while len(bg) > len(br) and bg[-1][2] > t_end - 3 * tol:
                bg.pop()
            while len(br) > len(bg) and br[-1][2] > t_end - 3 * tol:
                br.pop()
        n_bursts += len(br)
        if exact_bursts:
            assert len(bg) == len(br), f"{what} channel {c}: {len(bg)} bursts, reference {len(br)}"
            if t_end is None or not any(int(e["sample_counter"]) > t_end - 8 * tol for e in list(g[c][g[c]["kind"] >= 18]) + list(r[c][r[c]["kind"] >= 18])):
                assert message_list(g[c]) == message_list(r[c]), f"{what} channel {c}: transport messages differ"
            pairs = list(zip(bg, br))
        else:
            # noisy input: the reference itself misses a burst now and then (an early false sync inside the
            # preamble), and which ones is chaotic; match bursts by time and count the unmatched
            pairs, j = [], 0
            for x in br:
                while j < len(bg) and bg[j][2] < x[2] - 4 * sps:
                    j += 1; n_missing += 1
                if j < len(bg) and abs(bg[j][2] - x[2]) <= 4 * sps:
                    pairs.append((bg[j], x)); j += 1
                else:
                    n_missing += 1
            n_missing += len(bg) - j
        for x, y in pairs:
            n = payload_len(y[4], pay)
            if x[4][:n] != y[4][:n]:
                n_garbled += 1
                assert garbled_per_mille, f"{what} channel {c}: burst payload differs: {x[4]!r} vs {y[4]!r}"
                continue
            for name, i in (("reading", 1), ("burst", 2), ("no_carrier", 3)):
                if x[i] is not None and y[i] is not None:
                    d = abs(x[i] - y[i])
                    worst[name] = max(worst[name], d)
                    assert d <= tol, f"{what} channel {c}: {name} {d} samples off (tolerance {tol:.0f})"
            if x[0] is not None and y[0] is not None:
                d = abs(x[0] - y[0])
                worst["searching"] = max(worst["searching"], d)
                assert d <= 16 * 8 * sps, f"{what} channel {c}: Searching outside the preamble"
    if not exact_bursts:
        assert n_missing <= max(4, n_bursts // 25), f"{what}: {n_missing} of {n_bursts} bursts unmatched"
    assert n_garbled <= max(1, n_bursts * garbled_per_mille // 1000) * (1 if garbled_per_mille else 0), f"{what}: {n_garbled} of {n_bursts} payloads differ"
    return worst


def strict_events(sa, x, rate, builder=None, link_only=False):
    n_ch = x.shape[1]
    rx = (builder or sa.SameReceiverBuilder(rate)).build_batch(n_ch, link_only=link_only)
    rx.process_tensor(x)
    rx.sync()
    return rx.poll_events_np()


def cases(rows, n_old):
    """The first n_old rows keep the ids they had before the `sym` column (SAME_SYM) was added."""
    return [pytest.param(*r, id="-".join(str(v) for v in (r[:-1] if i < n_old else r))) for i, r in enumerate(rows)]


# sym "0": SAME_SYM=0 puts the pipeline's FASTMATH build in the symbol-paced kernel's place (the smallest shape that has two
# workgroups and a first, a middle and a last piece)
@pytest.mark.parametrize("n_ch,seconds,chunks,noise,rate,sym", cases([(256, 10.0, 8, 0.0, 22050, None), (512, 8.0, 4, 0.05, 22050, None),
                                                                      (192, 12.0, 6, 0.0, 22050, None), (256, 6.0, 4, 0.02, 48000, None),
                                                                      (128, 6.0, 3, 0.0, 44100, None), (128, 6.0, 3, 0.0, 22050, "0")], 5))
def test_time_parallel_meets_the_contract(sa, ob, arith, monkeypatch, n_ch, seconds, chunks, noise, rate, sym):
    from helpers.oracle_compare import assert_every_channel_matches_oracle
    if sym is not None:
        monkeypatch.setenv("SAME_SYM", sym)
    n = int(rate * seconds)
    x = sa.synth_afsk(n_ch, n, rate, seed=1000 + n_ch, noise_sigma=noise)
    ref = strict_events(sa, x, rate)
    assert_every_channel_matches_oracle(ob, ob.default_config(rate), x, ref)      # the yardstick itself
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=chunks)
    rx.process_tensor(x)
    rx.sync()
    assert rx.time_parallel_chunks() == chunks
    # relaxed arithmetic inside the chunks at all three rates the pipeline is built for (whole 64-channel groups)
    assert rx.kernel_name() == ("demod_pipe_kernel" if arith == "strict" else "demod_pipe_kernel<fastmath>" if sym == "0" else "demod_sym_kernel")
    got = rx.poll_events_np()
    assert len(got[got["kind"] == 3]) >= 2 * n_ch
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(1000 + n_ch, c), exact_bursts=(noise == 0.0),
                    garbled_per_mille=(1 if noise > 0.0 and arith == "fastmath" else 0))


def test_time_parallel_streaming_calls_continue_the_channel_state(sa):
    """Three chunked calls back to back: chunk 0 of a call continues from the state the previous call's
    last chunk left, bursts that straddle a call boundary included."""
    rate, n_ch, n = 22050, 128, 22050 * 15
    x = sa.synth_afsk(n_ch, n, rate, seed=808)
    ref = strict_events(sa, x, rate)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=4)
    parts = []
    for off in range(0, n, 22050 * 5):
        rx.process_tensor(x[off:off + 22050 * 5].contiguous())
        assert rx.time_parallel_chunks() == 4
    rx.sync()
    got = rx.poll_events_np()
    # events come per call; bring them into (channel, time) order over the whole stream
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(808, c))


@pytest.mark.parametrize("name", ["npt", "two_and_two", "long_message"])
def test_time_parallel_golden_recordings(sa, ob, name):
    """The reference's recordings cut into chunks (64 copies of the recording with different lead-ins, so
    chunk boundaries fall at 64 different places of the transmission): the decoded text equals the .txt."""
    import torch
    pcm = np.fromfile(os.path.join(GOLDEN, f"{name}.22050.s16le.bin"), dtype="<i2").astype(np.float32)
    n_ch = 64
    lead = [317 * c for c in range(n_ch)]
    n = len(pcm) + max(lead) + 4 * 22050           # + what samedec's end-of-file flush appends
    x = np.zeros((n, n_ch), np.float32)
    for c in range(n_ch):
        x[lead[c]:lead[c] + len(pcm), c] = pcm
    exp = [ln for ln in open(os.path.join(GOLDEN, f"{name}.22050.s16le.txt")).read().splitlines() if ln != "+OK"]
    # 3 and 5 chunks, and 12 chunks of ~1.5 s with a 0.4 s minimum: shorter than long_message's 2.2 s bursts, so a
    # chunk's run-on passes over the whole range of the next one and the hand-over skips it
    for chunks in (3, 5, 12):
        rx = sa.SameReceiverBuilder(22050).samedec().build_batch(n_ch, time_parallel=True)
        rx.time_parallel_config(max_chunks=chunks, min_own_samples=9000)
        rx.process_tensor(torch.from_numpy(x).cuda())
        rx.sync()
        assert rx.time_parallel_chunks() == chunks
        ev = split(rx.poll_events_np(), n_ch)
        for c in range(n_ch):
            lines = [r["bytes"][: int(r["len"])].tobytes().decode() if r["kind"] == sa.TRANSPORT_MSG_START else "NNNN"
                     for r in ev[c] if r["kind"] in (sa.TRANSPORT_MSG_START, sa.TRANSPORT_MSG_END)]
            assert lines == exp, f"{chunks} chunks, lead-in {lead[c]}: {lines}"


def test_short_calls_and_odd_batches_run_strict(sa, ob):
    """Calls too short to cut, and channel counts the pipeline cannot take, run as one strict launch and
    are then bit-exact."""
    rate = 22050
    for n_ch, n in ((64, 22050), (70, 22050 * 6)):
        x = sa.synth_afsk(n_ch, n, rate, seed=5)
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
        rx.process_tensor(x)
        rx.sync()
        assert rx.time_parallel_chunks() == 1
        got = rx.poll_events_np()
        ref = strict_events(sa, x, rate)
        lg, lr = got[got["kind"] <= 3], ref[ref["kind"] <= 3]
        assert np.array_equal(lg["kind"], lr["kind"]) and np.array_equal(lg["sample_counter"], lr["sample_counter"])
        assert np.array_equal(lg["bytes"], lr["bytes"])
        assert [m for c in split(got, n_ch) for m in message_list(c)] == [m for c in split(ref, n_ch) for m in message_list(c)]


def test_soft_symbols_of_a_chunk_that_starts_fresh(sa, ob):
    """What a chunk does, on one channel with the symbol trace on (strict API): a freshly built receiver
    started one warm-up before a burst's preamble produces, while the squelch is open (Reading ... Burst),
    symbols at instants within SOFT_INSTANT_TOLERANCE samples of the continuous receiver's, with equal
    sign and values within SOFT_SYMBOL_TOLERANCE."""
    rate, n = 22050, 22050 * 10
    warm = int(64 * rate / 520.83)
    x = sa.synth_afsk(64, n, rate, seed=99)
    full = sa.SameReceiverBuilder(rate).build_batch(64, trace_symbols=True, link_only=True)
    full.process_tensor(x); full.sync()
    ev = split(full.poll_events_np(), 64)
    checked, all_dt, all_err, sign_flips = 0, [], [], 0
    for c in range(0, 64, 5):
        reading = ev[c][ev[c]["kind"] == 2]["sample_counter"]
        bursts = ev[c][ev[c]["kind"] == 3]["sample_counter"]
        if len(reading) < 2 or len(bursts) < 2:
            continue
        t_read, t_burst = int(reading[1]), int(bursts[1])          # the channel's second burst
        start = t_read - 16 * 8 * 43 - warm                        # one warm-up before its preamble
        start -= start % 20
        if start < 0:
            continue
        part = sa.SameReceiverBuilder(rate).build_batch(64, trace_symbols=True, link_only=True)
        part.process_tensor(x[start:].contiguous()); part.sync()
        ta, tb = full.read_trace(c, cap=4096), part.read_trace(c, cap=4096)
        tb = tb.copy(); tb["sample_counter"] += start
        # transmitted symbols only: the burst event comes (max_invalid + 1) bytes after the carrier stopped
        a = ta[(ta["sample_counter"] > t_read) & (ta["sample_counter"] < t_burst - 5 * 8 * 43)]
        b = tb[(tb["sample_counter"] > t_read - 64) & (tb["sample_counter"] < t_burst + 64)]
        assert len(a) > 200
        idx = np.clip(np.searchsorted(b["sample_counter"], a["sample_counter"]), 1, len(b) - 1)
        ta_ = a["sample_counter"].astype(np.int64)
        near = np.where(np.abs(b["sample_counter"][idx].astype(np.int64) - ta_)
                        < np.abs(b["sample_counter"][idx - 1].astype(np.int64) - ta_), idx, idx - 1)
        all_dt.append(np.abs(b["sample_counter"][near].astype(np.int64) - ta_))
        all_err.append(np.abs(b["sym"][near] - a["sym"]))
        sign_flips += int(np.sum(np.sign(b["sym"][near]) != np.sign(a["sym"])))
        checked += 1
    assert checked >= 5
    dt, err = np.concatenate(all_dt), np.concatenate(all_err)
    stats = (f"{len(dt)} symbols of {checked} bursts: instants max {dt.max()} samples apart (mean {dt.mean():.2f}); "
             f"soft symbols max |diff| {err.max():.4f}, {np.mean(err <= SOFT_SYMBOL_TOLERANCE):.5f} within {SOFT_SYMBOL_TOLERANCE}, "
             f"{sign_flips} sign differences")
    print(stats)
    assert sign_flips == 0, stats
    assert dt.max() <= SOFT_INSTANT_TOLERANCE, stats
    assert err.max() <= SOFT_SYMBOL_TOLERANCE, stats


def assert_awgn_tallies_equal(sa, got, ref, payloads, n, grid, strict_arithmetic, tight=False, trial_by_trial=True):
    """AWGN Monte-Carlo trials (configs[4]) decoded two ways.  Strict arithmetic on both sides: all but a handful of
    marginal trials decode to the same bytes.  Relaxed arithmetic on one side: at the grid points where noise puts bit
    errors into a burst, WHICH marginal symbols flip is chaotic in the last bit of the matched-filter sums, so there the
    contract is statistical -- detection, intact headers and bit errors per grid point equal within sampling error --
    and trial by trial only where strict mode decodes (nearly) every header intact."""
    from sameold_amd import montecarlo as mc
    ta, tb = mc.new_tally(grid), mc.new_tally(grid)
    mc.score_bursts(ref, payloads, 0, n, grid, ta)
    mc.score_bursts(got, payloads, 0, n, grid, tb)
    g, r = split(got, n), split(ref, n)
    differ = np.zeros(grid, np.int64)
    for c in range(n):
        bg, br = burst_list(g[c]), burst_list(r[c])
        if not strict_arithmetic:        # the transmitted bytes; what follows them is decoded from the noise after the carrier
            bg = [b[:payload_len(b, payloads[c])] for b in bg]
            br = [b[:payload_len(b, payloads[c])] for b in br]
        differ[c % grid] += bg != br
    print("trials that decode differently per grid point:", differ.tolist(), "bit errors", tb["bit_errors"].tolist(), "vs", ta["bit_errors"].tolist())
    if strict_arithmetic:
        assert differ.sum() <= n // 100, f"{differ.sum()} of {n} trials decode differently"
    else:
        clean = ta["intact"] >= 0.99 * np.maximum(ta["trials"], 1)
        if trial_by_trial:
            assert clean.any() and np.all(differ[clean] <= 0.03 * ta["trials"][clean] + 2), (differ, clean)
        be_a, be_b = ta["bit_errors"].astype(np.float64), tb["bit_errors"].astype(np.float64)
        # (bit errors come in lumps -- a trial that loses byte sync for a while contributes dozens -- so a grid point's count is
        # a sum over a handful of trials and moves by a lump when one marginal trial decodes the other way)
        # tight: an ordinary launch (one receiver per trial, as strict mode has it); otherwise a time-parallel launch, whose
        # chunks also start from approximated state in the middle of the trial's burst
        # "paced": an ordinary launch of the symbol-paced pipeline, whose feedback rules (lock a block late, framer's answers a
        # symbol late) move marginal acquisitions at 3-6 dB: over 1 048 576 trials its bit errors per grid point are within 4 %
        # of strict mode's and its curves within 0.02 dB (profiles/r05_ber_vs_oracle_1M.json); a grid point of this test is ~550
        # trials, a handful of which decode, and one marginal trial going the other way moves it by a lump of dozens of bits
        slack = (0.25, 100) if tight == "paced" else ((0.15, 60) if tight else (0.30, 150))
        assert np.all(np.abs(be_a - be_b) <= slack[0] * np.maximum(be_a, be_b) + slack[1]), (be_a, be_b)
    for k in ("detected", "intact"):
        # binomial: |difference| within 4 sigma of the strict count per grid point
        sig = np.sqrt(np.maximum(ta[k] * (1 - ta[k] / np.maximum(ta["trials"], 1)), 1.0))
        assert np.all(np.abs(ta[k] - tb[k]) <= 4 * sig + 2), (k, ta[k], tb[k])


def test_awgn_tally_statistically_equal(sa, arith):
    """configs[4] through the time-parallel mode: every 2 s trial cut in two (the boundary falls inside the
    burst, so the first chunk runs on and the second joins mid-burst).  Strict chunks: burst lists agree with strict mode
    on all but a handful of marginal trials; relaxed chunks: the tallies are statistically equal (see above)."""
    from sameold_amd import montecarlo as mc
    n, grid, rate, seed = 4096, 15, 22050, 31
    T = 2 * rate - (2 * rate) % 20
    x = mc.synth_trials(n, 0, T, rate, seed, 0.0, 1.0, grid)
    ref = strict_events(sa, x, rate, link_only=True)
    rx = sa.SameReceiverBuilder(rate).build_batch(n, link_only=True, time_parallel=True)
    rx.time_parallel_config(max_chunks=2, min_own_samples=8000)
    rx.process_tensor(x); rx.sync()
    assert rx.time_parallel_chunks() == 2
    got = rx.poll_events_np()
    payloads = [sa.synth_payload(seed, c) for c in range(n)]
    assert_awgn_tallies_equal(sa, got, ref, payloads, n, grid, strict_arithmetic=(arith == "strict"))


def test_time_parallel_i16_and_channel_major_inputs(sa):
    """The other two input forms of the boundary run through the same chunked launch: int16 PCM (cast in the
    kernel) and a channel-major buffer (transposed on the device slab by slab, every slab cut on its own).
    Integer-valued samples make all three inputs the same signal."""
    import torch
    rate, n_ch, n = 22050, 64, 22050 * 8
    x = torch.round(sa.synth_afsk(n_ch, n, rate, seed=4711)).contiguous()
    ref = strict_events(sa, x, rate)
    pay = lambda c: sa.synth_payload(4711, c)
    for form in ("f32", "i16", "channel_major"):
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
        rx.time_parallel_config(max_chunks=4, min_own_samples=6000)
        if form == "f32":
            rx.process_tensor(x)
        elif form == "i16":
            rx.process_tensor(x.to(torch.int16))
        else:
            rx.process_tensor(x.t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
        rx.sync()
        assert rx.time_parallel_chunks() > 1, form
        got = rx.poll_events_np()
        got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
        assert_contract(sa, got, ref, rate, n_ch, pay, what=form)


def test_flush_and_reset_in_time_parallel_mode(sa):
    """flush() (4 s of zeros) and reset() on a time-parallel batch: the long_message recording's header only
    comes out during the flush (crates/samedec/src/app.rs:118), whichever way the calls are cut."""
    import torch
    pcm = np.fromfile(os.path.join(GOLDEN, "long_message.22050.s16le.bin"), dtype="<i2").astype(np.float32)
    exp = open(os.path.join(GOLDEN, "long_message.22050.s16le.txt")).read().splitlines()[0]
    n_ch = 32
    x = torch.from_numpy(np.repeat(pcm[:, None], n_ch, axis=1)).cuda()
    rx = sa.SameReceiverBuilder(22050).samedec().build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=4)
    for rep in range(2):
        rx.process_tensor(x)
        rx.sync()
        assert rx.time_parallel_chunks() == 4
        before = [m for c in split(rx.poll_events_np(), n_ch) for m in message_list(c)]
        assert before == []
        rx.flush()
        rx.sync()
        after = split(rx.poll_events_np(), n_ch)
        for c in range(n_ch):
            assert message_list(after[c])[:1] == [(sa.TRANSPORT_MSG_START, exp.encode())], f"rep {rep} channel {c}"
        rx.reset()


@pytest.mark.parametrize("n_ch,seconds,chunks,noise,sym", cases([(256, 10.0, 8, 0.0, None), (128, 12.0, 5, 0.0, None), (192, 9.0, 8, 0.05, None),
                                                                 (4096, 6.0, 12, 0.0, None),      # (49 152 columns: pieces sorted into workgroups)
                                                                 (128, 8.0, 4, 0.0, "0")], 4))    # (SAME_SYM=0: the pipeline's FASTMATH build)
def test_per_channel_boundaries_on_channel_major_input(sa, ob, arith, monkeypatch, n_ch, seconds, chunks, noise, sym):
    """A channel-major f32 input of whole blocks is read where it lies: an energy scout and a planner on the device
    put every chunk boundary of every channel at an idle instant (no run-on), each state column streams its own
    contiguous samples.  Same contract as the uniform cut."""
    monkeypatch.setenv("SAME_PIPE_LANES", "64")      # (small test batches would otherwise get 16-channel workgroups)
    if sym is not None:
        monkeypatch.setenv("SAME_SYM", sym)
    rate = 22050
    n = int(rate * seconds)
    n -= n % 1260                    # whole blocks of every kernel that may take the chunks (20, 36 and 42 samples)
    x = sa.synth_afsk(n_ch, n, rate, seed=3000 + n_ch, noise_sigma=noise)
    ref = strict_events(sa, x, rate)
    xc = x.t().contiguous()
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=chunks)
    rx.process_tensor(xc, layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    # (the planner may settle for fewer chunks than asked for when they would own too little)
    assert chunks - 1 <= rx.time_parallel_chunks() <= chunks and rx.time_parallel_per_channel()
    assert n_ch * rx.time_parallel_chunks() > 32768 or n_ch < 4096      # the big case exercises the sorted order
    if sym == "0":
        assert rx.kernel_name() == ("demod_pipe_kernel" if arith == "strict" else "demod_pipe_kernel<fastmath>")
    got = rx.poll_events_np()
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(3000 + n_ch, c), exact_bursts=(noise == 0.0), t_end=n,
                    garbled_per_mille=(1 if noise > 0.0 and arith == "fastmath" else 0))
    # and a second call continues from the state the last chunks left
    rx.process_tensor(xc, layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    again = rx.poll_events_np()
    assert len(again[again["kind"] == 3]) >= len(got[got["kind"] == 3]) - n_ch // 8


@pytest.mark.parametrize("rate,n_ch,chunks", [(48000, 256, 6), (44100, 128, 5)])
def test_per_channel_boundaries_at_the_other_rates(sa, ob, arith, rate, n_ch, chunks):
    """A channel-major call at 44.1 / 48 kHz: the pipelines of those rates read their input in time-major rows (the strict one
    on its DC wavefront, the symbol-paced one on T), so the call is transposed on the device slab by slab (65 520 samples each: cut in time where a slab is long enough
    for it, ordinary launches otherwise).  Same contract; until round 4 such a call went down the per-lane path and
    delivered nothing."""
    n = rate * 8
    n -= n % (32 * 36 * 4)
    x = sa.synth_afsk(n_ch, n, rate, seed=3300 + n_ch)
    ref = strict_events(sa, x, rate)
    xc = x.t().contiguous()
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=chunks)
    rx.process_tensor(xc, layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    # (the last slab of a call may be too short to cut: an ordinary strict launch, whose name is then the last one reported)
    assert not rx.time_parallel_per_channel() and rx.kernel_name() in (("demod_pipe_kernel",) if arith == "strict" else ("demod_pipe_kernel", "demod_sym_kernel"))
    got = rx.poll_events_np()
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]      # (events come per launch)
    assert len(got[got["kind"] == 3]) >= 2 * n_ch
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(3300 + n_ch, c), exact_bursts=True, t_end=n, what=f"channel-major {rate}")


def test_channel_major_call_that_is_not_whole_blocks(sa, ob, arith, monkeypatch):
    """A channel-major call whose length is no multiple of the kernel's block still takes the per-channel path: the
    samples behind the last whole block go through the any-configuration kernel on the channels' own state, and the next
    call continues from there."""
    monkeypatch.setenv("SAME_PIPE_LANES", "64")      # (small test batches would otherwise get 16-channel workgroups)
    rate, n_ch = 22050, 256
    n = 22050 * 5 + 26                 # a multiple of 4 (16-byte streams), of neither 20 nor 36
    assert n % 4 == 0 and n % 20 != 0 and n % 36 != 0
    x = sa.synth_afsk(n_ch, 2 * n, rate, seed=8800)
    ref = strict_events(sa, x, rate)
    parts = [x[i * n:(i + 1) * n].t().contiguous() for i in range(2)]       # (kept alive: the launches are asynchronous)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    for i in range(2):
        rx.process_tensor(parts[i], layout=sa.LAYOUT_CHANNEL_MAJOR)
        assert rx.time_parallel_chunks() >= 2 and rx.time_parallel_per_channel()
    rx.sync()
    got = rx.poll_events_np()
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(8800, c), exact_bursts=True, t_end=2 * n)


def test_per_channel_boundaries_streaming_calls_with_bursts_across_the_call_boundary(sa, monkeypatch):
    """Channel-major calls back to back, cut where bursts are in progress on many channels (every channel's schedule has its
    own lead-in): the state a call leaves is that of the chunk its hand-over chain ends in, so the burst that straddles the
    boundary is delivered whole by the next call.  The whole stream must meet the contract against strict mode."""
    monkeypatch.setenv("SAME_PIPE_LANES", "64")
    rate, n_ch = 22050, 256
    part = 22050 * 5
    part -= part % 1260
    x = sa.synth_afsk(n_ch, 4 * part, rate, seed=9090)
    ref = strict_events(sa, x, rate)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=4)
    for i in range(4):
        rx.process_tensor(x[i * part:(i + 1) * part].t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
        assert rx.time_parallel_per_channel() and rx.time_parallel_chunks() >= 3
    rx.sync()
    got = rx.poll_events_np()
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
    # bursts in progress at a boundary: a good third of the channels at each of the three
    link = ref[ref["kind"] <= 3]
    busy = sum(int(np.any((link["channel"] == c) & (link["kind"] == 2) & (link["sample_counter"] < b) &
                          (np.roll(link["sample_counter"], -1) > b))) for b in (part, 2 * part, 3 * part) for c in range(n_ch))
    assert busy >= n_ch // 2, busy
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(9090, c), what="streaming channel-major", t_end=4 * part)


def test_planning_on_the_plan_stream_and_on_a_callers_stream(sa, monkeypatch):
    """Channel-major calls of one stream alternately on the library's own stream (scout, planner and sort then run on the
    plan stream, beside the previous launch) and on a stream of the caller (everything in that stream's order): both
    streams' planning shares the energy map, the launches share the wide state.  Two calls stay in flight throughout; the
    whole stream must meet the contract, and SAME_TP_PLAN_STREAM=0 must deliver the very same events."""
    import torch
    monkeypatch.setenv("SAME_PIPE_LANES", "64")
    rate, n_ch = 22050, 4096
    part = 22050 * 3
    part -= part % 1260
    x = sa.synth_afsk(n_ch, 4 * part, rate, seed=5151)
    ref = strict_events(sa, x, rate)
    parts = [x[i * part:(i + 1) * part].t().contiguous() for i in range(4)]
    torch.cuda.synchronize()
    mine = torch.cuda.Stream()

    def run():
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
        for i, p in enumerate(parts):
            if i % 2 == 0:
                rx.process_tensor(p, layout=sa.LAYOUT_CHANNEL_MAJOR)                                  # own stream + plan stream
            else:
                rx.process_tensor(p, layout=sa.LAYOUT_CHANNEL_MAJOR, stream=mine.cuda_stream)       # the caller's stream
            assert rx.time_parallel_per_channel()
        rx.sync()
        got = rx.poll_events_np()
        return got[np.lexsort((np.arange(len(got)), got["channel"]))]

    got = run()
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(5151, c), what="alternating streams", t_end=4 * part)
    monkeypatch.setenv("SAME_TP_PLAN_STREAM", "0")
    same = run()
    assert len(same) == len(got) and np.array_equal(same["kind"], got["kind"]) and np.array_equal(same["sample_counter"], got["sample_counter"])
    assert np.array_equal(same["bytes"], got["bytes"])
    # ... and so must a launch whose fresh state columns, hand-over records, sort bins and cursors are made by separate
    # kernels (SAME_TP_PROLOGUE=0: rounds 2-5) instead of the one prologue kernel copying a template blob (round 6)
    monkeypatch.delenv("SAME_TP_PLAN_STREAM")
    monkeypatch.setenv("SAME_TP_PROLOGUE", "0")
    same = run()
    assert len(same) == len(got) and np.array_equal(same["kind"], got["kind"]) and np.array_equal(same["sample_counter"], got["sample_counter"])
    assert np.array_equal(same["bytes"], got["bytes"])


def test_prologue_kernel_on_a_time_major_call_equals_the_separate_launches(sa, monkeypatch, capfd):
    """A time-major time-parallel call (uniform cuts) starts with the same prologue kernel: the events of three streamed
    calls must equal those of the launches that initialise their columns with init_state_kernel, call for call.  Which
    start-up ran is read from the library's SAME_DEBUG line, so that the two runs cannot take the same path unnoticed."""
    rate, n_ch = 22050, 1024
    part = 22050 * 4
    part -= part % 1260
    x = sa.synth_afsk(n_ch, 3 * part, rate, seed=6262)

    def run():
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
        for i in range(3):
            rx.process_tensor(x[i * part:(i + 1) * part])
            assert rx.time_parallel_chunks() > 1
        rx.sync()
        got = rx.poll_events_np()
        return got[np.lexsort((np.arange(len(got)), got["channel"]))]

    monkeypatch.setenv("SAME_DEBUG", "1")
    capfd.readouterr()
    a = run()
    err = capfd.readouterr().err
    assert err.count("start-up: prologue kernel") == 3 and "start-up: separate launches" not in err, err[-2000:]
    monkeypatch.setenv("SAME_TP_PROLOGUE", "0")
    b = run()
    err = capfd.readouterr().err
    assert err.count("start-up: separate launches") == 3 and "start-up: prologue kernel" not in err, err[-2000:]
    assert len(a) == len(b) and len(a) > 0 and (a["kind"] == 3).sum() > n_ch
    assert np.array_equal(a["kind"], b["kind"]) and np.array_equal(a["channel"], b["channel"])
    assert np.array_equal(a["sample_counter"], b["sample_counter"]) and np.array_equal(a["bytes"], b["bytes"])


def test_sorted_launches_are_deterministic_and_the_timers_nest(sa, monkeypatch):
    """Pieces sorted by length into workgroups (more state columns than the machine holds at once): which pieces share a
    workgroup depends on the order atomics land in, what every column computes must not -- two runs deliver identical
    events.  And the demodulation kernel's own timer lies inside the launch's."""
    rate, n_ch = 22050, 4096
    n = 22050 * 6
    n -= n % 1260
    xc = sa.synth_afsk(n_ch, n, rate, seed=777).t().contiguous()
    runs = []
    for _ in range(2):
        rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
        rx.set_kernel_timing(True)
        rx.time_parallel_config(max_chunks=12)        # (the default with the symbol-paced pipeline is one round: 8 pieces)
        rx.process_tensor(xc, layout=sa.LAYOUT_CHANNEL_MAJOR)
        rx.sync()
        assert rx.time_parallel_per_channel() and n_ch * rx.time_parallel_chunks() > 32768
        assert 0.0 < rx.last_demod_kernel_ms() <= rx.last_kernel_ms()
        runs.append(rx.poll_events_np())
    a, b = runs
    assert len(a) == len(b) and np.array_equal(a["kind"], b["kind"]) and np.array_equal(a["channel"], b["channel"])
    assert np.array_equal(a["sample_counter"], b["sample_counter"]) and np.array_equal(a["bytes"], b["bytes"])


def test_per_channel_boundaries_fall_back_when_there_is_no_quiet_instant(sa, monkeypatch):
    """Channels that are never quiet (noise as loud as the bursts) leave the planner no allowed instant: it cuts at the
    length limit and the chunks run on until idle, as with uniform boundaries.  Whatever the two modes decode there
    is noise-driven; the call must complete and the clean channels beside them still meet the contract."""
    import torch
    monkeypatch.setenv("SAME_PIPE_LANES", "64")
    rate, n_ch, n = 22050, 128, 22050 * 8
    n -= n % 1260
    x = sa.synth_afsk(n_ch, n, rate, seed=77)
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    x[:, ::4] += torch.randn((n, n_ch // 4), device="cuda", generator=gen) * 3000.0      # every fourth channel drowned in noise
    ref = strict_events(sa, x, rate)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=6)
    rx.process_tensor(x.t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    assert rx.time_parallel_per_channel()
    got = rx.poll_events_np()
    clean = np.array([c for c in range(n_ch) if c % 4], dtype=np.uint32)
    remap = {int(c): i for i, c in enumerate(clean)}

    def only_clean(ev):
        e = ev[np.isin(ev["channel"], clean)].copy()
        e["channel"] = np.array([remap[int(c)] for c in e["channel"]], dtype=np.uint32)
        return e
    assert_contract(sa, only_clean(got), only_clean(ref), rate, len(clean), lambda i: sa.synth_payload(77, int(clean[i])))


def test_streaming_channel_major_calls_with_noise_and_forced_cuts(sa, monkeypatch, arith):
    """Four channel-major calls of one stream, bursts straddling the call boundaries, with mild noise on every channel
    (the contract is statistical there) and every eighth channel drowned in noise (no quiet instant: forced cuts, chunks
    that run on, calls that end without a hand-over -- the state carried on is then that of the chunk the chain stops in).
    The channels that can be decoded must meet the contract over the whole stream; the drowned ones must not disturb
    them or stall the calls."""
    import torch
    monkeypatch.setenv("SAME_PIPE_LANES", "64")
    rate, n_ch = 22050, 256
    part = 22050 * 5
    part -= part % 1260
    x = sa.synth_afsk(n_ch, 4 * part, rate, seed=8181, noise_sigma=0.03)
    gen = torch.Generator(device="cuda"); gen.manual_seed(9)
    x[:, ::8] += torch.randn((4 * part, n_ch // 8), device="cuda", generator=gen) * 3000.0
    ref = strict_events(sa, x, rate)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=4)
    for i in range(4):
        rx.process_tensor(x[i * part:(i + 1) * part].t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
        assert rx.time_parallel_per_channel()
    rx.sync()
    got = rx.poll_events_np()
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
    clean = np.array([c for c in range(n_ch) if c % 8], dtype=np.uint32)
    remap = np.full(n_ch, -1, dtype=np.int64); remap[clean] = np.arange(len(clean))

    def only_clean(ev):
        e = ev[np.isin(ev["channel"], clean)].copy()
        e["channel"] = remap[e["channel"]].astype(np.uint32)
        return e
    assert_contract(sa, only_clean(got), only_clean(ref), rate, len(clean), lambda i: sa.synth_payload(8181, int(clean[i])), exact_bursts=False,
                    what="noisy streaming channel-major", t_end=4 * part, garbled_per_mille=(2 if arith == "fastmath" else 1))


def test_bench_configuration_of_the_headline_mode(sa, ob, arith):
    """BASELINE.json configs[1] exactly as bench.py runs its headline mode: 4 096 channels x 220 500 samples per call, seed
    20260000, channel-major input, default knobs and chunk count (8 with the symbol-paced pipeline, 10 with strict arithmetic inside the chunks) -- and two more calls on carried state, which is what the
    bench's timed steps are.  One continuous stream of three calls (bursts straddle the call boundaries; bench.py itself
    feeds one buffer again and again, a discontinuity per step that means nothing to check): strict mode against the oracle
    on every channel of the first call, the time-parallel receiver against strict mode over the whole stream."""
    import bench
    from helpers.oracle_compare import assert_every_channel_matches_oracle
    rate, n_ch, n, seed = 22050, 4096, 220500, 20260000
    x3 = sa.synth_afsk(n_ch, 3 * n, rate, seed=seed)      # (its first n samples are the bench's input: the generator is causal)
    strict = sa.SameReceiverBuilder(rate).build_batch(n_ch)
    tp = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    refs, gots = [], []
    for k in range(3):
        x = x3[k * n:(k + 1) * n]
        strict.process_tensor(x.contiguous()); strict.sync()
        tp.process_tensor(x.t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR); tp.sync()
        assert tp.time_parallel_chunks() == (8 if arith == "fastmath" else 10) and tp.time_parallel_per_channel()
        assert tp.kernel_name() == ("demod_sym_kernel" if arith == "fastmath" else "demod_pipe_kernel")
        refs.append(strict.poll_events_np()); gots.append(tp.poll_events_np())
        if k == 0:
            assert_every_channel_matches_oracle(ob, ob.default_config(rate), x.contiguous(), refs[0])
            assert_contract(sa, gots[0], refs[0], rate, n_ch, lambda c: sa.synth_payload(seed, c), what="first call", t_end=n)
    ref, got = np.concatenate(refs), np.concatenate(gots)
    ref = ref[np.lexsort((np.arange(len(ref)), ref["channel"]))]
    got = got[np.lexsort((np.arange(len(got)), got["channel"]))]
    per_call = [int((g["kind"] == 3).sum()) for g in gots], [int((r["kind"] == 3).sum()) for r in refs]
    print("bursts per call, time-parallel / strict:", per_call)
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(seed, c), what="three calls", t_end=3 * n)
    ok, note = bench.tp_contract(sa, ref, got, n_ch, seed, "three calls on carried state", t_end=3 * n, rate=rate)
    print(note)
    assert ok, note


def test_a_weak_burst_beside_a_strong_one(sa, monkeypatch):
    """The boundary planner calls a stretch quiet when the scout's energy is below 8 % of the channel's own loudest reading:
    a burst five times weaker than its neighbours looks quiet, so cuts may fall inside it and the chunk before runs on
    through it.  Every other burst of every other channel at 0.2 of its amplitude: the contract holds all the same."""
    import torch
    monkeypatch.setenv("SAME_PIPE_LANES", "64")
    rate, n_ch = 22050, 256
    n = 22050 * 12
    n -= n % 1260
    x = sa.synth_afsk(n_ch, n, rate, seed=5150)
    ev = split(strict_events(sa, x, rate, link_only=True), n_ch)
    scale = torch.ones((n, n_ch), device=x.device)
    weak = 0
    for c in range(0, n_ch, 2):
        t_s = [int(t) for t in ev[c][ev[c]["kind"] == 1]["sample_counter"]]
        t_b = [int(t) for t in ev[c][ev[c]["kind"] == 3]["sample_counter"]]
        for i, tb in enumerate(t_b):
            if i % 2 == 1:
                ts = max([t for t in t_s if t < tb] or [0])
                scale[max(ts - 6000, 0):min(tb + 2000, n), c] = 0.2     # from well before the preamble to after the last byte
                weak += 1
    assert weak >= n_ch // 2
    x = (x * scale).contiguous()
    ref = strict_events(sa, x, rate)
    rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=8)
    rx.process_tensor(x.t().contiguous(), layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    assert rx.time_parallel_per_channel()
    got = rx.poll_events_np()
    assert len(ref[ref["kind"] == 3]) >= 4 * n_ch          # the weak bursts decode in strict mode (the AGC takes care of the level)
    assert_contract(sa, got, ref, rate, n_ch, lambda c: sa.synth_payload(5150, c), what="weak beside strong", t_end=n)
