"""Messages whose bursts disagree (tests/helpers/disagreeing_bursts.py), on the CPU and by the oracle alone.

The first two tests are the fixture's preconditions: on every channel the oracle's link layer delivers exactly the bytes that
were transmitted, burst by burst, and every class produces the outcome it is built for -- a START with corrected bits, a
START with the WRONG header where two of three bursts carry the same flipped bit (the reference votes by majority and the
result passes its header check: so does the oracle, and so must the device), MSG_ERR for two bursts that differ, no START
for a single burst, a START at a deadline poll wherever a burst is missing.  tests/test_disagreeing_bursts_gpu.py relies
on both.

The third holds the device's transport layer (sameold_amd/csrc/same_transport_dev.h, built with g++ under ASan + UBSan by
tests/test_device_transport_cpu.py's driver) to the oracle on these channels: fed the oracle's link events, and a wake-up at
each instant at which the oracle's transport state changed, it must report the oracle's transport events.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import disagreeing_bursts as db
from test_device_transport_cpu import driver, run          # noqa: F401  (the fixture that builds the stand-alone driver)

SEED = 2027
CASES = [("batch", 22050, 8), ("batch", 48000, 3), ("two_messages", 22050, 8)]
START, END, ERR = 18, 19, 20


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    binding.lib()
    return binding


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    yield
    _CASES.clear()


def the_case(ob, case):
    """(batch, the oracle's events per channel), computed once per module run"""
    if case not in _CASES:
        kind, rate, n = case
        b = db.batch(rate, SEED, n) if kind == "batch" else db.two_message_batch(rate, SEED, n)
        _CASES[case] = (b, db.oracle_events(ob, ob.default_config(rate), b["x"]))
    return _CASES[case]


def hamming(a, b):
    return int(np.unpackbits(np.frombuffer(a, np.uint8) ^ np.frombuffer(b, np.uint8)).sum())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_the_oracle_delivers_the_transmitted_bytes_of_every_burst(ob, case):
    b, events = the_case(ob, case)
    trailing = int(ob.default_config(case[1]).frame_max_invalid) + 1
    n = 0
    for c, ev in enumerate(events):
        got = [e[6] for e in ev if e[0] == 3]
        want = b["framed"][c]
        assert len(got) == len(want), f"channel {c} ({b['cls'][c]}): {len(got)} bursts, {len(want)} sent"
        for k, (g, w) in enumerate(zip(got, want)):
            # (behind the transmitted bytes: only what the framer decodes from the silence until the carrier is given up)
            assert g[:len(w)] == w and len(g) - len(w) <= trailing, f"channel {c} ({b['cls'][c]}) burst {k}: {g!r} for {w!r}"
        n += len(got)
    assert n >= 3 * len(events)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_every_class_gives_the_outcome_it_is_built_for(ob, case):
    b, events = the_case(ob, case)
    trailing = int(ob.default_config(case[1]).frame_max_invalid) + 1
    for c, ev in enumerate(events):
        name, h, what = b["cls"][c], b["header"][c], f"channel {c} ({b['cls'][c]})"
        tr = [e for e in ev if e[0] >= START]
        starts = [e for e in ev if e[0] == START]
        at_deadline = db.deadline_starts(ev)
        bursts = [e for e in ev if e[0] == 3]
        if name == "two_messages":
            assert [e[0] for e in tr] == [START, END, START], what
            assert [e[6] for e in starts] == list(h), what
            assert all(e[4] == 49 and e[5] == c % 2 for e in starts), what          # odd channels: one corrected bit each
            continue
        if name == "single":
            assert not starts, what
            assert [e[0] for e in tr] == [END], what
            continue
        if name == "two_mismatch":
            assert tr and tr[0][0] == ERR and tr[0][4] == 3, what                     # Malformed: the estimate stops at the mismatch
            assert tr[0][1] not in {e[1] for e in bursts}, what                       # (delivered at the deadline behind burst 2)
            continue
        assert starts, what
        first = starts[0]
        # every first START here comes at a deadline poll: 682 symbols behind the burst that armed it, in silence
        assert first in at_deadline, what
        armed_by = [e for e in bursts if e[1] < first[1]][-1]
        assert first[2] == armed_by[2] + db.INTERBURST_SYMBOLS, what
        if name in db.CORRECTED:
            assert first[6] == h and first[4] == 49 and first[5] > 0, what
        elif name == "same_bit_twice":
            wrong = [s for s in b["sent"][c][:3] if s != h]
            assert len(wrong) == 2 and wrong[0] == wrong[1], what
            assert first[6] == wrong[0] != h and hamming(first[6], h) == 1 and db.is_header(first[6]), what
            assert first[4] == 49 and first[5] == 1, what
        elif name in ("missing_second", "missing_third", "late_third"):
            # two bursts only when the deadline passes: no voting byte, no parity error, and the header whole
            assert first[6] == h and first[4] == 0 and first[5] == 0, what
            assert len([e for e in bursts if e[1] < first[1]]) == 2, what
        elif name in ("short_first", "short_third"):
            # the header whole, by two bursts where the short one has ended: three voted only on its bytes (and on the few
            # it decoded from the silence behind them)
            cut = 30 if name == "short_first" else 25
            assert first[6] == h and cut <= first[4] <= cut + trailing, what
        else:                                                                         # unanimous, four_bursts, the eom classes
            assert first[6] == h and first[4] == 49 and first[5] == 0, what
            assert len([e for e in bursts if e[1] < first[1]]) == (4 if name == "four_bursts" else 3), what
        ends = [e for e in tr if e[0] == END]
        if name in ("eom_nnzz", "eom_single", "eom_none"):
            assert not ends, what
        else:
            assert len(ends) == 1 and ends[0][1] > first[1], what


def test_the_device_transport_layer_equals_the_oracle(ob, driver, tmp_path):
    """same_transport_dev.h, fed the oracle's link events of every channel and a wake-up (kind 8) at each of the oracle's
    transport-event instants, reports the oracle's transport events: kind, sample counter and header text."""
    jobs = []
    for case in (CASES[0], CASES[2]):
        b, events = the_case(ob, case)
        for c, ev in enumerate(events):
            feed, want = [], []
            for kind, sample, symbol, _len, _aux, _aux2, data in ev:
                if kind < 16:
                    feed.append(f"{kind} {sample} {symbol} {data.hex() or '-'}")
                else:
                    feed.append(f"8 {sample} {symbol} -")
                    want.append((kind, sample, data.decode() if kind == START else ""))
            p = tmp_path / f"{case[0]}_{c}.txt"
            p.write_text("\n".join(feed) + "\n")
            jobs.append((f"{case[0]} channel {c} ({b['cls'][c]})", str(p), want))

    def one(job):
        what, path, want = job
        got = []
        for ln in run(driver, "golden", path):
            kind, sample, _n, text = ln.split(b" ", 3)
            got.append((int(kind), int(sample), text.decode() if int(kind) == START else ""))
        return what, got, want

    with ThreadPoolExecutor(8) as pool:
        results = list(pool.map(one, jobs))
    n_events = n_messages = 0
    for what, got, want in results:
        assert got == want, what
        n_events += len(want)
        n_messages += sum(k in (START, END) for k, _, _ in want)
    assert n_messages >= len(jobs)
    print(f"DISAGREE device core: {len(jobs)} channels, {n_events} transport events ({n_messages} START / END) equal the oracle's")
