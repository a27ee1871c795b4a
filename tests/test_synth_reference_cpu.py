"""The float64 reference of the signal generators (tests/helpers/synth_reference.py) held to what it can be held to without
a GPU: Philox to the published known answers, the header text to the library's host-side same_synth_payload, the ideal
detector to the textbook error rate, the reference's own noise to the law the device's noise is held to, and every shape
of tests/test_synth_gpu.py to the margin that lets that file compare every sample without excusing one."""
import numpy as np
import pytest

import sameold_amd as sa
from sameold_amd import build as sbuild
from helpers import synth_reference as ref


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return sa.load_library()


def test_philox_known_answers():
    for counter, key, want in ref.KAT_PHILOX4X32_10:
        got = ref.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]
    # vectorised over counters, with one key for all of them and with a key per counter
    counters = np.array([k[0] for k in ref.KAT_PHILOX4X32_10], dtype=np.uint64)
    keys = np.array([k[1] for k in ref.KAT_PHILOX4X32_10], dtype=np.uint64)
    want = np.array([k[2] for k in ref.KAT_PHILOX4X32_10], dtype=np.uint32)
    assert np.array_equal(ref.philox4x32_10(counters, keys), want)
    assert np.array_equal(ref.philox4x32_10(counters[[2, 2]], keys[2])[1], want[2])


def test_splitmix64_stream_and_its_closed_form():
    # first outputs of SplitMix64 from state 0 (Steele, Lea, Flood; the values every implementation's tests quote)
    state, outs = 0, []
    for _ in range(3):
        state, z = ref.splitmix64(state)
        outs.append(z)
    assert outs == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]
    start = np.array([0, 2 ** 64 - 1, 0x123456789abcdef0], dtype=np.uint64)
    got = ref._splitmix64_at(start[None, :], np.arange(1, 6, dtype=np.uint64)[:, None])
    for c, s in enumerate(start):
        state = int(s)
        for k in range(5):
            state, z = ref.splitmix64(state)
            assert int(got[k, c]) == z


def test_payload_equals_the_hosts_byte_for_byte(lib):
    rng = np.random.default_rng(20260101)
    pairs = [(int(s), int(c)) for s, c in zip(rng.integers(0, 2 ** 64, 2000, dtype=np.uint64),
                                              rng.integers(0, 2 ** 32, 2000, dtype=np.uint64))]
    pairs += [(s, c) for s in (0, 2 ** 64 - 1) for c in (0, 2 ** 32 - 1, 5)] + [(77, 0), (77, 2 ** 32 - 1)]
    pairs += [(31337, c) for c in range(1000, 1070)]                       # neighbouring channels of one seed, as the tests use them
    locations, originators = set(), set()
    for seed, channel in pairs:
        want = sa.synth_payload(seed, channel)
        got = ref.payload(seed, channel)
        assert got == want, (seed, channel, got, want)
        head, tail = got.split(b"+")
        locations.add(head.count(b"-") - 2)
        originators.add(head[5:8])
        assert len(tail) == len(b"TTTT-JJJHHMM-LLLLLLLL-")
    assert locations == {1, 2, 3, 4, 5, 6}
    assert originators == {b"EAS", b"CIV", b"WXR", b"PEP"}


def test_ideal_detector_meets_the_textbook_error_rate():
    """Clean bursts of trials()'s own modulator (skews over the whole +-0.25 %) in numpy's Gaussian noise at the sigma of
    their grid point, through noncoherent_fsk_bits: the error count lies within 4 binomial standard deviations of
    N exp(-Eb/2N0)/2 at 4, 6 and 8 dB.  This is the band the device's trials are held to in test_synth_gpu.py."""
    T = 34816                                                               # the longest burst at the slowest clock, whole
    r = ref.trials(192, 0, T, 22050, 555, 4.0, 2.0, 3, with_noise=False)
    assert np.array_equal(ref.whole_symbols(r, T), r["n_bits"])
    assert r["sps"].min() < 22050 / 520.83 / 1.002 and r["sps"].max() > 22050 / 520.83 * 1.002
    noise = np.random.default_rng(4242).standard_normal(r["clean"].shape) * r["sigma"][None, :]
    got = ref.noncoherent_fsk_bits(r["clean"] + noise, r["lead"], r["sps"], r["n_bits"], 22050)
    rows = ref.bit_error_z_scores(got, r, r["n_bits"])
    for db, bits, errors, z in rows:
        print(f"{db:4.1f} dB: {errors} errors in {bits} bits, z = {z:+.2f}")
    assert [row[0] for row in rows] == [4.0, 6.0, 8.0]
    assert all(row[1] > 30000 for row in rows)
    assert all(abs(row[3]) < 4.0 for row in rows), rows
    # and without noise it reads every bit
    clean = ref.noncoherent_fsk_bits(r["clean"], r["lead"], r["sps"], r["n_bits"], 22050)
    assert all(row[2] == 0 for row in ref.bit_error_z_scores(clean, r, r["n_bits"]))


def test_detector_counts_only_whole_symbols_of_a_cut_burst():
    case = {**ref.TRIAL_CASES["ebn0_axis"], "n_trials": 12, "n_samples": 24576}         # too short for a long header
    r = ref.trials(**case, with_noise=False)
    n_bits = ref.whole_symbols(r, case["n_samples"])
    assert (n_bits < r["n_bits"]).any() and (n_bits == r["n_bits"]).any() and n_bits.min() > 400
    got = ref.noncoherent_fsk_bits(r["clean"], r["lead"], r["sps"], n_bits, case["rate"])
    assert all(row[2] == 0 for row in ref.bit_error_z_scores(got, r, n_bits))


def test_the_references_own_noise_obeys_the_noise_law():
    case = ref.TRIAL_CASES["noise_law"]
    trial = [case["first_trial"] + c for c in range(case["n_trials"])]
    ref.assert_noise_law(ref.trial_normals(trial, case["n_samples"], case["seed"]), quads=True, what="trial noise")
    ref.assert_noise_law(ref.afsk(**ref.AFSK_CASES["noisy"])["g"], quads=False, what="workload noise")


def test_noise_law_notices_what_it_is_for():
    """a repeated normal every fourth sample, a shared uniform, a cut tail and a wrong scale each break the law"""
    g = np.random.default_rng(1).standard_normal((65536, 64))
    ref.assert_noise_law(g)
    repeated = g.copy()
    repeated[4::4] = repeated[3:-1:4]
    shared = g.copy()
    shared[1::4] = np.sqrt(0.5) * (g[0::4] + g[1::4])
    for bad in (repeated, shared, np.clip(g, -4.0, 4.0), g * np.sqrt(2.0), g + 0.03):
        with pytest.raises(AssertionError):
            ref.assert_noise_law(bad)


@pytest.mark.parametrize("name", sorted(ref.TRIAL_CASES))
def test_boundary_margin_of_the_trial_shapes(name):
    r = ref.trials(**ref.TRIAL_CASES[name], with_noise=False)
    assert r["boundary_margin"].shape == (ref.TRIAL_CASES[name]["n_trials"],)
    assert r["boundary_margin"].min() > 1e-9, r["boundary_margin"].min()


@pytest.mark.parametrize("name", sorted(ref.AFSK_CASES))
def test_boundary_margin_of_the_workload_shapes(name):
    r = ref.afsk(**{**ref.AFSK_CASES[name], "noise_sigma": 0.0})
    assert r["boundary_margin"].min() > 1e-9, r["boundary_margin"].min()
    if ref.AFSK_CASES[name]["integer_symbols"]:
        assert set(r["sps"]) == {{22050: 42.0, 44100: 84.0, 48000: 92.0}[ref.AFSK_CASES[name]["rate"]]}


def test_the_cycle_of_the_workload_reference():
    """H gap H gap H gap E gap E gap E gap2, the phase starting anew in every burst, and silence before the lead"""
    case = ref.AFSK_CASES["one_cycle"]
    r = ref.afsk(**{**case, "n_channels": 3})
    for c in range(3):
        first = r["burst_first"][c]
        assert len(first) >= 6 and first[0] == int(np.ceil(r["lead"][c]))
        assert [int(r["burst"][t, c]) for t in first[:6]] == [0, 1, 2, 3, 4, 5]
        assert np.all(r["clean"][: first[0], c] == 0.0)
        gaps = np.diff(first[:6]) - np.array([len(r["payloads"][c]) + 16] * 3 + [20] * 2) * 8 * r["sps"][c]
        assert np.all(np.abs(gaps - case["rate"]) < 1.0)
        dphi = np.float32(ref._dphi(ref.MARK_HZ, case["rate"]))
        assert np.all(r["clean"][first, c] == r["amp"][c] * np.cos(np.pi * float(dphi) / 2147483648.0))
