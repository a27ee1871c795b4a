"""The two signal generators of same_synth.hip (synth_kernel behind sa.synth_afsk, trials_kernel behind
montecarlo.synth_trials) against the float64 reference of tests/helpers/synth_reference.py, sample for sample, and against
what does not depend on that reference: the law of unit white noise, and the bit error rate of an ideal detector.

Three rules hold wherever samples are compared (tests/test_synth_reference_cpu.py shows that no symbol boundary of these
shapes lies within rounding of a sample, so no sample is excused):
  symbol index   inside a burst |x - x_ref| stays below 0.2 amp: a wrong symbol, tone or phase reset is far above it
  scale          everywhere |x - x_ref| < 1e-4 (amp + sigma): a gain or sigma error of 0.001 dB
  measured       |x - x_ref| / (amp + |sigma g|) < 4 x the worst value one MI355X gave (MEASURED below, and per shape in
                 profiles/r08_synth_vs_reference.txt):
                   trial generator               2.70e-07
                   workload generator, clean     1.33e-07
                   workload generator, noisy     1.81e-07   (__logf; recorded apart from the first)
                 Outside the bursts the same bound holds against sigma g_ref alone: nothing of the carrier leaks.
"""
import numpy as np
import pytest

from helpers import synth_reference as ref

pytestmark = pytest.mark.gpu

# worst |x - x_ref| / (amp + |sigma g|) measured on one MI355X against the float64 reference 
MEASURED = {"trials": 2.70e-07, "afsk_clean": 1.33e-07, "afsk_noisy": 1.81e-07}
SCALE = 1e-4


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


# (every shape is compared by one test only, so each reference lives as long as its test and no longer)
def trial_reference(name, with_noise=True):
    return ref.trials(**ref.TRIAL_CASES[name], with_noise=with_noise)


def afsk_reference(name):
    return ref.afsk(**ref.AFSK_CASES[name], with_margin=False)


def device_trials(name):
    from sameold_amd import montecarlo as mc
    k = ref.TRIAL_CASES[name]
    x = mc.synth_trials(k["n_trials"], k["first_trial"], k["n_samples"], k["rate"], k["seed"], k["lo"], k["step"], k["n_grid"])
    return x.cpu().numpy().astype(np.float64)


def device_afsk(sa, name):
    k = ref.AFSK_CASES[name]
    x = sa.synth_afsk(k["n_channels"], k["n_samples"], k["rate"], seed=k["seed"], noise_sigma=k["noise_sigma"],
                      integer_symbols=k["integer_symbols"])
    return x.cpu().numpy().astype(np.float64)


def assert_samples_equal(x, r, measured, what, sigma_in_scale=True):
    """the three rules of the module docstring on every sample of x [T, n]; returns the worst measured ratio"""
    assert x.shape == r["x"].shape and np.isfinite(x).all()
    amp, sigma = r["amp"][None, :], r["sigma"][None, :]
    noise = r["noise"] if "noise" in r else np.zeros_like(x)
    inside = r["sym_index"] >= 0
    d = np.abs(x - r["x"])
    ratio = d / (amp + np.abs(noise))
    worst = float(ratio.max())
    t, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"{what}: worst |x - x_ref| / (amp + |sigma g|) = {worst:.3e} at sample {t} of column {c} "
          f"({'burst' if inside[t, c] else 'silence'}); worst |x - x_ref| / (amp + sigma) = "
          f"{float((d / (amp + (sigma if sigma_in_scale else 0.0))).max()):.3e}; "
          f"in bursts, worst |x - x_ref| / amp = {float(np.where(inside, d / amp, 0.0).max()):.3e}")
    assert inside.any() and not inside.all()
    assert np.all(np.where(inside, d, 0.0) < 0.2 * amp), f"{what}: a symbol differs"
    assert np.all(d < SCALE * (amp + (sigma if sigma_in_scale else 0.0))), f"{what}: scale"
    assert 4.0 * measured < SCALE
    assert worst < 4.0 * measured, (what, worst, measured)
    # outside the bursts there is noise only: nothing of the carrier leaks
    leak = np.where(inside, 0.0, np.abs(x - noise) / (amp + np.abs(noise)))
    assert leak.max() < 4.0 * measured, (what, "carrier outside the burst", float(leak.max()))
    return worst


# ------------------------------------------------------------------ a. trial generator, sample for sample
@pytest.mark.parametrize("name", ["wave_and_a_bit", "44100", "48000", "trial_number_wraps", "one_grid_point",
                                  "negative_lo_fractional_step"])
def test_trials_equal_the_reference_sample_for_sample(sa, name):
    """trials_kernel against trials(): 70 trials (a whole wavefront and a partial one) from trial 1000 over a 0..14 dB grid at
    22 050 Hz, 6 trials at 44 100 and 48 000 Hz, 70 trials whose number wraps past 2^32 (the counter and the grid index use
    the wrapped 32-bit number), a one-point grid, and a grid from -2.5 dB in steps of 0.7 dB.
    Measured on one MI355X: worst |x - x_ref| / (amp + |sigma g|) = 2.70e-07 over these six shapes (MEASURED["trials"])."""
    k = ref.TRIAL_CASES[name]
    r = trial_reference(name)
    x = device_trials(name)
    assert_samples_equal(x, r, MEASURED["trials"], f"trials {name}")
    # some bursts end inside the buffer (a noise-only tail is compared) and the lead-in is noise only
    ends = r["lead"] + r["n_bits"] * r["sps"]
    assert (ends < k["n_samples"] - 100).any() and np.all(r["sym_index"][:int(0.1 * k["rate"])] < 0)
    if name == "trial_number_wraps":
        assert r["trial"][34] == 2 ** 32 - 1 and r["trial"][35] == 0
        assert np.array_equal(r["ebn0_db"][35:50], np.arange(15.0))
    if name == "one_grid_point":
        assert np.all(r["ebn0_db"] == 9.0)
    if name == "negative_lo_fractional_step":
        assert r["ebn0_db"].min() < -2.0 and len(np.unique(r["ebn0_db"])) == 7


# ------------------------------------------------------------------ b. trial generator, the law of its noise
def test_trial_noise_is_unit_white_gaussian(sa):
    """64 trials x 65 536 samples: (x - clean_ref) / sigma_ref per trial has mean 0, variance 1, no correlation at lags 1, 2
    and 4 nor inside the cos/sin pair of a Box-Muller draw (5 standard errors each), and its largest value over all
    4.2 M samples lies in (4.5, 5.8): the tail is there, and u1 is never 0.  Independent of the reference's Philox."""
    r = trial_reference("noise_law", False)
    x = device_trials("noise_law")
    assert np.isfinite(x).all()
    ref.assert_noise_law((x - r["clean"]) / r["sigma"][None, :], quads=True, what="trial noise")


# ------------------------------------------------------------------ c. workload generator
def test_workload_equals_the_reference_over_one_cycle(sa):
    """synth_kernel against afsk(): 70 channels, 11 s at 22 050 Hz (a 1 s lead at most and one whole cycle of six bursts),
    no noise.  Every sample under the three rules (amp alone in the scale), every gap exactly 0.0f, and the first sample of
    every burst amp cos(pi f32(dphi_mark) / 2^31): the phase starts anew.
    Measured on one MI355X: worst |x - x_ref| / amp = 1.33e-07 over this and the integer-symbol shapes below
    (MEASURED["afsk_clean"])."""
    r = afsk_reference("one_cycle")
    x = device_afsk(sa, "one_cycle")
    assert_samples_equal(x, r, MEASURED["afsk_clean"], "workload one_cycle", sigma_in_scale=False)
    assert np.all(x[r["sym_index"] < 0] == 0.0)
    assert min(len(f) for f in r["burst_first"]) >= 6 and set(np.unique(r["burst"])) == {-1, 0, 1, 2, 3, 4, 5}
    first = np.cos(np.pi * float(np.float32(ref._dphi(ref.MARK_HZ, 22050))) / 2147483648.0)
    for c, starts in enumerate(r["burst_first"]):
        assert np.all(np.abs(x[starts, c] - r["amp"][c] * first) < 4.0 * MEASURED["afsk_clean"] * r["amp"][c]), c


@pytest.mark.parametrize("rate,sps", [(22050, 42), (44100, 84), (48000, 92)])
def test_workload_with_integer_symbols(sa, ob, rate, sps):
    """8 channels with flag bit 0: symbols of 42, 84 and 92 samples, sample for sample; at 22 050 Hz channel 0's first burst
    also decodes through the oracle to the header the generator says it sent."""
    name = f"integer_{rate}"
    r = afsk_reference(name)
    assert np.all(r["sps"] == sps)
    x = device_afsk(sa, name)
    assert_samples_equal(x, r, MEASURED["afsk_clean"], f"workload {name}", sigma_in_scale=False)
    assert np.all(x[r["sym_index"] < 0] == 0.0)
    # the device's symbols are that long: the preamble's first bits are 1 1 0, so sample 2 sps of the first burst is the
    # first step at the space tone, after 2 sps steps at the mark tone (worked out here, not read from the reference's x)
    mark, space = ref._dphi(ref.MARK_HZ, rate), ref._dphi(ref.SPACE_HZ, rate)
    phase = np.float32((2 * sps * mark + space) % 2 ** 32)
    for c in range(x.shape[1]):
        start = r["burst_first"][c][0]
        assert np.array_equal(r["sym_index"][start:start + 2 * sps + 1, c], np.repeat([0, 1, 2], [sps, sps, 1]))
        want = r["amp"][c] * np.cos(np.pi * float(phase) / 2147483648.0)
        assert abs(x[start + 2 * sps, c] - want) < 4.0 * MEASURED["afsk_clean"] * r["amp"][c], c
    if rate == 22050:
        sent = sa.synth_payload(ref.AFSK_CASES[name]["seed"], 0)
        assert sent == r["payloads"][0]
        events = [e.as_tuple() for e in ob.Receiver(ob.default_config(rate)).run(np.ascontiguousarray(x[:, 0].astype(np.float32)))]
        bursts = [t[2] for t in events if t[0] == sa.LINK_BURST and t[2].startswith(b"ZCZC")]
        assert bursts and all(b.startswith(sent) for b in bursts), bursts


def test_noisy_workload_equals_the_reference_and_its_noise_is_white(sa):
    """16 channels x 65 536 samples at noise_sigma = 0.05: sample for sample against the reference's splitmix noise, and the
    noise law of test_trial_noise_is_unit_white_gaussian on (x - clean_ref) / (noise_sigma amp).
    Measured on one MI355X: worst |x - x_ref| / (amp + |sigma g|) = 1.81e-07 (MEASURED["afsk_noisy"]; this path takes __logf)."""
    r = afsk_reference("noisy")
    x = device_afsk(sa, "noisy")
    assert_samples_equal(x, r, MEASURED["afsk_noisy"], "workload noisy", sigma_in_scale=False)
    ref.assert_noise_law((x - r["clean"]) / r["sigma"][None, :], quads=False, what="workload noise")


# ------------------------------------------------------------------ d. the Eb/N0 axis, by physics
def test_ebn0_axis_by_the_error_rate_of_an_ideal_detector(sa):
    """256 trials at 4, 6 and 8 dB through noncoherent_fsk_bits with the reference's timing and text: per grid point the
    error count lies within 4 binomial standard deviations of N exp(-Eb/2N0)/2.  24 576 samples hold the whole burst of a
    header of one or two locations (93 bytes at the slowest clock would need about 33 800); of a longer one the symbols
    that lie wholly inside the buffer are counted, about 44 000 bits per point.  0.15 dB at 6 dB is about 4 standard
    deviations; a factor sqrt(2) in sigma misses by tens.
    Measured on one MI355X: z = +1.97, +0.28, -0.54 (6 432, 2 981 and 929 errors in 44 153, 43 423 and 44 334 bits)."""
    k = ref.TRIAL_CASES["ebn0_axis"]
    r = trial_reference("ebn0_axis", False)
    x = device_trials("ebn0_axis")
    n_bits = ref.whole_symbols(r, k["n_samples"])
    got = ref.noncoherent_fsk_bits(x, r["lead"], r["sps"], n_bits, k["rate"])
    rows = ref.bit_error_z_scores(got, r, n_bits)
    for db, bits, errors, z in rows:
        print(f"Eb/N0 axis: {db:4.1f} dB: {errors} errors in {bits} bits, z = {z:+.2f}")
    assert [row[0] for row in rows] == [4.0, 6.0, 8.0] and all(row[1] > 43000 for row in rows)
    assert all(abs(row[3]) < 4.0 for row in rows), rows
