"""The tone detector's contract (include/same_tones.h) on channels that carry nothing, restated in numpy
(tests/helpers/tones_reference.py) and read from no library of the project.  The contract takes the block's mean out of the
energy, Em = E - S S / N, but not out of the three Goertzel sums, and 853 Hz and 960 Hz make 34.12 and 38.4 cycles in a block:
a constant leaks into P_0 and P_1.  On an idle channel Em is a few counts of noise or f32 rounding residue, and without the
guard `Em >= E / 64` every block of such a channel qualifies as ATTENTION (profiles/tone_family_reach_mutants.txt has the rows
and the counts).  Here: no block of the idle matrix qualifies for either class and none of its streams gives an event, in the
f32 form and in the float64 form, with no block left out; and a tone on an offset of up to three times its amplitude still
qualifies in every block."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402

RATES = (8000, 22050, 48000, 96000)
BLOCKS = 30
# Em / E of a tone of amplitude A on an offset of d A: (A^2 / 2) / (A^2 / 2 + d^2 A^2) for the 1050 Hz tone, and with A^2 / 4
# (two sines of A / 2) for the two-tone
SHARE = {(tr.WAT, 0.3): 0.847, (tr.WAT, 1.0): 0.333, (tr.WAT, 3.0): 0.0526,
         (tr.ATTENTION, 0.3): 0.735, (tr.ATTENTION, 1.0): 0.200, (tr.ATTENTION, 3.0): 0.0270}

_memo = {}


def forms(rate, which):
    """(names, streams [n x samples] float64, f32 values, f32 E, float64 ratios, float64 shares) of a matrix at a rate"""
    key = (rate, which)
    if key not in _memo:
        rows = tr.idle_matrix(rate, BLOCKS) if which == "idle" else [(name, x) for name, _, x in tr.tone_on_dc_matrix(rate, BLOCKS)]
        x = np.stack([r[1] for r in rows])
        vals, E = tr.blocks_f32(x.astype(np.float32), rate, True)
        _memo[key] = ([r[0] for r in rows], x, vals, E, tr.ratios_f64(x, rate), tr.share_f64(x, rate))
    return _memo[key]


def events(attn, wat, rate):
    return tr.Channel(0, tr.block_length(rate)).feed(attn, wat)


@pytest.mark.parametrize("rate", RATES)
def test_no_block_of_an_idle_channel_qualifies(rate):
    names, x, vals, E, r, share = forms(rate, "idle")
    assert vals.shape == (len(names), BLOCKS, 4) and len(names) == 17
    # int16 carries the same samples, and gives the same blocks
    v16, E16 = tr.blocks_f32(x.astype(np.int16), rate, True)
    assert np.array_equal(x.astype(np.int16).astype(np.float64), x)
    assert np.array_equal(v16.view(np.uint32), vals.view(np.uint32)) and np.array_equal(E16.view(np.uint32), E.view(np.uint32))
    a32, w32 = tr.qualify_f32(vals, rate, E)
    a64, w64 = tr.qualify_f64(r, share)
    for i, name in enumerate(names):
        what = f"{rate} Hz, {name}"
        print(f"{what}: Em / E at most {share[i].max():.3g} (f32 {np.max(vals[i, :, 3] / np.maximum(E[i], 1e-30)):.3g}), "
              f"P_0 / ref at most {r[i, :, 0].max():.3g}")
        assert not a32[i].any() and not w32[i].any(), f"{what}: f32 blocks {np.flatnonzero(a32[i] | w32[i]).tolist()} qualify"
        assert not a64[i].any() and not w64[i].any(), f"{what}: float64 blocks {np.flatnonzero(a64[i] | w64[i]).tolist()} qualify"
        assert events(a32[i], w32[i], rate) == [] and events(a64[i], w64[i], rate) == [], what
        assert tr.events_of_stream(x[i].astype(np.float32), rate) == [] and tr.events_of_stream(x[i].astype(np.int16), rate) == [], what
    # none of them is near the guard: the largest share of the matrix lies far below 1 / 64 in both forms
    assert share.max() < tr.LIVE_SHARE / 4 and np.all(vals[..., 3] <= E * np.float32(tr.LIVE_SHARE / 4))


@pytest.mark.parametrize("rate", RATES)
def test_the_matrix_would_alarm_without_the_guard(rate):
    """the matrix is not idle by construction: with the guard taken away (E = 0 makes it vacuous) most of its noisy rows qualify
    as ATTENTION in every block -- the defect the guard closes"""
    names, x, vals, E, r, share = forms(rate, "idle")
    attn, wat = tr.qualify_f32(vals, rate, np.zeros_like(E))
    full = [name for i, name in enumerate(names) if attn[i].all()]
    print(f"{rate} Hz: ATTENTION in all {BLOCKS} blocks without the guard: {full}")
    assert "500 + round(2 randn)" in full and "37 + round(0.3 randn)" in full and "30000 + round(150 randn)" in full
    assert not wat.any()                                     # 1050 Hz makes exactly 42 cycles: no leak


@pytest.mark.parametrize("rate", RATES)
def test_a_tone_on_an_offset_of_up_to_three_amplitudes_qualifies_in_every_block(rate):
    names, x, vals, E, r, share = forms(rate, "tone")
    rows = tr.tone_on_dc_matrix(rate, BLOCKS)
    assert np.abs(x).max() <= 30001 and np.abs(x).max() >= 29000
    a32, w32 = tr.qualify_f32(vals, rate, E)
    a64, w64 = tr.qualify_f64(r, share)
    N = tr.block_length(rate)
    for i, (name, kind, _) in enumerate(rows):
        what = f"{rate} Hz, {name}"
        d = tr.TONE_DC[i % 3]
        print(f"{what}: Em / E {share[i].min():.4f} .. {share[i].max():.4f}")
        # (a block holds 4.28 beats of 960 - 853 Hz: the two-tone's energy, and with it the share, moves by a few per cent
        # from block to block around the figure)
        assert np.all(np.abs(share[i] - SHARE[(kind, d)]) <= 0.1 * SHARE[(kind, d)]), what
        assert abs(share[i].mean() - SHARE[(kind, d)]) <= 0.02 * SHARE[(kind, d)], what
        for attn, wat in ((a32[i], w32[i]), (a64[i], w64[i])):
            mine, other = (wat, attn) if kind == tr.WAT else (attn, wat)
            assert mine.all() and not other.any(), what
            assert events(attn, wat, rate) == [(0, kind, tr.START, 0, 0, 0)], what
        for dtype in (np.float32, np.int16):
            assert tr.events_of_stream(x[i].astype(dtype), rate) == [(0, kind, tr.START, 0, 0, 0)], what
    assert N * BLOCKS == x.shape[1]


def test_the_limit_a_tone_on_five_or_six_amplitudes_of_offset_is_not_live():
    """the header's limit, which is no defect: at an offset of 5 A the two-tone (Em / E = 0.0099) and at 6 A the 1050 Hz tone
    (0.0137) fall below 1 / 64"""
    rate, n = 8000, 30 * 320
    for kind, d, share in ((tr.ATTENTION, 5.0, 0.0099), (tr.WAT, 6.0, 0.0137)):
        A = 30000.0 / (1.0 + d)
        x = np.round(tr.tone(kind, n, rate, A) + d * A)
        s = tr.share_f64(x, rate)
        assert np.all(np.abs(s - share) <= 0.1 * share) and abs(s.mean() - share) <= 0.02 * share and s.max() < tr.LIVE_SHARE
        vals, E = tr.blocks_f32(x.astype(np.float32), rate, True)
        attn, wat = tr.qualify_f32(vals, rate, E)
        assert not attn.any() and not wat.any()
        attn, wat = tr.qualify_f64(tr.ratios_f64(x, rate), s)
        assert not attn.any() and not wat.any()
