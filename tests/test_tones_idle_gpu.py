"""The tone detector on the device on channels that carry nothing, and on tones that stand on an offset: the 8 000 Hz rows of
the idle matrix and of the tone-on-DC matrix (tests/helpers/tones_reference.py; tests/test_tones_idle_cpu.py holds the reference
itself to them) repeated over 130 channels, 30 blocks, in three ragged calls.  Block records bit for bit, events equal to the
reference's, no event on any idle channel and a START at sample 0 on every tone-on-DC channel; and with float capture on, no
chunk for any idle channel."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tones_reference as tr  # noqa: E402
import tone_audio_reference as ar  # noqa: E402
from test_tone_audio_gpu import BOTH, CHANNEL_MAJOR, TIME_MAJOR, assert_same_chunks, device_input  # noqa: E402

pytestmark = pytest.mark.gpu

RATE, N, BLOCKS, C = 8000, 320, 30, 130
SENTINEL = -12345.5
VARIANTS = {
    "f32-time": [(np.float32, TIME_MAJOR)] * 3,
    "i16-channel": [(np.int16, CHANNEL_MAJOR)] * 3,
    "mixed": [(np.float32, CHANNEL_MAJOR), (np.int16, TIME_MAJOR), (np.int16, CHANNEL_MAJOR)],      # test_tones_gpu.py's sequence
}


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
def idle_case():
    """(streams [130 x 9 600] float32, the kind of every channel -- 0 idle, else the tone's class --, three ragged calls, the
    reference's blocks, energies and events per channel)"""
    rows = [(0, x) for _, x in tr.idle_matrix(RATE, BLOCKS)] + [(kind, x) for _, kind, x in tr.tone_on_dc_matrix(RATE, BLOCKS)]
    assert len(rows) == 23
    kind_of = np.array([rows[c % len(rows)][0] for c in range(C)])
    x = np.stack([rows[c % len(rows)][1] for c in range(C)]).astype(np.float32)
    third = BLOCKS * N // 3
    k0 = third - np.arange(C) % 7 * 41
    k1 = third - np.arange(C) % 5 * 63
    k1[::9] = 0
    calls = [k0, k1, BLOCKS * N - k0 - k1]
    assert all(k.min() >= 0 for k in calls) and len({int(v) % N for v in k0}) > 3      # the channels' block phases differ
    vals, E = tr.blocks_f32(x, RATE, True)
    attn, wat = tr.qualify_f32(vals, RATE, E)
    events = [tr.Channel(c, N).feed(attn[c], wat[c]) for c in range(C)]
    # the reference alone: the idle channels are silent, every tone has its START at 0 and no END
    for c in range(C):
        assert events[c] == ([] if kind_of[c] == 0 else [(c, kind_of[c], tr.START, 0, 0, 0)])
    assert (kind_of == 0).sum() > 90 and (kind_of == tr.WAT).sum() >= 15 and (kind_of == tr.ATTENTION).sum() >= 15
    return x, kind_of, calls, vals, events


def by_channel(events):
    out = [[] for _ in range(C)]
    for e in events:
        out[int(e["channel"])].append(tuple(int(e[k]) for k in ("channel", "kind", "edge", "reserved", "sample_counter", "duration")))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_idle_channels_give_no_event_and_tones_on_an_offset_start(sa, idle_case, variant):
    import torch
    x, kind_of, calls, vals, ref_events = idle_case
    td = sa.ToneDetector(C, RATE)
    done = np.zeros(C, np.int64)
    got = [[] for _ in range(C)]
    events = []
    for k, (dtype, layout) in zip(calls, VARIANTS[variant]):
        want, most = td.block_counts(int(k.max()), k)
        assert np.array_equal(want, (done % N + k) // N)
        blocks = torch.full((most + 1, C, 4), SENTINEL, dtype=torch.float32, device="cuda")
        td.process(device_input(x, done, k, dtype, layout), k, layout, blocks)
        td.sync()
        b = blocks.cpu().numpy()
        for c in range(C):
            got[c].append(b[:want[c], c])
            assert np.all(b[want[c]:, c] == np.float32(SENTINEL)), f"channel {c}: a row behind its blocks was written"
        events += list(td.poll())
        done += k
    per_channel = by_channel(events)
    for c in range(C):
        mine = np.concatenate(got[c])
        assert mine.shape == vals[c].shape == (BLOCKS, 4)
        assert np.array_equal(mine.view(np.uint32), vals[c].view(np.uint32)), f"{variant}: channel {c}"
        assert per_channel[c] == ref_events[c], f"{variant}: channel {c}"
        if kind_of[c] == 0:
            assert per_channel[c] == [], f"{variant}: idle channel {c} gave an event"
        else:
            assert [(e[1], e[2], e[4]) for e in per_channel[c]] == [(kind_of[c], tr.START, 0)], f"{variant}: channel {c}"


def test_no_capture_opens_on_an_idle_channel(sa, idle_case):
    x, kind_of, calls, vals, ref_events = idle_case
    want = ar.chunks_of_calls(x, RATE, calls, BOTH, 3, 20, x.size)
    assert {c[0] for call in want for c in call} == set(np.flatnonzero(kind_of != 0).tolist())
    td = sa.ToneDetector(C, RATE)
    td.set_audio_capture(BOTH, 3, 20, x.size)
    done = np.zeros(C, np.int64)
    chunks = []
    for k in calls:
        td.process(device_input(x, done, k, np.float32, TIME_MAJOR), k, TIME_MAJOR)
        done += k
        td.sync()
        chunks.append([(int(r["channel"]), int(r["flags"]), int(r["kind"]), int(r["sample_counter"]), int(r["tone_start"]), a)
                       for r, a in td.poll_audio()])
    for call in chunks:
        for ch in call:
            assert kind_of[ch[0]] != 0, f"idle channel {ch[0]} opened a capture"
    assert_same_chunks(chunks, want, "idle")
    assert by_channel(td.poll()) == ref_events
