"""bench.py's step loop (run_steps) on a stub receiver, no GPU: W untimed passes and the pre-heat before the timed region, EXACTLY K
process calls inside it, the untimed launch the first timed pass collects kept out of the kernel-time mean, and -- N ranks -- the
number of pre-heat passes agreed through the hook (a pass of an N-rank run holds a collective: every rank must make the same number)."""
import os
import sys
import time
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StubRx:
    """Two launches in flight: a process call queues launch k and collects launch k - 1 (its events become pending)."""
    def __init__(self, log):
        self.log, self.launched, self.collected, self.pending, self.kms = log, 0, 0, 0, 0.0
    def process_device_ptr(self, ptr, T, layout, stream):
        self.launched += 1
        self.log.append(("process", self.launched))
        self._collect(self.launched - 1)
    def _collect(self, upto):
        while self.collected < upto:
            self.collected += 1
            self.pending += 10
            self.kms = float(self.collected)          # launch k "took" k ms: the mean tells which launches were counted
    def sync(self):
        self.log.append(("sync", self.launched)); self._collect(self.launched)
    def pending_events(self): return self.pending
    def last_kernel_ms(self): return self.kms
    def last_demod_kernel_ms(self): return self.kms
    def peek_events_np(self):
        self.log.append(("peek", self.collected))
        ev = np.zeros(self.pending, dtype=[("sample_counter", "<u8"), ("kind", "<u4")]); ev["sample_counter"] = 1
        return ev
    def drop_events(self, n): self.pending -= n
    def input_sample_counter(self): return 0


@pytest.mark.parametrize("steps,warmup,preheat", [(20, 5, 30.0), (20, 3, 0.0), (4, 1, 0.0), (3, 0, 0.0), (5, 2, 10.0)])
def test_run_steps_times_exactly_k_passes(monkeypatch, steps, warmup, preheat):
    import torch
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    log, agreed = [], []
    rx = StubRx(log)
    sa = types.SimpleNamespace(receiver=types.SimpleNamespace(EVENT_DTYPE=np.dtype([("sample_counter", "<u8"), ("kind", "<u4")])))
    x = types.SimpleNamespace(data_ptr=lambda: 0)
    monkeypatch.setattr(bench, "PREHEAT_MS", [preheat])
    def agree(v):
        agreed.append(v); return v
    monkeypatch.setattr(bench, "AGREE", [agree])
    gathered = []
    def barrier(): log.append(("barrier", rx.launched))
    el, kms, first_ev, nb, steady = bench.run_steps(sa, rx, x, 100, None, steps, warmup, lambda r: gathered.append(r.pending_events()) or 0, barrier)
    marks = [n for what, n in log if what == "barrier"]
    assert len(marks) == 2 and marks[1] - marks[0] == steps                      # exactly K launches between the two barriers
    untimed = marks[0]
    assert untimed >= warmup                                                      # W warm-up passes (+ the pre-heat's) before the first
    if preheat > 0.0:
        assert (untimed - warmup) % 8 == 0 and len(agreed) == (untimed - warmup) // 8    # pre-heat in agreed chunks of eight passes
    else:
        assert untimed == warmup and not agreed
    # the kernel times counted are those of the K timed launches (launch k "took" k ms), not the untimed one the first pass collected
    assert kms == pytest.approx(np.mean(np.arange(untimed + 1, untimed + steps + 1)))
    assert sum(1 for what, _ in log if what == "peek") == 1                       # only the first pass's events are materialised
    assert bench.run_steps.last_launches == untimed + steps
    assert rx.pending == 0 and rx.collected == rx.launched                        # everything collected and consumed inside the region


def test_preheat_pass_count_follows_the_slowest_rank(monkeypatch):
    """The ranks stop pre-heating together: the hook returns the maximum over the ranks, so a rank whose own clock says
    "enough" goes on while another's does not."""
    import torch
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    rx = StubRx([])
    sa = types.SimpleNamespace(receiver=types.SimpleNamespace(EVENT_DTYPE=np.dtype([("sample_counter", "<u8"), ("kind", "<u4")])))
    x = types.SimpleNamespace(data_ptr=lambda: 0)
    calls = []
    def agree(v):
        calls.append(v)
        return 0.0 if len(calls) < 4 else 1e9          # "another rank" is not done for three rounds
    monkeypatch.setattr(bench, "PREHEAT_MS", [5.0])
    monkeypatch.setattr(bench, "AGREE", [agree])
    bench.run_steps(sa, rx, x, 100, None, 2, 1, lambda r: 0, lambda: None)
    assert len(calls) == 4 and bench.run_steps.last_launches == 1 + 4 * 8 + 2


EVENT_DTYPE = np.dtype([("kind", "<u4"), ("channel", "<u4"), ("sample_counter", "<u8"), ("symbol_count", "<u8"),
                        ("len", "<u4"), ("aux", "<u4"), ("aux2", "<u4"), ("reserved", "<u4"), ("bytes", "u1", (288,))])   # sameold_amd.receiver's


class CountingRx(StubRx):
    """StubRx whose launches carry samples: launch k covers samples ((k - 1) T, k T], each of its events on a channel of its own."""
    T = 100
    def __init__(self, log):
        super().__init__(log)
        self.queue = []
    def _collect(self, upto):
        while self.collected < upto:
            self.collected += 1
            k = self.collected
            for c in range(10):
                self.queue.append((c, (k - 1) * self.T + 1 + c, 3 if c % 2 else 1, 7 + k, c % 4))
            self.pending = len(self.queue)
            self.kms = float(k)
    def peek_events_np(self):
        self.log.append(("peek", self.collected))
        ev = np.zeros(len(self.queue), dtype=EVENT_DTYPE)
        for i, (c, t, kind, sym, n) in enumerate(self.queue):
            ev[i]["channel"], ev[i]["sample_counter"], ev[i]["kind"], ev[i]["symbol_count"], ev[i]["len"] = c, t, kind, sym + c, n
            ev[i]["bytes"][:n] = np.arange(1, n + 1) + c
        return ev
    def drop_events(self, n):
        del self.queue[:n]
        self.pending = len(self.queue)
    def input_sample_counter(self): return self.launched * self.T


@pytest.mark.parametrize("steps,warmup,preheat", [(20, 5, 10.0), (1, 0, 0.0), (3, 2, 0.0)])
def test_run_steps_keeps_the_last_timed_launch(monkeypatch, steps, warmup, preheat):
    """--dump-outputs: the events of the LAST timed launch, counted from the start of its call, and still exactly K timed launches
    with the whole queue consumed."""
    import torch
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(bench, "PREHEAT_MS", [preheat])
    monkeypatch.setattr(bench, "AGREE", [lambda v: v])
    log = []
    rx = CountingRx(log)
    sa = types.SimpleNamespace(receiver=types.SimpleNamespace(EVENT_DTYPE=EVENT_DTYPE))
    x = types.SimpleNamespace(data_ptr=lambda: 0)
    def barrier(): log.append(("barrier", rx.launched))
    bench.run_steps(sa, rx, x, CountingRx.T, None, steps, warmup, lambda r: 0, barrier, keep_last=True)
    marks = [n for what, n in log if what == "barrier"]
    assert marks[1] - marks[0] == steps and rx.launched == marks[1]
    last = bench.run_steps.last_events
    assert len(last) == 10 and list(last["channel"]) == list(range(10))
    assert list(last["sample_counter"]) == [1 + c for c in range(10)]             # from the start of the last call
    assert list(last["symbol_count"]) == [7 + rx.launched + c for c in range(10)]  # (launch k's events carry 7 + k)
    assert rx.pending == 0 and rx.collected == rx.launched
    bench.run_steps(sa, CountingRx([]), x, CountingRx.T, None, steps, warmup, lambda r: 0, lambda: None)
    assert bench.run_steps.last_events is None


def test_dump_outputs_files(tmp_path):
    """What --dump-outputs writes: float arrays only, the same for the same events, a seeded channel sample above the limit."""
    import bench
    ev = np.zeros(12, dtype=EVENT_DTYPE)
    ev["channel"] = [5, 1, 1, 9000, 5, 1, 2, 3, 4, 6, 7, 8]
    ev["sample_counter"] = [9, 4, 2, 1, 3, 8, 1, 1, 1, 1, 1, 1]
    ev["symbol_count"] = [50, 41, 40, 9, 42, 43, 1, 1, 1, 1, 1, 1]
    ev["kind"] = 3
    ev["len"] = [3, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    ev["bytes"][:, :3] = [[1, 2, 3]] * 12
    a = bench.dump_outputs(str(tmp_path / "a"), ev, 16)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in a)
    for n in a:
        got = np.load(tmp_path / "a" / (n + ".npy"))
        assert got.dtype in (np.float32, np.float64) and np.array_equal(got, a[n])
    assert list(a["event_channel"][:4]) == [1, 1, 1, 2] and list(a["event_sample_offset"][:3]) == [2, 4, 8]
    assert list(a["event_symbol_offset"][:3]) == [0, 1, 3]
    assert list(a["event_payload"]) == [1, 2, 1, 2, 3]          # channel 1's event at sample 2, then channel 5's at sample 9
    assert 9000 not in a["event_channel"] and len(a["channels"]) == 16
    # above the channel limit: a seeded sample, the same every time, and only events of sampled channels
    b1 = bench.dump_outputs(str(tmp_path / "b1"), ev, 3 * bench.DUMP_MAX_CHANNELS)
    b2 = bench.dump_outputs(str(tmp_path / "b2"), ev[::-1].copy(), 3 * bench.DUMP_MAX_CHANNELS)
    assert len(b1["channels"]) == bench.DUMP_MAX_CHANNELS
    assert all(np.array_equal(b1[n], b2[n]) for n in b1)
    assert set(b1["event_channel"]) <= set(b1["channels"])
