"""Ragged calls (same_batch_process_device_ragged) against the plain call: ms per call in steady state.

32 768 channels at 22.05 kHz, 2-s calls (44 100 rows), strict and relaxed.  Each ragged call draws fresh counts
n * (1 - U[0, j]) per channel, for j in 0, 0.01, 0.05, 0.25 (j = 0: every count n, i.e. the plain path).  The plain call
of n rows is the baseline.  Every configuration is pre-heated with 5 calls, then 20 calls are timed between two
synchronisations (same_batch_sync + torch.cuda.synchronize), so the figure includes the harvest that overlaps each launch.
One JSON line per configuration; --out FILE also writes them there.

For the ragged kernel's share, run one configuration under rocprofv3 --kernel-trace --stats, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ragged_probe.py --modes strict --js 0.25
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32768)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="strict,relaxed")
    ap.add_argument("--js", default="plain,0,0.01,0.05,0.25")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sameold_amd as sa
    sa.load_library()
    n_ch, n = a.channels, int(a.rate * a.seconds)
    x = sa.synth_afsk(n_ch, n, a.rate, seed=3, noise_sigma=0.05)
    rng = np.random.default_rng(1)
    lines = []
    for mode in a.modes.split(","):
        for js in a.js.split(","):
            rx = sa.SameReceiverBuilder(a.rate).build_batch(n_ch, relaxed=(mode == "relaxed"))
            j = None if js == "plain" else float(js)

            def one():
                if j is None:
                    rx.process_tensor(x)
                    return n, n
                k = np.floor(n * (1.0 - rng.uniform(0.0, j, n_ch))).astype(np.uint32) if j > 0 else np.full(n_ch, n, np.uint32)
                rx.process_ragged(x, k)
                return int(k.min()), int(k.max())

            for _ in range(a.warmup):
                one()
            rx.sync(); torch.cuda.synchronize()
            rx.poll_events_np()
            spans = []
            t0 = time.perf_counter()
            for _ in range(a.calls):
                spans.append(one())
            rx.sync(); torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            rx.poll_events_np()
            line = {"mode": mode, "j": js, "channels": n_ch, "rows": n, "calls": a.calls, "ms_per_call": round(ms, 3),
                    "mean_min_count": float(np.mean([s[0] for s in spans])), "mean_max_count": float(np.mean([s[1] for s in spans])),
                    "kernel": rx.kernel_name()}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del rx
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
