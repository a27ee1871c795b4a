"""The tone detector (include/same_tones.h) in steady state: ms per call of the tone pass.

22.05 kHz, the synthetic AFSK workload, at 32 768 channels x 2-s calls and 4 096 channels x 10-s calls; both layouts; f32 and
int16.  Per combination, pre-heated with --warmup calls and then timed over --calls calls between two synchronisations (the
detector's own sync included, so the copy of the event slots and their harvest are inside):
  - tones_ms:    ToneDetector.process alone (descriptor copy, block kernel, state-machine kernel, event-slot copy);
  - share_of_hbm_peak: bytes / tones_ms over 8 TB/s, bytes = the samples read once (descriptors and event slots not counted);
  - relaxed_ms:  the relaxed batch's own call on the same buffer in the same run, its sync and event poll included.
One JSON line per combination; --out FILE also writes them there.

For the kernels' own time, run one combination under rocprofv3 --kernel-trace --stats, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tones_probe.py --shapes 32768x2 --layouts time --samples f32 --no-batch
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE = 22050
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768x2,4096x10", help="CHANNELSxSECONDS,...")
    ap.add_argument("--layouts", default="time,channel")
    ap.add_argument("--samples", default="f32,i16")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true", help="leave out the relaxed batch's call")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sameold_amd as sa
    sa.load_library()
    assert torch.cuda.is_available(), "the probe measures on the GPU or not at all"

    def timed(fn, sync):
        for _ in range(a.warmup):
            fn()
        sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    lines = []
    for shape in a.shapes.split(","):
        n_ch, seconds = (int(v) for v in shape.split("x"))
        n = RATE * seconds
        base = sa.synth_afsk(n_ch, n, RATE, seed=3, noise_sigma=0.05)          # [n, C] float32
        for layout_name in a.layouts.split(","):
            layout = sa.LAYOUT_TIME_MAJOR if layout_name == "time" else sa.LAYOUT_CHANNEL_MAJOR
            for sample in a.samples.split(","):
                x = base if layout == sa.LAYOUT_TIME_MAJOR else base.T.contiguous()
                if sample == "i16":
                    x = x.round().clamp(-32768, 32767).to(torch.int16)
                torch.cuda.synchronize()
                td = sa.ToneDetector(n_ch, RATE)
                tones_ms = timed(lambda: td.process(x, None, layout), td.sync)
                n_events = int(len(td.poll()))
                del td
                nbytes = n_ch * n * (2 if sample == "i16" else 4)
                line = {"channels": n_ch, "seconds": seconds, "layout": layout_name, "sample": sample, "calls": a.calls,
                        "tones_ms": round(tones_ms, 3), "bytes": nbytes, "tones_GBps": round(nbytes / tones_ms / 1e6, 1),
                        "share_of_hbm_peak": round(nbytes / (tones_ms * 1e-3) / HBM_PEAK, 4), "tone_events": n_events}
                if not a.no_batch:
                    rx = sa.SameReceiverBuilder(RATE).build_batch(n_ch, relaxed=True)

                    def drain():
                        rx.sync()
                        rx.poll_events_np()

                    line["relaxed_ms"] = round(timed(lambda: rx.process_tensor(x, layout), drain), 3)
                    line["relaxed_kernel"] = rx.kernel_name()
                    del rx
                print(json.dumps(line), flush=True)
                lines.append(line)
                del x
        del base
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
