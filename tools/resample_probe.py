"""The mixed-rate resampler (include/same_resample.h) in steady state: ms per call.

32 768 channels, 2-s calls, a strict 22.05 kHz batch behind the resampler.  Three inputs: every channel a 48 kHz source, every
channel an 8 kHz source, and the seven rates 48 / 44.1 / 22.05 / 16 / 8 / 11.025 / 32 kHz interleaved channel by channel (every
wavefront mixes every ratio).  The sources are the synthetic 22.05 kHz workload taken to each source rate on the device by a
resampler of its own, so the batch demodulates the signal the plain call does.  Per input, each pre-heated with 5 calls and
then timed over 20 calls between two synchronisations:
  - resampler_ms: Resampler.process alone into a buffer that is reused (its three kernels and the descriptor copy);
  - process_ms:   MixedRateReceiver.process (resampling, the fresh output tensor, the batch's ragged call and its harvest);
and beside them plain_ms, the same batch kind's plain 2-s call on the 22.05 kHz signal.  bytes: the source samples the
resampler reads plus the output samples it writes (taps and history not counted).  One JSON line per input; --out FILE also
writes them there.

--sources adds the per-source call beside the time-major one, on the same samples: every channel's samples a
contiguous slice of one allocation, handed over through Resampler.process_source_ptrs, a handle of its own, the same
protocol.  sources_ms / sources_GBps are its resampler_ms / resampler_GBps; outputs_equal says that the two handles' last
outputs are the same bits; sources_process_ms is MixedRateReceiver.process_sources on one tensor per channel.

For the kernels' own time, run one input under rocprofv3 --kernel-trace --stats, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/resample_probe.py --inputs mix --only-resampler
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIX = [48000, 44100, 22050, 16000, 8000, 11025, 32000]
OUT_RATE = 22050


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32768)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inputs", default="48000,8000,mix")
    ap.add_argument("--i16", action="store_true", help="int16 sources (default float32)")
    ap.add_argument("--only-resampler", action="store_true")
    ap.add_argument("--sources", action="store_true", help="also time the per-source call on the same samples")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sameold_amd as sa
    sa.load_library()
    n_ch, n22 = a.channels, int(OUT_RATE * a.seconds)
    base = sa.synth_afsk(n_ch, n22, OUT_RATE, seed=3, noise_sigma=0.05)

    def source_at(rate):
        """the 22.05 kHz workload as a source at `rate`: [rate * seconds, C] float32"""
        if rate == OUT_RATE:
            return base
        up = sa.Resampler([OUT_RATE] * n_ch, rate)
        y, _ = up.process(base, np.full(n_ch, n22, np.uint32))
        torch.cuda.synchronize()
        return y[: int(rate * a.seconds)]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    lines = []
    plain_ms = None
    if not a.only_resampler:
        rx = sa.SameReceiverBuilder(OUT_RATE).build_batch(n_ch)

        def plain():
            rx.process_tensor(base)

        for _ in range(a.warmup):
            plain()
        rx.sync(); torch.cuda.synchronize()
        rx.poll_events_np()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            plain()
        rx.sync(); torch.cuda.synchronize()
        plain_ms = (time.perf_counter() - t0) * 1e3 / a.calls
        rx.poll_events_np()
        kernel = rx.kernel_name()
        del rx
    for name in a.inputs.split(","):
        rates = [MIX[c % 7] for c in range(n_ch)] if name == "mix" else [int(name)] * n_ch
        counts = np.array([int(r * a.seconds) for r in rates], np.uint32)
        n_rows = int(counts.max())
        x = torch.zeros((n_rows, n_ch), dtype=torch.float32, device="cuda")
        for r in sorted(set(rates)):
            cols = torch.tensor([c for c in range(n_ch) if rates[c] == r], device="cuda")
            src = source_at(r)
            x[: src.shape[0], cols] = src[:, cols]
            del src
        if a.i16:
            x = x.round().clamp(-32768, 32767).to(torch.int16)
        rs = sa.Resampler(rates, OUT_RATE)
        out, rows = rs.out_counts(counts)
        y = torch.zeros((rows + 1, n_ch), dtype=torch.float32, device="cuda")
        resampler_ms = timed(lambda: rs.process(x, counts, y))
        line = {"input": name, "channels": n_ch, "rows": n_rows, "sample": "i16" if a.i16 else "f32", "calls": a.calls,
                "resampler_ms": round(resampler_ms, 3),
                "bytes": int(counts.astype(np.int64).sum()) * (2 if a.i16 else 4) + int(out.astype(np.int64).sum()) * 4}
        line["resampler_GBps"] = round(line["bytes"] / resampler_ms / 1e6, 1)
        del rs
        if a.sources:
            # channel c's samples at flat[off[c] : off[c] + counts[c]]
            off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
            flat = torch.empty(int(off[-1]), dtype=x.dtype, device="cuda")
            for r in sorted(set(rates)):
                cols = np.array([c for c in range(n_ch) if rates[c] == r])
                n_r = int(r * a.seconds)
                for lo in range(0, len(cols), 1024):
                    part = cols[lo:lo + 1024]
                    idx = torch.from_numpy(off[part]).cuda()[:, None] + torch.arange(n_r, device="cuda")[None, :]
                    flat[idx] = x[:n_r, torch.from_numpy(part).cuda()].T
                    del idx
            ptrs = np.uint64(flat.data_ptr()) + off[:-1].astype(np.uint64) * np.uint64(flat.element_size())
            rs = sa.Resampler(rates, OUT_RATE)
            ys = torch.zeros_like(y)
            stream = torch.cuda.current_stream().cuda_stream
            sources_ms = timed(lambda: rs.process_source_ptrs(ptrs, counts, ys.data_ptr(), ys.shape[0], stream, a.i16))
            line["sources_ms"] = round(sources_ms, 3)
            line["sources_GBps"] = round(line["bytes"] / sources_ms / 1e6, 1)
            line["outputs_equal"] = bool(torch.equal(y.view(torch.int32), ys.view(torch.int32)))
            del rs, ys
        del y
        if not a.only_resampler:
            mr = sa.MixedRateReceiver(sa.SameReceiverBuilder(OUT_RATE), rates)
            for _ in range(a.warmup):
                mr.process(x, counts)
            mr.sync(); torch.cuda.synchronize()
            mr.poll_events_np()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                mr.process(x, counts)
            mr.sync(); torch.cuda.synchronize()
            line["process_ms"] = round((time.perf_counter() - t0) * 1e3 / a.calls, 3)
            line["events"] = int(len(mr.poll_events_np()))
            line["plain_ms"] = round(plain_ms, 3)
            line["kernel"] = kernel
            del mr
            if a.sources:
                mr = sa.MixedRateReceiver(sa.SameReceiverBuilder(OUT_RATE), rates)
                srcs = [flat[off[c]:off[c + 1]] for c in range(n_ch)]
                for _ in range(a.warmup):
                    mr.process_sources(srcs)
                mr.sync(); torch.cuda.synchronize()
                mr.poll_events_np()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    mr.process_sources(srcs)
                mr.sync(); torch.cuda.synchronize()
                line["sources_process_ms"] = round((time.perf_counter() - t0) * 1e3 / a.calls, 3)
                line["sources_events"] = int(len(mr.poll_events_np()))
                del mr, srcs
        if a.sources:
            del flat
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
