"""The tone detector (include/same_tones.h) in steady state: ms per call of the tone pass.

22.05 kHz, the synthetic AFSK workload, at 32 768 channels x 2-s calls and 4 096 channels x 10-s calls; both layouts; f32 and
int16.  Per combination, pre-heated with --warmup calls and then timed over --calls calls between two synchronisations (the
detector's own sync included, so the copy of the event slots and their harvest are inside):
  - tones_ms:    ToneDetector.process alone (descriptor copy, block kernel, state-machine kernel, event-slot copy);
  - share_of_hbm_peak: bytes / tones_ms over 8 TB/s, bytes = the samples read once (descriptors and event slots not counted);
  - relaxed_ms:  the relaxed batch's own call on the same buffer in the same run, its sync and event poll included.
One JSON line per combination; --out FILE also writes them there.

--capture measures tone-alert audio (include/same_tone_audio.h) instead: whole-call times by the same
protocol, of variants alternated in one run, --repeats times each for the spread.  At 32 768 channels x 2 s, both layouts, f32
and int16: a handle with capture off ("off"), one with capture on and nothing open ("quiet": the AFSK workload holds no tone),
one with a 1050 Hz tone on every 64th channel ("one_in_64", capture off and on).  At 4 096 x 2 s: the tone on every channel
("all", capture off and on).  Each handle is first fed 2 s of its input, so that its captures are open (max_blocks is out of
reach) and every timed call copies every row of its tone channels, on the device and then to the host: a call's time has its
process call and a same_tone_audio_peek / same_tone_audio_drop of what has arrived, the samples' way to the host included.

--delivery measures the delivery form (include/same_tone_delivery.h) by the same protocol and beside the same
variants, alternated in the same run: "one_in_64_delivery" / "all_delivery" is a handle set with same_tone_delivery_set at
--out-rate (8 000 Hz), gain 1, and the same samples_per_call as the float capture.  bytes_to_host_per_call: what the last timed
call's chunks hold, 4 bytes per float sample, 2 per delivered one (chunks are packed: there is no padding).

For the kernels' own time, run one combination under rocprofv3 --kernel-trace --stats, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tones_probe.py --shapes 32768x2 --layouts time --samples f32 --no-batch
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tones_probe.py --capture --shapes 4096x2 --layouts time --samples f32 --repeats 1
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/tones_probe.py --delivery --shapes 4096x2 --layouts time --samples f32 --repeats 1
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
    ap.add_argument("--capture", action="store_true", help="measure tone-alert audio instead (see above)")
    ap.add_argument("--delivery", action="store_true", help="as --capture, with the delivery form beside the float capture")
    ap.add_argument("--out-rate", type=int, default=8000)
    ap.add_argument("--repeats", type=int, default=3)
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
    if a.delivery:
        a.capture = True
    if a.capture:
        import ctypes
        import math
        import numpy as np
        for shape in (a.shapes if a.shapes != ap.get_default("shapes") else "32768x2,4096x2").split(","):
            n_ch, seconds = (int(v) for v in shape.split("x"))
            n = RATE * seconds
            quiet = sa.synth_afsk(n_ch, n, RATE, seed=3, noise_sigma=0.05)          # [n, C] float32
            # a 1050 Hz tone that is continuous from call to call (n is a whole number of seconds)
            tone = (8000.0 * torch.sin(2.0 * math.pi * 1050.0 / RATE * torch.arange(n, dtype=torch.float64, device="cuda"))).round().to(torch.float32)
            every = 64 if n_ch > 4096 else 1
            loud = quiet.clone()
            loud[:, ::every] = tone[:, None]
            captured = (n_ch + every - 1) // every * n
            for layout_name in a.layouts.split(","):
                layout = sa.LAYOUT_TIME_MAJOR if layout_name == "time" else sa.LAYOUT_CHANNEL_MAJOR
                for sample in a.samples.split(","):
                    def tensor(base):
                        x = base if layout == sa.LAYOUT_TIME_MAJOR else base.T.contiguous()
                        return x.round().clamp(-32768, 32767).to(torch.int16) if sample == "i16" else x
                    xq, xl = tensor(quiet), tensor(loud)
                    name = "one_in_64" if every == 64 else "all"
                    variants = ([("off", xq, False), ("quiet", xq, True)] if every == 64 else []) + [(name + "_off", xl, False), (name + "_on", xl, True)]
                    if a.delivery:
                        variants.append((name + "_delivery", xl, "delivery"))
                    times = {v[0]: [] for v in variants}
                    chunks, to_host = {}, {}
                    for _ in range(a.repeats):
                        for vname, x, on in variants:              # alternated: every repeat runs every variant
                            td = sa.ToneDetector(n_ch, RATE)
                            deliver = on == "delivery"
                            if deliver:
                                td.set_audio_delivery(sa.TONE_WAT | sa.TONE_ATTENTION, 3, 1 << 30, captured, a.out_rate)
                            elif on:
                                td.set_audio_capture(sa.TONE_WAT | sa.TONE_ATTENTION, 3, 1 << 30, captured)
                            td.process(x, None, layout)            # (the tone is confirmed: captures are open from here on)
                            td.sync()
                            td.poll_audio()
                            td.poll_delivery()
                            peek = td._L.same_tone_delivery_peek if deliver else td._L.same_tone_audio_peek
                            drop = td._L.same_tone_delivery_drop if deliver else td._L.same_tone_audio_drop
                            rec = sa.TONE_DELIVERY_CHUNK_DTYPE if deliver else sa.TONE_AUDIO_CHUNK_DTYPE

                            def take():                            # the chunks that have arrived leave the queue, uncopied
                                ptr, k = ctypes.c_void_p(), ctypes.c_size_t()
                                assert peek(td._h, ctypes.byref(ptr), ctypes.byref(k)) == 0
                                if k.value:
                                    recs = np.frombuffer((ctypes.c_char * (k.value * rec.itemsize)).from_address(ptr.value), dtype=rec)
                                    chunks[vname] = int(recs["n_samples"].sum()) // max(1, len(set(recs["sample_counter"].tolist())))
                                    to_host[vname] = chunks[vname] * (2 if deliver else 4)
                                    assert drop(td._h, k.value) == 0

                            def call():
                                td.process(x, None, layout)
                                if on:
                                    take()

                            def drain():
                                td.sync()
                                if on:
                                    take()
                            times[vname].append(round(timed(call, drain), 3))
                            del td
                    line = {"channels": n_ch, "seconds": seconds, "layout": layout_name, "sample": sample, "calls": a.calls,
                            "ms": times, "captured_samples_of_the_last_call": chunks, "bytes_to_host_per_call": to_host,
                            "copy_bytes_per_call": {name: captured * ((2 if sample == "i16" else 4) + 4)}}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del xq, xl
            del quiet, loud
    for shape in ([] if a.capture else a.shapes.split(",")):
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
