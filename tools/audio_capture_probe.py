"""Alert audio capture at the configs[3] shard (relaxed, 32 768 channels, messages-only, 2-s calls taken in turn from a 12-s
synthetic buffer -- long enough for the H H H ... E E E cycle to keep about a quarter of channel-time inside messages --, STEPS
calls after 3 warm-up calls): host CPU time, wall time and same_batch_last_kernel_ms per call, and the captured samples,
in four cases:
    off     capture off
    idle    capture on, zeroed input (no channel in a message)
    sparse  capture on, the synthetic workload on about 1 % of the channels, the rest zeroed
    dense   capture on, the full synthetic workload
Each call polls its events and its audio, as a server would.  The capture kernel's own time: run under
rocprofv3 --kernel-trace --stats and read capture_kernel's line.

    python tools/audio_capture_probe.py off|idle|sparse|dense STEPS
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sameold_amd as sa  # noqa: E402

mode, steps = sys.argv[1], int(sys.argv[2])
rate, n_ch, n, n_buf = 22050, 32768, 44100, 6
x = sa.synth_afsk(n_ch, n * n_buf, rate, seed=7, noise_sigma=0.05)
if mode == "idle":
    x.zero_()
elif mode == "sparse":
    import torch
    keep = torch.arange(n_ch, device=x.device) % 100 == 0       # every 100th channel
    x[:, ~keep] = 0.0
rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=True, messages_only=True)
if mode != "off":
    rx.set_audio_capture(n * n_ch // 2)
rx.set_kernel_timing(True)
cpu, wall, kms, nev, nsamp, nchunks = [], [], [], 0, 0, 0
calls = [x[k * n:(k + 1) * n] for k in range(n_buf)]
for i in range(steps + 3):
    c0, w0 = time.process_time(), time.perf_counter()
    rx.process_tensor(calls[i % n_buf])
    ev = rx.poll_events_np(1 << 24)
    au = rx.poll_audio() if mode != "off" else []
    c1, w1 = time.process_time(), time.perf_counter()
    if i >= 3:
        cpu.append((c1 - c0) * 1e3); wall.append((w1 - w0) * 1e3); kms.append(rx.last_kernel_ms()); nev += len(ev)
        nsamp += sum(len(a[3]) for a in au); nchunks += len(au)
rx.sync()
med = lambda v: sorted(v)[len(v) // 2]
print(json.dumps({"mode": mode, "steps": steps, "cpu_ms_per_call_median": med(cpu), "wall_ms_per_call_median": med(wall),
                  "wall_ms_per_call_min": min(wall), "wall_ms_per_call_max": max(wall),
                  "kernel_ms_median": med(kms), "events_per_call": nev / steps, "chunks_per_call": nchunks / steps,
                  "captured_samples_per_call": nsamp / steps, "kernel": rx.kernel_name()}))
