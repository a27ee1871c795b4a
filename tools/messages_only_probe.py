"""The configs[3] shard (relaxed, 32 768 channels, one synthetic 2-s buffer streamed as STEPS calls after 3 warm-up calls): host
CPU time per call, wall time per call and same_batch_last_kernel_ms, without the flag or with SAME_BATCH_MESSAGES_ONLY.

    SAME_DEBUG=1 SAME_HOST_THREADS=1 python tools/messages_only_probe.py flagless|mo STEPS
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sameold_amd as sa  # noqa: E402

mode, steps = sys.argv[1], int(sys.argv[2])
rate, n_ch, n = 22050, 32768, 44100
x = sa.synth_afsk(n_ch, n, rate, seed=7, noise_sigma=0.05)
rx = sa.SameReceiverBuilder(rate).build_batch(n_ch, relaxed=True, messages_only=(mode == "mo"))
rx.set_kernel_timing(True)
cpu, wall, kms, nev = [], [], [], 0
for i in range(steps + 3):
    c0, w0 = time.process_time(), time.perf_counter()
    rx.process_tensor(x)
    ev = rx.poll_events_np(1 << 24)
    c1, w1 = time.process_time(), time.perf_counter()
    if i >= 3:
        cpu.append((c1 - c0) * 1e3); wall.append((w1 - w0) * 1e3); kms.append(rx.last_kernel_ms()); nev += len(ev)
rx.sync()
med = lambda v: sorted(v)[len(v) // 2]
print(json.dumps({"mode": mode, "steps": steps, "cpu_ms_per_call_median": med(cpu), "wall_ms_per_call_median": med(wall),
                  "kernel_ms_median": med(kms), "kernel_ms_min": min(kms), "events_per_call": nev / steps,
                  "transport_on_device": rx.transport_on_device(), "kernel": rx.kernel_name()}))
