#!/usr/bin/env python3
"""Host cost of the launch path where it runs most often: 2000 queued rt_render_async(ctx, 1) calls on the Demo scene at 200x120, then one blocking
read -- six rounds with a reset between; round 0 holds the measurement of cooperative any-hit against plain and is not counted.  Prints one JSON line:
the host time of the 2000 calls per round, its median over rounds 1 to 5, and the same with the wait for the frame (profiles/HISTORY.md r23, r29).

    python tools/pass_per_call_probe.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402

W, H, CALLS, ROUNDS = 200, 120, 2000, 6


def main():
    queue, total = [], []
    with api.RtContext(W, H) as ctx:
        ctx.set_scene(host.demo_scene())
        ctx.set_camera(host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, W, H))
        for _ in range(ROUNDS):
            ctx.reset()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                ctx.render_async(1)
            t1 = time.perf_counter()
            ctx.read_pixels()
            t2 = time.perf_counter()
            queue.append((t1 - t0) * 1e3)
            total.append((t2 - t0) * 1e3)
        kernel = ctx.last_kernel
    print(json.dumps({"build_id": api.build_id(), "kernel": kernel, "calls": CALLS, "queue_ms_per_round": [round(v, 3) for v in queue],
                      "queue_ms_median_of_rounds_1_to_5": round(statistics.median(queue[1:]), 3),
                      "with_wait_ms_median_of_rounds_1_to_5": round(statistics.median(total[1:]), 3)}), flush=True)


if __name__ == "__main__":
    main()
