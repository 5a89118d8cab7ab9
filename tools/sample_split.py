#!/usr/bin/env python3
"""Two measurements of the render-state calls (include/rt_api.h "render state"), one JSON record each:

    python tools/sample_split.py [--repeats 12] >> profiles/rNN_sample_split.jsonl

  sample_split   the Demo scene at the reference's 800x600 window, 64 passes: ONE context against 2 x 32 and 4 x 16 passes on contexts
                 that run at once, each on its own rt_stream and its own seed stream (1 .. K), then rt_merge_async into the first and
                 rt_read_pixels_async.  A small grid leaves wave slots empty; K grids of the full size in pixels fill them by count.
                 Wall time from the first call of the frame to the drained read-back (rt_throttle(ctx, 0)), median of the repeats
                 after five warm-up frames (the small-scene probe of cooperative any-hit takes four launches); PSNR of each form's
                 frame against one 1024-pass frame of the default stream.
                 A split frame is a correct rendering that reproduces no reference frame: its passes come from K seed streams.
  reseed         rt_seed_stream_async(k) + 64 passes against rt_reset_async + 64 passes at 1080p, the same protocol, and the two
                 calls alone (queued and drained, nothing rendered): what the 16.6 MB the seed kernel writes cost.
HIP gives a process GPU_MAX_HW_QUEUES hardware queues (4 unless set); the four contexts of the 4 x 16 form need all four."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=12)
args = ap.parse_args()
WARM = 5
sph = host.demo_scene()


def context(w, h, cam):
    c = api.RtContext(w, h)
    c.set_scene(sph)
    c.set_camera(cam)
    return c


def timed(frame, repeats):
    """Median and spread (ms) of `frame()` -- which must return drained -- over `repeats` calls after WARM warm-up calls."""
    ms = []
    for r in range(WARM + repeats):
        t0 = time.perf_counter()
        frame(r)
        if r >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": repeats}


def sample_split():
    w, h, spp = 800, 600, 64
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    with context(w, h, cam) as ref:
        truth = ref.render_pass(1024)
        ref.reset()
        default_64 = ref.render_pass(spp)
    rec = {"record": "sample_split", "scene": "demo", "w": w, "h": h, "spp": spp, "reference_frame": "1024 passes, default stream",
           "psnr_default_stream_64": round(host.psnr(default_64, truth), 3), "forms": {},
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)"), "build_id": api.build_id()}
    for k in (1, 2, 4):
        ctxs = [context(w, h, cam) for _ in range(k)]
        out = np.zeros(w * h, np.uint32)
        dst = ctxs[0]
        dst.pin_output(out)
        dst.throttle(0)                                     # (switches the bookkeeping on: from now on it drains)
        if k > 1:
            for c in ctxs:
                c.set_pixel_write(False)                    # nobody looks at a part's frame: the merged plane is packed once

        def frame(_r):
            for i, c in enumerate(ctxs):
                c.seed_stream(i + 1, c.stream)
                c.render_async(spp // k, c.stream)
            if k > 1:
                dst.merge(ctxs[1:], dst.stream)
            dst.read_pixels_async(out, dst.stream)
            dst.throttle(0)

        t = timed(frame, args.repeats)
        assert dst.current_sample == spp
        t["contexts"], t["passes_each"] = k, spp // k
        t["psnr_vs_reference_frame"] = round(host.psnr(out, truth), 3)
        t["kernel"] = dst.last_kernel
        rec["forms"]["%dx%d" % (k, spp // k)] = t
        dst.pin_output(None)
        for c in ctxs:
            c.close()
    one = rec["forms"]["1x64"]["median_ms"]
    for name, t in rec["forms"].items():
        t["vs_one_context"] = round(t["median_ms"] / one, 4)
    return rec


def reseed():
    w, h, spp = 1920, 1080, 64
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    rec = {"record": "reseed", "scene": "demo", "w": w, "h": h, "spp": spp, "seed_bytes": 8 * w * h, "build_id": api.build_id()}
    with context(w, h, cam) as c:
        c.throttle(0)

        def frame_reset(_r):
            c.reset_async(c.stream)
            c.render_async(spp, c.stream)
            c.throttle(0)

        def frame_seeded(r):
            c.seed_stream(r + 1, c.stream)
            c.render_async(spp, c.stream)
            c.throttle(0)

        def only_reset(_r):
            c.reset_async(c.stream)
            c.throttle(0)

        def only_seeded(r):
            c.seed_stream(r + 1, c.stream)
            c.throttle(0)

        rec["reset_async_then_render"] = timed(frame_reset, args.repeats)
        rec["seed_stream_async_then_render"] = timed(frame_seeded, args.repeats)
        rec["reset_async_then_render_again"] = timed(frame_reset, args.repeats)       # (A, B, A: drift shows as A != A)
        rec["reset_async_alone"] = timed(only_reset, 4 * args.repeats)
        rec["seed_stream_async_alone"] = timed(only_seeded, 4 * args.repeats)
    rec["frame_difference_ms"] = round(rec["seed_stream_async_then_render"]["median_ms"] -
                                       0.5 * (rec["reset_async_then_render"]["median_ms"] + rec["reset_async_then_render_again"]["median_ms"]), 4)
    rec["call_difference_ms"] = round(rec["seed_stream_async_alone"]["median_ms"] - rec["reset_async_alone"]["median_ms"], 4)
    return rec


for make in (sample_split, reseed):
    print(json.dumps(make()), flush=True)
