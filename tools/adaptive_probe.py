#!/usr/bin/env python3
"""Measurements of adaptive sampling (include/rt_api.h "adaptive sampling"), one JSON record per case, stamped with rt_build_id():

    python tools/adaptive_probe.py [--scenes demo,cornell,caustic] [--db 30] [--max-passes 256] [--reference-passes 4096] \\
                                   >> profiles/r11_adaptive.jsonl

  per scene   at 800x600, two contexts on seed streams 1 and 2: rt_render_converged to a WHOLE-FRAME target of --db against
              rt_render_adaptive to the same figure PER TILE (min_passes 16, a check every 8 passes, the same pass limit), each followed by
              rt_merge_async.  Recorded for both: wall ms from the first launch to the merged frame, samples rendered (rt_get_stats of
              both halves), checks, passes, and the PSNR of the merged frame against a --reference-passes frame of seed stream 3; for
              the adaptive run also the smallest, median and largest tile pass count.  Nothing here promises that the adaptive run
              is faster: a subset launch pays the LDS staging per workgroup like any other, every check waits for 8 bytes.
  call_costs  Demo scene, 800x600, 16 passes rendered: wall ms (median of --repeats, queued and drained) of one rt_select_tiles from a
              device map, and of one rt_render_tiles_async of 1 pass on a SINGLE group with the list build (a new selection each time)
              and without it (the same selection again)."""
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
from tools.reference_scenes import load_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="demo,cornell,caustic")
ap.add_argument("--db", type=float, default=30.0)
ap.add_argument("--max-passes", type=int, default=256)
ap.add_argument("--reference-passes", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=20)
args = ap.parse_args()
W, H, MIN_PASSES, PER_CHECK = 800, 600, 16, 8


def context(scene, stream_id):
    sph, orig, target = scene
    c = api.RtContext(W, H)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(orig, target, W, H))
    c.seed_stream(stream_id, c.stream)
    return c


def one_run(scene, truth, adaptive):
    with context(scene, 1) as a, context(scene, 2) as b:
        for x in (a, b):                                    # the first launches of a scene measure and price: not part of the figure
            x.render_pass(PER_CHECK)
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
        a.throttle(0), b.throttle(0)
        t0 = time.perf_counter()
        if adaptive:
            reached, last, checks = a.render_adaptive(b, args.db, MIN_PASSES, PER_CHECK, args.max_passes)
        else:
            reached, last, checks = a.render_converged(b, args.db, PER_CHECK, args.max_passes)
        passes = a.current_sample
        samples = a.stats()["samples"] + b.stats()["samples"]
        tiles = np.sort(a.tile_passes().reshape(-1))
        a.merge([b], a.stream)
        px = a.read_pixels()
        wall = (time.perf_counter() - t0) * 1e3
        out = {"reached": reached, "checks": checks, "passes_per_half": passes, "wall_ms": round(wall, 3), "samples_rendered": int(samples),
               "samples_of_whole_frames": 2 * W * H * passes, "last_pair_psnr_db": round(api.error_psnr(last), 3),
               "merged_vs_reference_db": round(host.psnr(px, truth), 3), "kernel": a.last_kernel}
        if adaptive:
            out["tile_passes"] = {"min": int(tiles[0]), "median": int(tiles[tiles.size // 2]), "max": int(tiles[-1])}
        return out


def scene_record(name):
    scene = (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET) if name == "demo" else load_scene(name)
    with context(scene, 3) as ref:
        truth = ref.render_pass(args.reference_passes)
    return {"record": "adaptive_vs_converged", "scene": name, "w": W, "h": H, "target_db": args.db, "min_passes": MIN_PASSES, "passes_per_check": PER_CHECK,
            "max_passes": args.max_passes, "reference_frame": "%d passes, seed stream 3" % args.reference_passes,
            "converged": one_run(scene, truth, False), "adaptive": one_run(scene, truth, True), "build_id": api.build_id()}


def call_costs():
    scene = (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET)

    def median_ms(fn, ctx):
        ms = []
        for r in range(3 + args.repeats):
            ctx.throttle(0)
            t0 = time.perf_counter()
            fn()
            ctx.throttle(0)
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 5)

    with context(scene, 1) as a:
        a.render_pass(16)
        ty, tx = a.compare_tiles()
        err = np.zeros((ty, tx), np.uint32)
        err[ty // 2, tx // 2] = 1                           # one tile above 0: its group alone
        d = api.DeviceWords(err)
        rec = {"record": "call_costs", "scene": "demo", "w": W, "h": H, "repeats": args.repeats, "build_id": api.build_id()}
        rec["select_wall_ms"] = median_ms(lambda: a.select_tiles(d.ptr, 0, a.stream), a)

        def launch_with_list():
            a.select_tiles(d.ptr, 0, a.stream)
            a.render_tiles_async(1, a.stream)
        rec["select_list_and_one_group_launch_wall_ms"] = median_ms(launch_with_list, a)
        rec["one_group_launch_wall_ms"] = median_ms(lambda: a.render_tiles_async(1, a.stream), a)
        rec["kernel"] = a.last_kernel
    return rec


for name in [s for s in args.scenes.split(",") if s]:
    print(json.dumps(scene_record(name)), flush=True)
print(json.dumps(call_costs()), flush=True)
