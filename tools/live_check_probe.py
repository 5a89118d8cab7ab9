#!/usr/bin/env python3
"""What a check of the filtered adaptive loop costs when it filters only the groups still rendering (include/rt_api.h
rt_denoise_pair_tiles_async, rt_render_adaptive_filtered_tiles), one JSON record per case, stamped with rt_build_id():

    python tools/live_check_probe.py [--runs 12] [--sizes 800x600,1920x1080] >> profiles/r15_live_checks.jsonl

  kernel  the Demo scene, two contexts on seed streams 1 and 2 with --passes passes each, the default filter parameters.  Device time between
          two HIP events on the first context's stream, the device idle before the first event: rt_denoise_pair_async (variance kernel and pair
          kernel over the frame), and rt_denoise_pair_tiles_async (variance kernel over the frame, pair kernel over the selected groups; the
          list of groups is built in the warm-up runs) with all, one half, one quarter and one eighth of the groups selected by a hand-made error
          map -- the first n / k groups in raster order from the bottom row.  Before every timed refresh one pass on the selected groups of both
          contexts, outside the events, puts the planes one selection behind.  3 runs to warm up, then the median, smallest and largest of --runs.
  loop    wall time of rt_render_adaptive_filtered and of rt_render_adaptive_filtered_tiles with identical arguments, in this process, on this
          library, the two alternating, each on contexts freshly put back to pass 0 of their seed streams; 2 runs each to warm up, then --runs.
          Beside it the number of checks and the live groups per check, counted once by the same loop written with the public calls.
No time is an acceptance criterion of anything: the records say what was measured."""
import argparse
import ctypes as C
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
ap.add_argument("--passes", type=int, default=8, help="passes per half of the frame the kernels are timed on")
ap.add_argument("--runs", type=int, default=12)
ap.add_argument("--sizes", default="800x600,1920x1080")
ap.add_argument("--fractions", default="1,2,4,8", help="one k per case: n / k of the groups selected")
ap.add_argument("--tile-db", type=float, default=28.0)
ap.add_argument("--min-passes", type=int, default=4)
ap.add_argument("--passes-per-check", type=int, default=4)
ap.add_argument("--max-passes", type=int, default=32)
args = ap.parse_args()
if args.runs < 10:
    ap.error("--runs: a median of at least 10 runs")


class Events:
    """Two HIP events of the runtime the library itself is linked against (as tools/filtered_error_probe.py)."""

    def __init__(self):
        self.hip = api.DeviceWords._runtime()
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            if self.hip.hipEventCreate(C.byref(e)) != 0:
                raise api.RtError(-3, "hipEventCreate failed")

    def idle(self):
        if self.hip.hipDeviceSynchronize() != 0:
            raise api.RtError(-3, "hipDeviceSynchronize failed")

    def time(self, stream, fn):
        """The device idle, then fn() queues work on `stream`; returns the device milliseconds between the events either side of it."""
        self.idle()
        if self.hip.hipEventRecord(self.ev[0], C.c_void_p(stream)) != 0:
            raise api.RtError(-3, "hipEventRecord failed")
        fn()
        ms = C.c_float()
        if self.hip.hipEventRecord(self.ev[1], C.c_void_p(stream)) != 0 or self.hip.hipEventSynchronize(self.ev[1]) != 0 or \
                self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) != 0:
            raise api.RtError(-3, "timing between HIP events failed")
        return float(ms.value)

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def context(w, h, stream_id):
    c = api.RtContext(w, h)
    c.set_scene(host.demo_scene())
    c.set_camera(host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h))
    c.seed_stream(stream_id, c.stream)
    return c


def restart(a, b):
    a.seed_stream(1, a.stream)
    b.seed_stream(2, b.stream)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def shape(w, h):
    tiles_x = (w + 7) // 8
    return (h + 7) // 8, tiles_x, (tiles_x + 3) // 4


def first_groups(w, h, k):
    """An error map that selects the first n / k groups in raster order with above = 0: 1 in the first tile of each."""
    ty, tx, gx = shape(w, h)
    n = ty * gx
    err = np.zeros((ty, tx), np.uint32)
    for g in range(max(n // k, 1)):
        err[g // gx, 4 * (g % gx)] = 1
    return err, max(n // k, 1), n


def kernel_records(a, b, ev):
    w, h = a.w, a.h
    base = {"scene": "demo", "w": w, "h": h, "params": api.denoise_defaults().as_dict(), "passes_per_half": args.passes, "runs": args.runs,
            "timed_with": "HIP events on the context's stream, the device idle before the first; 3 warm-up runs", "build_id": api.build_id()}
    restart(a, b)
    a.render_async(args.passes, a.stream)
    b.render_async(args.passes, b.stream)
    whole = [ev.time(a.stream, lambda: a.denoise_pair(b, None, a.stream)) for _ in range(3 + args.runs)][3:]
    yield {"record": "live_check_kernel", "call": "rt_denoise_pair_async", "groups": shape(w, h)[0] * shape(w, h)[2], "ms": spread(whole), **base}
    for k in [int(v) for v in args.fractions.split(",")]:
        err, m, n = first_groups(w, h, k)
        restart(a, b)
        a.render_async(args.passes, a.stream)
        b.render_async(args.passes, b.stream)
        a.denoise_pair(b, None, a.stream)
        d = api.DeviceWords(err)
        got = a.select_tiles(d.ptr, 0, a.stream), b.select_tiles(d.ptr, 0, b.stream)
        d.close()
        assert got[0] == got[1] and got[0][0] == m, (got, m)
        ms = []
        for _ in range(3 + args.runs):
            a.render_tiles_async(1, a.stream)
            b.render_tiles_async(1, b.stream)
            ms.append(ev.time(a.stream, lambda: a.denoise_pair_tiles(b, None, a.stream)))
        yield {"record": "live_check_kernel", "call": "rt_denoise_pair_tiles_async", "groups": n, "selected_groups": m,
               "selection": "the first n / %d groups in raster order from the bottom row" % k, "ms": spread(ms[3:]),
               "over_whole_frame_call": round(statistics.median(ms[3:]) / statistics.median(whole), 3), **base}


def by_public_calls(a, b):
    """rt_render_adaptive_filtered_tiles written with the public calls: (reached, checks, live groups per check)."""
    above = min(int(np.floor(255.0 * 255.0 * 192.0 / 10.0 ** (args.tile_db / 10.0))), 2 ** 32 - 1)
    n0 = min(args.min_passes, args.max_passes)
    a.render_async(n0, a.stream)
    b.render_async(n0, b.stream)
    a.denoise_pair(b, None, a.stream)
    live = []
    while True:
        _, tiles = a.compare_filtered(b, tiles=True)
        d = api.DeviceWords(tiles)
        ca, cb = a.select_tiles(d.ptr, above, a.stream), b.select_tiles(d.ptr, above, b.stream)
        d.close()
        assert ca == cb
        live.append(ca[0])
        n = min(args.passes_per_check, args.max_passes - a.current_sample)
        if ca[0] == 0 or n == 0:
            return ca[0] == 0, len(live), live
        a.render_tiles_async(n, a.stream)
        b.render_tiles_async(n, b.stream)
        a.denoise_pair_tiles(b, None, a.stream)


def loop_record(a, b, ev):
    w, h = a.w, a.h
    loops = {"rt_render_adaptive_filtered": a.render_adaptive_filtered, "rt_render_adaptive_filtered_tiles": a.render_adaptive_filtered_tiles}
    loop_args = (args.tile_db, args.min_passes, args.passes_per_check, args.max_passes)
    wall, result, passes = {k: [] for k in loops}, {}, {}
    for run in range(2 + args.runs):
        for name, loop in loops.items():                    # alternating
            restart(a, b)
            ev.idle()
            t0 = time.perf_counter()
            reached, last, checks = loop(b, *loop_args)
            t1 = time.perf_counter()
            if run >= 2:
                wall[name].append((t1 - t0) * 1e3)
            result[name] = {"reached": reached, "checks": checks, "last_psnr_db": round(api.error_psnr(last), 3)}
            passes[name] = a.tile_passes()
    assert np.array_equal(*passes.values()), "the two loops left different pass maps"
    restart(a, b)
    reached, checks, live = by_public_calls(a, b)
    ty, _, gx = shape(w, h)
    old, new = statistics.median(wall["rt_render_adaptive_filtered"]), statistics.median(wall["rt_render_adaptive_filtered_tiles"])
    return {"record": "live_check_loop", "scene": "demo", "w": w, "h": h, "tile_psnr_db": args.tile_db, "min_passes": args.min_passes,
            "passes_per_check": args.passes_per_check, "max_passes": args.max_passes, "params": api.denoise_defaults().as_dict(), "runs": args.runs,
            "groups": ty * gx, "checks": checks, "live_groups_per_check": live,
            "mean_passes_per_tile": round(float(passes["rt_render_adaptive_filtered_tiles"].mean()), 3),
            "baseline": "rt_render_adaptive_filtered", "wall_ms": {k: spread(v) for k, v in wall.items()}, "results": result,
            "new_over_baseline": round(new / old, 3), "render_kernel": a.last_kernel,
            "timed_with": "host clock around the call (it ends in a wait on both streams), the device idle before; the two loops alternate; 2 warm-up runs each",
            "build_id": api.build_id()}


for size in [s for s in args.sizes.split(",") if s]:
    w, h = (int(v) for v in size.split("x"))
    with context(w, h, 1) as a, context(w, h, 2) as b:
        ev = Events()
        for x in (a, b):                                    # the first launches of a scene measure and price (four steps): not part of any figure
            for _ in range(6):
                x.render_pass(args.passes)
        for rec in kernel_records(a, b, ev):
            print(json.dumps(rec), flush=True)
        print(json.dumps(loop_record(a, b, ev)), flush=True)
        ev.close()
