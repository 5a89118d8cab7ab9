#!/usr/bin/env python3
"""Measurements of the error estimate of the filtered frame (include/rt_api.h "the error of the filtered frame"), one JSON record per case,
stamped with rt_build_id():

    python tools/filtered_error_probe.py [--scenes demo,c16_demo_plus_10] [--reference-passes 4096] [--runs 12] >> profiles/r14_filtered_error.jsonl

  time      the Demo scene at 800x600 and 1920x1080, search radius 3, 5 and 8 (patch radius 1): two contexts on seed streams 1 and 2 render
            --passes passes each.  rt_denoise_pair_async (its variance kernel and the pair kernel) on the first context's own stream between
            two HIP events, 3 runs to warm up, then the median, smallest and largest of --runs runs.  In the same run, as the yardstick,
            rt_denoise_async of their merge in a third context, timed the same way (the merge made again before every run, outside the
            events), and one half's --passes passes in one launch: what a check costs against what it can save.  The pair call does two
            filters' arithmetic on shared staging, so about twice the single filter is what to expect.
  estimate  per scene at 800x600, 4, 16 and 64 passes per half: the PSNR (over the packed 8-bit channels) between the halves (rt_compare),
            between the cross-filtered halves (rt_compare_filtered), and of the filtered merge against a context of --reference-passes passes
            of the default seed stream -- the device's version of the header's table.
  stop      per scene at 800x600: the pass number at which rt_render_converged and rt_render_converged_filtered stop for --target dB
            (8 passes per check, at most --max-passes).
No time is an acceptance criterion of anything: the records say what was measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="demo,c16_demo_plus_10")
ap.add_argument("--reference-passes", type=int, default=4096)
ap.add_argument("--passes", type=int, default=8, help="passes per half of the timed frame")
ap.add_argument("--runs", type=int, default=12)
ap.add_argument("--sizes", default="800x600,1920x1080")
ap.add_argument("--radii", default="3,5,8")
ap.add_argument("--estimate-passes", default="4,16,64")
ap.add_argument("--target", type=float, default=30.0)
ap.add_argument("--max-passes", type=int, default=1024)
args = ap.parse_args()
if args.runs < 10:
    ap.error("--runs: a median of at least 10 runs")


class Events:
    """Two HIP events of the runtime the library itself is linked against (api.DeviceWords finds it): elapsed device time on a stream
    (as tools/denoise_probe.py times the single filter)."""

    def __init__(self):
        self.hip = api.DeviceWords._runtime()
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            if self.hip.hipEventCreate(C.byref(e)) != 0:
                raise api.RtError(-3, "hipEventCreate failed")

    def time(self, stream, fn):
        """fn() queues work on `stream`; returns the device milliseconds between the events either side of it."""
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


def scene_of(name):
    if name == "demo":
        return host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET
    return host.read_scene(os.path.join(ROOT, "raytracing_simple_amd", "scenes_scn", name + ".scn"), reference_doubling=False)


def context(scene, w, h, stream_id=None):
    sph, orig, target = scene
    c = api.RtContext(w, h)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(orig, target, w, h))
    if stream_id is not None:
        c.seed_stream(stream_id, c.stream)
    return c


def spread(ms):
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def time_record(w, h, radius):
    scene = scene_of("demo")
    with context(scene, w, h, 1) as a, context(scene, w, h, 2) as b, context(scene, w, h) as dst:
        ev = Events()
        for x in (a, b):                                    # the first launches of a scene measure and price (four steps): not part of any figure
            for _ in range(6):
                x.render_pass(args.passes)
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
        render_ms = ev.time(a.stream, lambda: a.render_async(args.passes, a.stream))
        b.render_async(args.passes, b.stream)
        params = {"search_radius": radius, "patch_radius": 1}
        pair_ms, single_ms = [], []
        for run in range(3 + args.runs):
            t = ev.time(a.stream, lambda: a.denoise_pair(b, params, a.stream))
            dst.reset_async(dst.stream)
            dst.merge([a, b], dst.stream)
            s = ev.time(dst.stream, lambda: dst.denoise(a, b, params, dst.stream))
            if run >= 3:
                pair_ms.append(t)
                single_ms.append(s)
        ev.close()
        pm, smed = spread(pair_ms), spread(single_ms)
        return {"record": "filtered_error_time", "scene": "demo", "w": w, "h": h, "search_radius": radius, "patch_radius": 1,
                "passes_per_half": args.passes, "runs": args.runs, "pair_ms_median": pm[0], "pair_ms_min": pm[1], "pair_ms_max": pm[2],
                "denoise_ms_median": smed[0], "denoise_ms_min": smed[1], "denoise_ms_max": smed[2], "pair_over_denoise": round(pm[0] / smed[0], 3),
                "render_ms_one_half": round(render_ms, 4), "render_kernel": a.last_kernel,
                "timed_with": "HIP events on the context's stream, 3 warm-up runs", "build_id": api.build_id()}


def estimate_records(name, w=800, h=600):
    scene = scene_of(name)
    with context(scene, w, h) as ref, context(scene, w, h) as a, context(scene, w, h) as b, context(scene, w, h) as dst:
        done = 0
        while done < args.reference_passes:                 # (launches of at most 256 passes)
            n = min(256, args.reference_passes - done)
            ref.render_async(n, ref.stream)
            done += n
        for n in [int(v) for v in args.estimate_passes.split(",")]:
            a.seed_stream(1, a.stream)
            b.seed_stream(2, b.stream)
            a.render_async(n, a.stream)
            b.render_async(n, b.stream)
            pair = api.error_psnr(a.compare(b))
            a.denoise_pair(b, None, a.stream)
            cross = api.error_psnr(a.compare_filtered(b))
            dst.reset_async(dst.stream)
            dst.merge([a, b], dst.stream)
            dst.denoise(a, b, None, dst.stream)
            shown = api.error_psnr(dst.compare(ref))
            yield {"record": "filtered_error_estimate", "scene": name, "spheres": int(len(scene[0])), "w": w, "h": h, "passes_per_half": n,
                   "params": api.denoise_defaults().as_dict(), "reference_frame": "%d passes, default seed stream" % args.reference_passes,
                   "pair_psnr_db": round(pair, 3), "cross_filtered_pair_psnr_db": round(cross, 3), "filtered_vs_reference_psnr_db": round(shown, 3),
                   "estimate_minus_truth_db": round(cross - shown, 3), "build_id": api.build_id()}
        stops = {}
        for key, loop in (("raw_pair", lambda: a.render_converged(b, args.target, 8, args.max_passes)),
                          ("cross_filtered_pair", lambda: a.render_converged_filtered(b, args.target, 8, args.max_passes))):
            a.seed_stream(1, a.stream)
            b.seed_stream(2, b.stream)
            reached, last, checks = loop()
            stops[key] = {"reached": reached, "passes_per_half": a.current_sample, "checks": checks, "psnr_db": round(api.error_psnr(last), 3)}
        yield {"record": "filtered_error_stop", "scene": name, "w": w, "h": h, "target_psnr_db": args.target, "passes_per_check": 8,
               "max_passes": args.max_passes, **stops, "build_id": api.build_id()}


for size in [s for s in args.sizes.split(",") if s]:
    w, h = (int(v) for v in size.split("x"))
    for radius in [int(v) for v in args.radii.split(",")]:
        print(json.dumps(time_record(w, h, radius)), flush=True)
for name in [s for s in args.scenes.split(",") if s]:
    for rec in estimate_records(name):
        print(json.dumps(rec), flush=True)
