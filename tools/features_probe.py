#!/usr/bin/env python3
"""What the feature plane costs swept and walked (include/rt_api.h "feature planes"; csrc/rt_instance.h features_form), one JSON record per scene and
size, stamped with rt_build_id(), and a last record that reads the threshold off the curves:

    python tools/features_probe.py [--runs 12] > profiles/r35_features_walk.jsonl

  rt_features_async between two HIP events on the context's stream, the device idle before the first (median of --runs), on a context of the
  diagnostics library forced to the sweep (rt_debug_set_features_form 1: rt_features_kernel, the kernel every scene had before) and forced to the
  hierarchy (2; the placement the LDS limits give), and -- the product library, nothing forced -- what the rule picks; beside ONE pass of the same
  scene on the product library, measured the same way in the same run.  Scenes: random_spheres(n) for the probed counts and the Demo scene.  A scene
  without a hierarchy has no walked figure: the Demo scene, and random_spheres(56), whose ground stays outside the tree and leaves 55 spheres in it,
  one short of the 56 a hierarchy is built from -- so random_spheres(57), the smallest random scene that has one, is probed beside it.
  The last record, "case": "threshold": the smallest probed count from which the hierarchy is faster at every size and stays faster at every larger
  probed count -- 56, the fewest records a hierarchy exists from, when it never loses.  csrc/rt_instance.h kFeaturesWalkMin is set to that.
One process; every step runs under its own time limit: faulthandler.dump_traceback_later(limit, exit=True), a watchdog THREAD that prints where the
step stands and ends the process with _exit -- also while the main thread is blocked inside the HIP runtime, where a Python signal handler would
never run -- so nothing more is started on the device.
No time is an acceptance criterion of any test: the records say what was measured."""
import argparse
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=12)
ap.add_argument("--sizes", default="800x600,1920x1080")
ap.add_argument("--counts", default="56,57,128,256,512,1024,2048,8192,262144")
ap.add_argument("--step-limit", type=int, default=120, help="seconds a step (one scene at one size) may take")
args = ap.parse_args()
SIZES = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
COUNTS = [int(v) for v in args.counts.split(",")]
BUILD = api.build_id()
RT_ERR_STATE = -5


class Events:
    """Two HIP events of the runtime the library itself is linked against (as tools/reproject_probe.py)."""

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
        if self.hip.hipDeviceSynchronize() != 0 or self.hip.hipEventRecord(self.ev[0], C.c_void_p(stream)) != 0:
            raise api.RtError(-3, "hipEventRecord failed")
        fn()
        ms = C.c_float()
        if self.hip.hipEventRecord(self.ev[1], C.c_void_p(stream)) != 0 or self.hip.hipEventSynchronize(self.ev[1]) != 0 or \
                self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) != 0:
            raise api.RtError(-3, "timing between HIP events failed")
        return float(ms.value)


EV = Events()


def timed(stream, fn, warm, runs):
    ms = [EV.time(stream, fn) for _ in range(warm + runs)][warm:]
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def emit(rec):
    print(json.dumps({"build_id": BUILD, **rec}), flush=True)


def context(sph, cam, w, h, diag):
    c = api.RtContext(w, h, diag=diag)
    c.set_scene(sph)
    c.set_camera(cam)
    return c


def step(name, sph, orig, target, w, h):
    cam = host.compute_camera(orig, target, w, h)
    rec = {"case": "time", "scene": name, "records": len(sph), "w": w, "h": h, "runs": args.runs}
    with context(sph, cam, w, h, True) as F, context(sph, cam, w, h, False) as P:
        F._check(F._lib.rt_debug_set_features_form(F._h, 1))
        rec["swept_ms"] = timed(F.stream, lambda: F.features_async(F.stream), 2, args.runs)
        rec["swept_kernel"] = F.last_features_kernel()
        F._check(F._lib.rt_debug_set_features_form(F._h, 2))
        try:
            rec["walked_ms"] = timed(F.stream, lambda: F.features_async(F.stream), 2, args.runs)
            rec["walked_kernel"] = F.last_features_kernel()
        except api.RtError as e:
            if e.code != RT_ERR_STATE:
                raise
            rec["walked_ms"], rec["walked_kernel"] = None, None          # no hierarchy: nothing to walk
        rec["rule_ms"] = timed(P.stream, lambda: P.features_async(P.stream), 2, args.runs)
        rec["rule_kernel"] = P.last_features_kernel()
        for _ in range(6):                                   # the scene's first launches settle which form renders it
            P.render_async(1, P.stream)
        rec["one_pass_ms"] = timed(P.stream, lambda: P.render_async(1, P.stream), 2, args.runs)
        rec["pass_kernel"] = P.last_kernel
    emit(rec)
    return rec


def the_scenes():
    yield "demo", host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET
    for n in COUNTS:
        sph, orig, target = scenes.random_spheres(n)
        yield "random_%d" % n, sph, orig, target


records = []
for name, sph, orig, target in the_scenes():
    for w, h in SIZES:
        faulthandler.dump_traceback_later(args.step_limit, exit=True)
        records.append(step(name, sph, orig, target, w, h))
        faulthandler.cancel_dump_traceback_later()

# the threshold: per probed count, is the hierarchy faster at EVERY size; then the smallest count from which that holds at every larger one
wins = {}
for r in records:
    if r["scene"].startswith("random_") and r["walked_ms"] is not None:
        wins[r["records"]] = wins.get(r["records"], True) and r["walked_ms"]["median"] < r["swept_ms"]["median"]
least = None
for n in sorted(wins, reverse=True):
    if not wins[n]:
        break
    least = n
never_loses = bool(wins) and all(wins.values())
emit({"case": "threshold", "faster_walked_at_every_size": {str(n): wins[n] for n in sorted(wins)}, "smallest_probed_count_walked_from_there_on": least,
      "hierarchy_never_loses": never_loses, "kFeaturesWalkMin": 56 if never_loses else least,
      "note": "56 when the hierarchy never loses: the rule's first clause -- a hierarchy exists -- then decides alone"})
