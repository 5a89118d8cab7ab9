#!/usr/bin/env python3
"""Device time of the per-pixel kernels that call csrc/rt_rules.h, for comparing two builds of the library in one session:

    python tools/rules_probe.py --lib PATH/librt_hip.so --label parent >> profiles/r31_rules.jsonl      (one process = one run; alternate the builds)
    python tools/rules_probe.py --verdict profiles/r31_rules.jsonl

One JSON record per scene and kernel, stamped with rt_build_id(): the call between two HIP events on the context's stream, the device idle before the
first, three warm-ups, the median of --runs, as tools/reproject_probe.py measures.  1920x1080, the Demo scene and random_spheres(1024) (c3_random_1024):
  rt_features_kernel            rt_features_async
  rt_atrous_prepare_kernel<3>   rt_atrous_async, 0 levels, from the colour plane
  rt_atrous_prepare_kernel<4>   ... from the temporal plane
  rt_reproject_kernel<3>        rt_reproject_async from the source's colour plane
  rt_reproject_kernel<4>        ... from its temporal plane
--verdict: per scene and kernel, the median over each label's runs; `new` holds when its median <= the parent's median + the parent's own max - min."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--label", default="new")
ap.add_argument("--runs", type=int, default=12)
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--verdict")
args = ap.parse_args()

if args.verdict:
    rows = {}
    for line in open(args.verdict):
        r = json.loads(line)
        rows.setdefault((r["scene"], r["kernel"]), {}).setdefault(r["label"], []).append(r["ms"]["median"])
    ok = True
    for (scene, kernel), by in sorted(rows.items()):
        p, n = by["parent"], by["new"]
        bound = statistics.median(p) + (max(p) - min(p))
        holds = statistics.median(n) <= bound
        ok = ok and holds
        print("%-16s %-28s parent %.4f (%d runs, %.4f .. %.4f)  new %.4f (%d runs)  bound %.4f  %s" % (
            scene, kernel, statistics.median(p), len(p), min(p), max(p), statistics.median(n), len(n), bound, "holds" if holds else "MISSES"))
    sys.exit(0 if ok else 1)

from raytracing_simple_amd import api, host, scenes  # noqa: E402

if args.lib:
    api.lib_path = lambda diag=False: os.path.abspath(args.lib)        # (before the first load)
W, H = (int(v) for v in args.size.split("x"))
BUILD = api.build_id()
hip = api.DeviceWords._runtime()
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
EV = [C.c_void_p(), C.c_void_p()]
for e in EV:
    if hip.hipEventCreate(C.byref(e)) != 0:
        raise api.RtError(-3, "hipEventCreate failed")


def once(stream, fn):
    if hip.hipDeviceSynchronize() != 0 or hip.hipEventRecord(EV[0], C.c_void_p(stream)) != 0:
        raise api.RtError(-3, "hipEventRecord failed")
    fn()
    ms = C.c_float()
    if hip.hipEventRecord(EV[1], C.c_void_p(stream)) != 0 or hip.hipEventSynchronize(EV[1]) != 0 or hip.hipEventElapsedTime(C.byref(ms), EV[0], EV[1]) != 0:
        raise api.RtError(-3, "timing between HIP events failed")
    return float(ms.value)


def timed(scene, kernel, stream, fn):
    ms = [once(stream, fn) for _ in range(3 + args.runs)][3:]
    print(json.dumps({"build_id": BUILD, "label": args.label, "scene": scene, "kernel": kernel, "w": W, "h": H, "runs": args.runs,
                      "ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}}), flush=True)


def view(sph, orig, target, stream_id, passes):
    c = api.RtContext(W, H)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(orig, target, W, H))
    c.seed_stream(stream_id, c.stream)
    c.render_async(passes, c.stream)
    c.features_async(c.stream)
    return c


def moved(orig, target, share):                             # sideways by `share` of the distance to the target
    import numpy as np
    o, t = np.asarray(orig, np.float64), np.asarray(target, np.float64)
    side = np.cross(t - o, (0.0, 1.0, 0.0))
    return tuple(float(v) for v in o + side / np.linalg.norm(side) * np.linalg.norm(t - o) * share)


for name, (sph, o, t) in (("demo", (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET)), ("c3_random_1024", scenes.random_spheres(1024))):
    with view(sph, o, t, 1, 4) as S, view(sph, moved(o, t, 0.02), t, 2, 2) as D, view(sph, moved(o, t, -0.02), t, 3, 2) as P:
        timed(name, "rt_features_kernel", D.stream, lambda: D.features_async(D.stream))
        timed(name, "rt_atrous_prepare_kernel<3>", D.stream, lambda: D.atrous_async({"levels": 0}, D.stream))
        timed(name, "rt_reproject_kernel<3>", D.stream, lambda: D.reproject_async(S, None, D.stream))
        S.reproject_async(P, None, S.stream)                # S's temporal plane is current from here
        timed(name, "rt_reproject_kernel<4>", D.stream, lambda: D.reproject_async(S, None, D.stream))
        timed(name, "rt_atrous_prepare_kernel<4>", D.stream, lambda: D.atrous_async({"levels": 0}, D.stream))
