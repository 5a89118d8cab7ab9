#!/usr/bin/env python3
"""What the edge-avoiding wavelet filter costs and gains on the device (include/rt_api.h "edge-avoiding wavelet filter"), one JSON record per case,
stamped with rt_build_id():

    python tools/atrous_probe.py [--runs 12] >> profiles/r30_atrous.jsonl

  time     rt_atrous_async between two HIP events on the context's stream, the device idle before the first (median of --runs): the Demo scene at
           800x600 and 1920x1080, the context 2 passes from an origin moved sideways by 2 % of its distance to the target, with 1, 3 and 5 levels,
           from its COLOUR plane (3 floats a pixel) and from its TEMPORAL plane (4, reprojected from 16 passes of the Demo origin) -- beside ONE
           pass, rt_features_async, rt_reproject_async and rt_denoise_async (two halves of one pass each, the defaults), measured the same way in
           the same run.
  quality  the header's table from rendered contexts: cornell and simple (tests/golden) and Demo at 96x96, cornell and Demo at 192x192 and at
           800x600; S 16 passes of seed stream 1, D 2 passes of stream 2, truth 1024 passes (512 at 192x192) of the default stream from the moved
           origin; PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5 of T, of T filtered with 1 to 5 levels, of D alone and of D alone
           filtered with 3 levels.
No time is an acceptance criterion of anything: the records say what was measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=12)
ap.add_argument("--sizes", default="800x600,1920x1080")
ap.add_argument("--quality", default="cornell:96x96,demo:96x96,simple:96x96,demo:192x192,cornell:192x192,demo:800x600,cornell:800x600")
args = ap.parse_args()
SIZES = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
BUILD = api.build_id()


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


def sideways(orig, target, share):
    o, t = np.asarray(orig, np.float64), np.asarray(target, np.float64)
    d = t - o
    side = np.cross(d, (0.0, 1.0, 0.0))
    return tuple(float(v) for v in o + side / np.linalg.norm(side) * np.linalg.norm(d) * share)


def view(sph, orig, target, w, h, stream_id, passes):
    c = api.RtContext(w, h)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(orig, target, w, h))
    c.seed_stream(stream_id, c.stream)
    if passes:
        c.render_async(passes, c.stream)
    c.features_async(c.stream)
    return c


# ---- time ----------------------------------------------------------------------------------------------------------------
o, t = host.DEMO_ORIG, host.DEMO_TARGET
for w, h in SIZES:
    moved = sideways(o, t, 0.02)
    with view(host.demo_scene(), o, t, w, h, 1, 16) as S, view(host.demo_scene(), moved, t, w, h, 2, 2) as D, \
            view(host.demo_scene(), moved, t, w, h, 3, 1) as a, view(host.demo_scene(), moved, t, w, h, 4, 1) as b, \
            view(host.demo_scene(), moved, t, w, h, 0, 0) as dst:
        rec = {"case": "time", "scene": "demo", "w": w, "h": h, "runs": args.runs}
        for levels in (1, 3, 5):
            rec["rt_atrous_async_ms_from_colour_plane_levels_%d" % levels] = timed(D.stream, lambda: D.atrous_async({"levels": levels}, D.stream), 3, args.runs)
        rec["rt_reproject_async_ms"] = timed(D.stream, lambda: D.reproject_async(S, None, D.stream), 3, args.runs)
        for levels in (0, 1, 3, 5):                          # D's temporal plane is current from here: the 4-channel preparation
            rec["rt_atrous_async_ms_from_temporal_plane_levels_%d" % levels] = timed(D.stream, lambda: D.atrous_async({"levels": levels}, D.stream), 3, args.runs)
        rec["rt_features_async_ms"] = timed(D.stream, lambda: D.features_async(D.stream), 3, args.runs)
        def denoise():                                       # (the merge the filter works on is formed again outside the timed call, as tools/denoise_probe.py does)
            dst.reset_async(dst.stream)
            dst.merge([a, b], dst.stream)
            return EV.time(dst.stream, lambda: dst.denoise(a, b, None, dst.stream))

        ms = [denoise() for _ in range(3 + args.runs)][3:]
        rec["rt_denoise_async_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        for _ in range(6):                                   # the scene's first launches settle which form renders it
            D.render_async(1, D.stream)
        rec["one_pass_ms"] = timed(D.stream, lambda: D.render_async(1, D.stream), 2, args.runs)
        rec["pass_kernel"] = D.last_kernel
        emit(rec)


# ---- quality -------------------------------------------------------------------------------------------------------------
def psnr8(img, ref):
    pack = lambda c: (np.clip(np.asarray(c, np.float64), 0.0, 1.0) ** (1 / 2.2) * 255 + .5).astype(np.int64)      # noqa: E731
    d = (pack(img) - pack(ref)).astype(np.float64)
    return round(float(10 * np.log10(255.0 ** 2 / np.mean(d * d))), 2)


def quality_scene(name):
    if name == "demo":
        return host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET
    z = np.load(os.path.join(ROOT, "tests", "golden", name + "_96x96_4spp.npz"))
    cam = z["camera"].astype(np.float32)
    return z["spheres"].view(api.SPHERE_DT).copy(), tuple(float(v) for v in cam[0:3]), tuple(float(v) for v in cam[3:6])


for case in args.quality.split(","):
    if not case:
        continue
    name, size = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    sph, orig, target = quality_scene(name)
    moved = sideways(orig, target, 0.02)
    n_truth = 512 if (W, H) == (192, 192) else 1024
    with view(sph, orig, target, W, H, 1, 16) as S, view(sph, moved, target, W, H, 2, 2) as D, view(sph, moved, target, W, H, 0, n_truth) as truth:
        ref = truth.read_colors()
        rgb = lambda plane: plane[..., 0:3].reshape(-1)      # noqa: E731
        D.atrous_async({"levels": 3}, D.stream)              # no temporal plane yet: D's colour plane, n = 2 everywhere
        alone = psnr8(rgb(D.read_atrous(packed=False)), ref)
        D.reproject_async(S, None, D.stream)
        T = D.read_temporal(packed=False)
        levels = {}
        for n in (1, 2, 3, 4, 5):
            D.atrous_async({"levels": n}, D.stream)
            levels[str(n)] = psnr8(rgb(D.read_atrous(packed=False)), ref)
        emit({"case": "quality", "scene": name, "w": W, "h": H, "src_passes": 16, "dst_passes": 2, "truth_passes": n_truth, "moved_by": 0.02,
              "temporal_db": psnr8(rgb(T), ref), "temporal_filtered_db_by_levels": levels, "dst_alone_db": psnr8(D.read_colors(), ref),
              "dst_alone_filtered_db_levels_3": alone})
