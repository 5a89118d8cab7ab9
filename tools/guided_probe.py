#!/usr/bin/env python3
"""What the feature planes and the guided filters cost and gain on the device (include/rt_api.h "feature planes"), one JSON record per case,
stamped with rt_build_id():

    python tools/guided_probe.py [--runs 10] >> profiles/r21_guided.jsonl

  features  rt_features_async between two HIP events on the context's stream, the device idle before the first: the Demo scene and 1024 / 8192 /
            262 144 random spheres at 800x600 and 1920x1080, beside ONE pass of the same scene by rt_render_async (after the scene's first launches
            have settled which form renders it).  The feature kernel is a plain sweep, pixels x records; the pass is whatever the library picks.
  filters   the Demo scene, two contexts on seed streams 1 and 2 with 8 passes each, the default filter parameters and the default guide:
            rt_denoise_async, rt_denoise_pair_async and rt_denoise_pair_tiles_async (half of the groups selected), unguided and guided, the same way.
            The unguided kernels are the machine code they were before the guide existed.
  gain      halves of 4 and 16 passes on seed streams 1 and 2, merged and filtered on the device without and with the guide, against 2048 passes of
            the default stream; PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5; Demo and the two fixture scenes of tests/golden, 96x64.
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
from raytracing_simple_amd import api, host, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--sizes", default="800x600,1920x1080")
ap.add_argument("--counts", default="1024,8192,262144")
args = ap.parse_args()
SIZES = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
BUILD = api.build_id()


class Events:
    """Two HIP events of the runtime the library itself is linked against (as tools/live_check_probe.py)."""

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


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(stream, fn, warm, runs, before=None):
    out = []
    for k in range(warm + runs):
        if before:
            before()
        ms = EV.time(stream, fn)
        if k >= warm:
            out.append(ms)
    return spread(out)


def emit(rec):
    print(json.dumps({"build_id": BUILD, **rec}), flush=True)


# ---- features ------------------------------------------------------------------------------------------------------------
def feature_cases():
    yield "demo", host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET
    for n in (int(v) for v in args.counts.split(",")):
        sph, orig, target = scenes.random_spheres(n)
        yield "random_%d" % n, sph, orig, target


for name, sph, orig, target in feature_cases():
    for w, h in SIZES:
        with api.RtContext(w, h) as c:
            c.set_scene(sph)
            c.set_camera(host.compute_camera(orig, target, w, h))
            ft = timed(c.stream, lambda: c.features_async(c.stream), 2, max(3, args.runs // 2))
            for _ in range(6):                               # the scene's first launches settle which form renders it
                c.render_async(1, c.stream)
            one = timed(c.stream, lambda: c.render_async(1, c.stream), 1, 3)
            emit({"case": "features", "scene": name, "spheres": int(len(sph)), "w": w, "h": h, "rt_features_async_ms": ft, "one_pass_ms": one,
                  "pass_kernel": c.last_kernel})


# ---- filters -------------------------------------------------------------------------------------------------------------
def demo_pair(w, h, passes, sph=None, cam=None, extra=0):
    out = []
    for k in range(2 + extra):
        c = api.RtContext(w, h)
        c.set_scene(host.demo_scene() if sph is None else sph)
        c.set_camera(host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h) if cam is None else cam)
        if k < 2:
            c.seed_stream(1 + k, c.stream)
            c.render_async(passes, c.stream)
        out.append(c)
    return out


def half_the_groups(a, b):
    """The first half of the groups in raster order from the bottom row, selected on both contexts from one hand-made error map."""
    tiles_x, tiles_y = (a.w + 7) // 8, (a.h + 7) // 8
    groups_x = (tiles_x + 3) // 4
    n = groups_x * tiles_y
    err = np.zeros((tiles_y, tiles_x), np.uint32)
    for g in range(n // 2):
        gy, gx = divmod(g, groups_x)
        err[gy, 4 * gx:4 * gx + 4] = 1
    dev = api.DeviceWords(err.reshape(-1))
    counts = a.select_tiles(dev.ptr, 0, a.stream), b.select_tiles(dev.ptr, 0, b.stream)
    return dev, counts


for w, h in SIZES:
    a, b, dst = demo_pair(w, h, 8, extra=1)
    with a, b, dst:
        dst.merge([a, b], dst.stream)
        rec = {"case": "filters", "scene": "demo", "w": w, "h": h, "passes_per_half": 8}
        for label, guide in (("unguided", None), ("guided", api.guide_defaults())):
            for c in (a, b):
                c.set_denoise_guide(guide)
                if guide is not None:
                    c.features_async(c.stream)
            rec["rt_denoise_async_ms_" + label] = timed(dst.stream, lambda: dst.denoise(a, b, None, dst.stream), 3, args.runs)
            rec["rt_denoise_pair_async_ms_" + label] = timed(a.stream, lambda: a.denoise_pair(b, None, a.stream), 3, args.runs)
            dev, counts = half_the_groups(a, b)

            def behind():
                a.render_tiles_async(1, a.stream)
                b.render_tiles_async(1, b.stream)

            rec["rt_denoise_pair_tiles_async_ms_" + label] = timed(a.stream, lambda: a.denoise_pair_tiles(b, None, a.stream), 3, args.runs, before=behind)
            rec["groups_selected"] = int(counts[0][0])
            a.reset()
            b.reset()
            a.seed_stream(1, a.stream)
            b.seed_stream(2, b.stream)
            a.render_async(8, a.stream)
            b.render_async(8, b.stream)
        emit(rec)


# ---- gain ----------------------------------------------------------------------------------------------------------------
def psnr8(img, ref):
    pack = lambda c: (np.clip(np.asarray(c, np.float64), 0.0, 1.0) ** (1 / 2.2) * 255 + .5).astype(np.int64)      # noqa: E731
    d = (pack(img) - pack(ref)).astype(np.float64)
    return round(float(10 * np.log10(255.0 ** 2 / np.mean(d * d))), 2)


def gain_scenes(w, h):
    yield "demo", host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    for name in ("cornell", "simple"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + "_96x96_4spp.npz"))
        cam = z["camera"].astype(np.float32)
        yield name, z["spheres"].view(api.SPHERE_DT).copy(), host.compute_camera(tuple(cam[0:3]), tuple(cam[3:6]), w, h)


W, H = 96, 64
for name, sph, cam in gain_scenes(W, H):
    with api.RtContext(W, H) as truth:
        truth.set_scene(sph)
        truth.set_camera(cam)
        truth.render_async(2048, truth.stream)
        ref = truth.read_colors()
    for passes in (4, 16):
        a, b, dst = demo_pair(W, H, passes, sph, cam, extra=1)
        with a, b, dst:
            rec = {"case": "gain", "scene": name, "w": W, "h": H, "passes_per_half": passes, "truth_passes": 2048}
            dst.merge([a, b], dst.stream)
            merged = dst.read_colors().copy()
            rec["merged_db"] = psnr8(merged, ref)
            for label, guide in (("unguided", None), ("guided", api.guide_defaults())):
                for c in (a, b):
                    c.set_denoise_guide(guide)
                    if guide is not None:
                        c.features_async(c.stream)
                dst.write_state(merged, None, 2 * passes)
                dst.denoise(a, b, None, dst.stream)
                rec[label + "_db"] = psnr8(dst.read_colors(), ref)
            emit(rec)
