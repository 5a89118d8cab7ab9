#!/usr/bin/env python3
"""What shadow-aware history costs and gains on the device (include/rt_api.h "shadow-aware history"), one JSON record per case, stamped with
rt_build_id():

    python tools/shadow_history_probe.py [--runs 12] >> profiles/r33_shadow_history.jsonl

  time     rt_reproject_async between two HIP events on the context's stream, the device idle before the first, with rt_set_shadow_history ON against
           OFF, ALTERNATING call by call in one process (median of --runs each), at 800x600 and 1920x1080, the source read through its colour plane,
           the destination at 2 passes, with pair lists of 1, 16 and 1024 pairs: the Demo scene followed by small spheres below the ground (they are
           in no pixel and in every pixel's pair loop), that many of them moved.
  quality  the header's table from rendered contexts: cornell and simple (tests/golden) and Demo at 96x96, twelve frames of 2 passes, frame f on
           seed stream f with one record moved by (f - 1) steps, two contexts taking turns, the defaults of both calls, then three a-trous levels;
           truth 512 passes of the default stream of the last frame's scene; PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5 of the
           last T and A with the setting off and on, and the share of pixels the last frame flagged.
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
ap.add_argument("--pairs", default="1,16,1024")
ap.add_argument("--quality", default="cornell:16:-1.5,demo:4:-2.0,simple:6:-2.5")
args = ap.parse_args()
SIZES = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",") if s]
BUILD = api.build_id()
F = np.float32


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


def emit(rec):
    print(json.dumps({"build_id": BUILD, **rec}), flush=True)


def view(sph, orig, target, w, h, stream_id, passes):
    c = api.RtContext(w, h)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(orig, target, w, h))
    c.seed_stream(stream_id, c.stream)
    if passes:
        c.render_async(passes, c.stream)
    c.features_async(c.stream)
    return c


def alternating(stream, call, setting, warm=3, runs=args.runs):
    """`call` timed with the setting ON and OFF in turn; setting(on) switches it.  Returns the two records."""
    ms = {True: [], False: []}
    for k in range(2 * (warm + runs)):
        on = k % 2 == 0
        setting(on)
        ms[on].append(EV.time(stream, call))
    out = {}
    for on in (True, False):
        v = ms[on][warm:]
        out["on" if on else "off"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return out


def with_buried(n_pairs):
    """The Demo scene and `n_pairs` small spheres inside the ground sphere, where no ray meets them; the moved copy: all of them a step aside."""
    demo = host.demo_scene()
    sph = np.zeros(len(demo) + n_pairs, api.SPHERE_DT)
    sph[:len(demo)] = demo
    rng = np.random.default_rng(n_pairs)
    for k in range(n_pairs):
        sph[len(demo) + k] = (0.5, (rng.uniform(-60, 60), rng.uniform(-40, -10), rng.uniform(-60, 60)), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 0)
    moved = sph.copy()
    moved["p"][len(demo):, 0] += F(1.0)
    return sph, moved


# ---- time ----------------------------------------------------------------------------------------------------------------
o, t = host.DEMO_ORIG, host.DEMO_TARGET
for w, h in SIZES:
    for n_pairs in (int(v) for v in args.pairs.split(",") if v):
        before, after = with_buried(n_pairs)
        assert len(api.shadow_history_pairs(before, after)) == n_pairs
        with view(before, o, t, w, h, 1, 16) as S, view(after, o, t, w, h, 2, 2) as D:
            switch = lambda on: D.set_shadow_history({} if on else None)      # noqa: E731
            rec = {"case": "time", "scene": "demo + buried", "w": w, "h": h, "pairs": n_pairs, "runs": args.runs, "alternating": True,
                   "rt_reproject_async_ms": alternating(D.stream, lambda: D.reproject_async(S, None, D.stream), switch)}
            D.set_shadow_history({})
            D.reproject_async(S, None, D.stream)
            rec["share_flagged"] = round(float(D.read_history_flags().mean()), 4)
            d = rec["rt_reproject_async_ms"]
            rec["ns_per_pair_and_pixel"] = round((d["on"]["median"] - d["off"]["median"]) * 1e6 / (n_pairs * w * h), 5)
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


FRAMES, W, H = 12, 96, 96
for case in args.quality.split(","):
    if not case:
        continue
    name, record, step = case.split(":")
    record, step = int(record), F(step)
    sph0, orig, target = quality_scene(name)
    rec = {"case": "quality", "scene": name, "w": W, "h": H, "frames": FRAMES, "passes_per_frame": 2, "moved_record": record, "step_x_per_frame": float(step),
           "truth_passes": 512, "levels": 3}
    for on in (False, True):
        with view(sph0, orig, target, W, H, 0, 0) as A, view(sph0, orig, target, W, H, 0, 0) as B:
            for f in range(1, FRAMES + 1):
                ctx, other = (A, B) if f % 2 else (B, A)
                sph = sph0.copy()
                sph["p"][record][0] += F(f - 1) * step
                ctx.set_shadow_history({} if on else None)
                ctx.update_spheres(record, sph[record:record + 1])
                ctx.seed_stream(f, ctx.stream)
                ctx.features_async(ctx.stream)
                ctx.render_async(2, ctx.stream)
                if f > 1:
                    ctx.reproject_async(other, None, ctx.stream)
            with view(sph, orig, target, W, H, 0, 512) as truth:
                ref = truth.read_colors().reshape(H, W, 3)
            T = ctx.read_temporal(packed=False)
            ctx.atrous_async({"levels": 3}, ctx.stream)
            a = ctx.read_atrous(packed=False)
            key = "on" if on else "off"
            rec["temporal_db_" + key], rec["atrous_db_" + key] = psnr8(T[..., 0:3], ref), psnr8(a[..., 0:3], ref)
            if on:
                rec["share_flagged_last_frame"] = round(float(ctx.read_history_flags().mean()), 4)
    emit(rec)
