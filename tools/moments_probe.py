#!/usr/bin/env python3
"""What the temporal luminance moments cost and gain on the device (include/rt_api.h "temporal luminance moments"), one JSON record per case, stamped
with rt_build_id():

    python tools/moments_probe.py [--runs 12] >> profiles/r32_moments.jsonl

  time     rt_reproject_async and rt_atrous_async (0 and 3 levels) between two HIP events on the context's stream, the device idle before the first,
           with rt_set_temporal_moments ON against OFF, ALTERNATING call by call in one process (median of --runs each): the Demo scene at 800x600
           and 1920x1080, the destination 2 passes from an origin moved sideways by 2 % of its distance to the target.  The reprojection is timed
           from a source read through its COLOUR plane (rule 25's luminance) and from one whose temporal and moments planes are current (one more
           16-byte load per tap); the filter with k_min 1, so that rule 28 applies wherever it can.
  quality  the header's table from rendered contexts: cornell and simple (tests/golden) and Demo at 96x96, eight frames of 2 passes, frame f on seed
           stream f from an origin moved sideways by f * 0.5 % of its distance to the target, two contexts taking turns, the defaults; truth 1024
           passes of the default stream from the last origin; PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5 of the last T and of A
           with rule 21 and with rule 28 at 1, 3 and 5 levels, over the whole frame and over the pixels within 2 pixels of a shadow edge of the truth
           frame (shadow_edges below: tests/test_moments_cpu.py's definition).
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
ap.add_argument("--quality", default="cornell:96x96,simple:96x96,demo:96x96")
args = ap.parse_args()
SIZES = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",") if s]
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


# ---- time ----------------------------------------------------------------------------------------------------------------
o, t = host.DEMO_ORIG, host.DEMO_TARGET
for w, h in SIZES:
    moved = sideways(o, t, 0.02)
    with view(host.demo_scene(), o, t, w, h, 1, 16) as Col, view(host.demo_scene(), o, t, w, h, 5, 4) as P, view(host.demo_scene(), o, t, w, h, 1, 12) as S, \
            view(host.demo_scene(), moved, t, w, h, 2, 2) as D:
        S.set_temporal_moments({})
        S.reproject_async(P, None, S.stream)                  # S holds a current temporal plane AND a current moments plane; Col neither
        S.read_moments()
        rec = {"case": "time", "scene": "demo", "w": w, "h": h, "runs": args.runs, "alternating": True}
        switch = lambda on: D.set_temporal_moments({"k_min": 1.0} if on else None)      # noqa: E731
        rec["rt_reproject_async_ms_from_colour_plane"] = alternating(D.stream, lambda: D.reproject_async(Col, None, D.stream), switch)
        rec["rt_reproject_async_ms_from_temporal_and_moments_planes"] = alternating(D.stream, lambda: D.reproject_async(S, None, D.stream), switch)
        D.set_temporal_moments({"k_min": 1.0})
        D.reproject_async(S, None, D.stream)                  # M is current from here, whatever the setting says afterwards
        D.read_moments()
        for levels in (0, 3):
            rec["rt_atrous_async_ms_levels_%d" % levels] = alternating(D.stream, lambda: D.atrous_async({"levels": levels}, D.stream), switch)
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


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def shadow_edges(truth, feat, spheres, w, h, step=0.35, reach=2):
    """Pixels within `reach` pixels of a pair of 4-neighbours of the truth frame that show the same DIFFUSE record with normals within 0.1 of each
    other and whose luminances, both below 1, differ by more than `step` of the larger (tests/test_moments_cpu.py states it at length)."""
    l = lum(np.asarray(truth, np.float64).reshape(h, w, 3))
    feat = np.asarray(feat, np.float32).reshape(h, w, 8)
    ids, N = feat[..., 7].view(np.uint32), feat[..., 3:6].astype(np.float64)
    refl = api.as_spheres(spheres)["refl"]
    diffuse = (ids < len(refl)) & (refl[np.minimum(ids, len(refl) - 1)] == 0)
    edge = np.zeros((h, w), bool)
    for dy, dx in ((0, 1), (1, 0)):
        a, b = (slice(0, h - dy), slice(0, w - dx)), (slice(dy, h), slice(dx, w))
        hi = np.maximum(l[a], l[b])
        pair = (ids[a] == ids[b]) & diffuse[a] & (((N[a] - N[b]) ** 2).sum(axis=-1) < 0.01) & (hi < 1.0) & (np.abs(l[a] - l[b]) > step * hi) & (hi > 0.02)
        edge[a] |= pair
        edge[b] |= pair
    near = np.zeros((h, w), bool)
    for y, x in zip(*np.nonzero(edge)):
        near[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
    return near


FRAMES, STEP = 8, 0.005
for case in args.quality.split(","):
    if not case:
        continue
    name, size = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    sph, orig, target = quality_scene(name)
    last = sideways(orig, target, FRAMES * STEP)
    with view(sph, orig, target, W, H, 0, 0) as A, view(sph, orig, target, W, H, 0, 0) as B, view(sph, last, target, W, H, 0, 1024) as truth:
        for f in range(1, FRAMES + 1):
            ctx, other = (A, B) if f % 2 else (B, A)
            ctx.set_temporal_moments({})
            ctx.set_camera(host.compute_camera(sideways(orig, target, f * STEP), target, W, H))
            ctx.seed_stream(f, ctx.stream)
            ctx.features_async(ctx.stream)
            ctx.render_async(2, ctx.stream)
            if f > 1:
                ctx.reproject_async(other, None, ctx.stream)
        ref = truth.read_colors().reshape(H, W, 3)
        near = shadow_edges(ref, truth.read_features(), sph, W, H)
        T, M = ctx.read_temporal(packed=False), ctx.read_moments()
        rec = {"case": "quality", "scene": name, "w": W, "h": H, "frames": FRAMES, "passes_per_frame": 2, "moved_by_per_frame": STEP, "truth_passes": 1024,
               "k_min": 4.0, "temporal_db": psnr8(T[..., 0:3], ref), "temporal_db_near_shadow_edges": psnr8(T[..., 0:3][near], ref[near]),
               "share_near_shadow_edges": round(float(near.mean()), 4), "share_at_k_min": round(float((M[..., 2] >= 4.0).mean()), 4)}
        for rule, setting in (("21", None), ("28", {})):
            ctx.set_temporal_moments(setting)
            whole, edges = {}, {}
            for n in (1, 3, 5):
                ctx.atrous_async({"levels": n}, ctx.stream)
                a = ctx.read_atrous(packed=False)[..., 0:3]
                whole[str(n)], edges[str(n)] = psnr8(a, ref), psnr8(a[near], ref[near])
            rec["rule_%s_db_by_levels" % rule], rec["rule_%s_db_near_shadow_edges_by_levels" % rule] = whole, edges
        emit(rec)
