"""First-hit frames: the closest-hit decision of a whole render kernel for its camera rays, ray by ray, against binary64
(tests/test_fast_first_hit_cpu.py on the oracle, tests/test_gpu_fast_first_hit.py on every shipped rt_trace_fast_* instance).

THE TRICK.  An emitter ends a path (rt_shade.inc.h no_emission / emitted; the sweep's and the walk's hit branch): after ONE pass over a
scene in which EVERY sphere is an emitter the colour plane of a pixel is e_id * |n.d| of the sphere its camera ray hit, or three zeros for
a miss.  No light is sampled, nothing bounces, and the running average of pass 0 is the sample itself (fold_sample).  Sphere i gets the
emission (1, 1 + (i & 127) / 128, 1 + (i >> 7) / 128) -- up to 16 384 indices, x never 0 --, colour 0 and DIFF; geometry stays the maker's.

DECODING (derived, not measured).  Each channel is ONE rounded product e_c * |n.d| (the products with the throughput 1 and the sum with
the radiance 0 are exact, fused or not), the red channel |n.d| itself.  The quotients g / r and b / r, formed on the host in binary64,
are therefore within a relative 2u(1 + u) of the code e_c in [1, 2): (g / r - 1) * 128 lies within 128 * 2 * 2u(1 + u) = 3.1e-5 of an
integer in [0, 128), and neighbouring codes are a whole unit apart.  A pixel whose channels do not decode that way, or that are zero,
subnormal or not finite on a hit the reference decides, is a failure -- never an exclusion.

REFERENCE.  The seed pair of the default stream is replayed (mwc_word), the camera ray formed in binary64 WITH its envelope exactly as
_fast_reference.shade64(0, ...) does (rd, origin, e_unit), and pairs64 / scene64 run on it with those input envelopes, 256 rays at a
time (a table of 5000 records then stays below a gigabyte of host memory).  Where id_decided holds, hit or miss and the decoded index
must be binary64's; there the red channel must lie within the envelope the same running error gives for hp = o + d t,
nrm = e_unit(hp - p), e_dot(nrm, d).  The share of pixels the exclusion rule leaves out is capped at 2 % per scene (R.cap)."""
import functools
import os
import sys

import numpy as np

import _fast_reference as R
from raytracing_simple_amd import api, host, scenes

sys.path.insert(0, os.path.join(R.ROOT, "tools"))
from bvh_scenes import _many_spheres  # noqa: E402

F, D = np.float32, np.float64
W, H = 96, 64
CHUNK = 256
DECODE_MARGIN = 128.0 * 2.0 * 2.0 * R.U * (1.0 + R.U)
RECORDS = os.path.join(R.ROOT, "profiles", "r26_fast_first_hit.jsonl")

def _nearer(maker, share=0.35):
    """The maker's scene seen from `share` of the way out from its target to its camera.  The geometry is the maker's; the camera is
    this module's to choose, and from the makers' own (150 units from the spheres) binary32 resolves the discriminant of a sphere of
    radius 0.3 .. 1.2 so badly (module docstring of tests/_fast_reference.py: 12 u (b^2 + |op|^2), doubled by the camera ray's own
    envelope) that among 5000 of them 7 % of the pixels have an undecided pair: the cap of 2 % says such a frame tests too little."""
    def make():
        sph, orig, target = maker()
        return sph, tuple(float(t + share * (o - t)) for o, t in zip(orig, target)), target
    return make


SCENES = {
    "demo": lambda: (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET),
    "random64": lambda: scenes.random_spheres(64),
    "random65": lambda: scenes.random_spheres(65),
    "demo_plus16": lambda: scenes.demo_plus(16),
    "random256": lambda: scenes.random_spheres(256),
    "random1024": _nearer(lambda: scenes.random_spheres(1024)),
    "many2000": _nearer(lambda: _many_spheres(2000)),
    "many5000": _nearer(lambda: _many_spheres(5000), 0.15),        # (at 0.35 still 2.3 % under K.exact(); here 1.7 %, 760 spheres seen)
}


def all_emitters(spheres):
    """the maker's geometry, every record an emitter that carries its own index (module docstring)"""
    sph = api.as_spheres(spheres).copy()
    n = len(sph)
    assert n <= 16384
    i = np.arange(n)
    sph["e"] = np.stack([np.ones(n), 1.0 + (i & 127) / 128.0, 1.0 + (i >> 7) / 128.0], 1).astype(F)
    sph["c"] = 0
    sph["refl"] = api.DIFF
    return sph


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (records with the encoding, camera)"""
    sph, orig, target = SCENES[name]()
    return all_emitters(sph), host.compute_camera(orig, target, W, H)


def behind_the_winner(p, k):
    """scene64 leaves a ray out as soon as ONE of its pairs is undecided.  Among thousands of small spheres a camera ray passes the
    silhouette of some sphere within det's envelope on every seventh pixel (at 150 units binary32 resolves det to 0.05, a sphere of radius
    0.3 has r^2 = 0.09), yet most of those spheres lie BEHIND the sphere the ray hits.  Such a pair cannot matter: whatever the device
    decides about it, the distance it can return is at least  lb = (b - eb) - sqrt(det + edet) (1 + rounding)  (the nearer root of the
    largest discriminant its envelope allows, less the root's own rounding), and where lb lies beyond the upper end of the envelope of the
    nearest FULLY decided hit, that hit's distance is smaller on the device too.  Those pairs are taken out (no hit, decided) before
    scene64 runs; an undecided pair in front of, or within the envelopes of, the nearest decided hit still excludes the ray, and so does
    an undecided pair of a ray without a decided hit.  A condition on the reference alone, and it only adds comparisons."""
    with np.errstate(all="ignore"):
        ok = p["decided"] & (~p["hit"] | p["t_decided"])
        hi = np.where(ok & p["hit"], p["t"] + p["t_env"], np.inf).min(1)
        root = R.Err(np.maximum(p["det"].v + p["det"].e, 0.0)).sqrt(k.sqrt)
        near = (p["b"].v - p["b"].e) - (root.v + root.e)
        lb = near - R.U * np.abs(near) - R.TINY
        out = p["finite"] & ~ok & (lb > hi[:, None])
    q = dict(p)
    q["hit"], q["decided"] = p["hit"] & ~out, p["decided"] | out
    q["t_decided"] = p["t_decided"] & ~out
    return q


@functools.lru_cache(maxsize=None)
def reference(name, fast):
    """binary64's first hit of every pixel's first camera ray (gid order: y * W + x) under K.measured() (fast) or K.exact()"""
    k = R.K.measured() if fast else R.K.exact()
    assert k is not None
    sph, cam = scene(name)
    tab = R.table_of(sph)
    n_px = W * H
    seeds = api.stream_seeds(0, 2 * n_px)
    rec = np.zeros((n_px, 16), F)
    words = rec.view(np.uint32)
    words[:, 0], words[:, 1] = seeds[0::2], seeds[1::2]
    gid = np.arange(n_px)
    items, _, _ = R.shade64(0, rec, {"cam": np.asarray(cam, F), "w": W, "h": H, "px": gid % W, "py": gid // W}, k)
    o, d = items[1][2], items[2][2]
    out = {"id": np.zeros(n_px, np.int64), "any_hit": np.zeros(n_px, bool), "id_decided": np.zeros(n_px, bool),
           "nd": np.zeros(n_px, D), "nd_env": np.full(n_px, np.inf, D), "nd_ok": np.zeros(n_px, bool)}
    with np.errstate(all="ignore"):
        for a in range(0, n_px, CHUNK):
            sl = slice(a, min(a + CHUNK, n_px))
            oc, dc = [R.Err(c.v[sl], c.e[sl]) for c in o], [R.Err(c.v[sl], c.e[sl]) for c in d]
            p = behind_the_winner(R.pairs64(None, tab, k, oc, dc), k)
            s = R.scene64(p, np.full(len(oc[0].v), R.T_NONE, F))
            rows, win = np.arange(len(oc[0].v)), s["id"]
            t = R.Err(p["t"][rows, win], p["t_env"][rows, win])
            hp = [oc[j] + dc[j] * t for j in range(3)]
            nrm = R.e_unit([hp[j] - R.Err(tab[win, j].astype(D)) for j in range(3)], k)
            dp = R.e_dot(nrm, dc)
            out["id"][sl], out["any_hit"][sl], out["id_decided"][sl] = win, s["any_hit"], s["id_decided"]
            out["nd"][sl], out["nd_env"][sl] = np.abs(dp.v), dp.e
            out["nd_ok"][sl] = s["id_decided"] & s["any_hit"] & p["t_decided"][rows, win] & np.isfinite(dp.e) & np.isfinite(dp.v)
    out["n"] = len(sph)
    return out


def decode(colors):
    """the colour plane (read_colors' layout: row h - 1 - y) -> per pixel in gid order: channels [N, 3], hit, usable, valid code, index"""
    c = np.ascontiguousarray(colors, F).reshape(H, W, 3)[::-1].reshape(-1, 3)
    with np.errstate(all="ignore"):
        hit = (c != 0).any(1)                                                   # (a NaN channel counts as a hit and then fails to decode)
        usable = (np.isfinite(c) & (np.abs(c) >= F(2.0 ** -126))).all(1)
        r = c[:, 0].astype(D)
        q_lo, q_hi = (c[:, 1].astype(D) / r - 1.0) * 128.0, (c[:, 2].astype(D) / r - 1.0) * 128.0
        i_lo, i_hi = np.rint(q_lo), np.rint(q_hi)
        valid = usable & (np.abs(q_lo - i_lo) <= DECODE_MARGIN) & (np.abs(q_hi - i_hi) <= DECODE_MARGIN)
        valid &= (i_lo >= 0) & (i_lo < 128) & (i_hi >= 0) & (i_hi < 128)
        idx = np.where(valid, i_hi * 128 + i_lo, -1).astype(np.int64)
    return {"c": c, "hit": hit, "usable": usable, "valid": valid, "id": idx}


def check_frame(name, colors, ref, verbose=True):
    """The assertions of a first-hit frame against ref = reference(...).  -> {counts, the largest observed / bound of |n.d|}"""
    got = decode(colors)
    dec = ref["id_decided"]
    n_px = len(dec)
    sel = dec & ref["any_hit"]
    with np.errstate(all="ignore"):
        ratio = np.where(ref["nd_ok"], np.abs(got["c"][:, 0].astype(D) - ref["nd"]) / ref["nd_env"], 0.0)
    out = {"scene": name, "pixels": n_px, "decided": int(dec.sum()), "excluded": int((~dec).sum()), "hits": int(sel.sum()),
           "misses": int((dec & ~ref["any_hit"]).sum()), "spheres_seen": int(len(np.unique(ref["id"][sel]))),
           "nd_compared": int(ref["nd_ok"].sum()), "nd_ratio": float(np.nanmax(ratio)) if n_px else 0.0}
    if verbose:
        print("%-34s pixels %5d  excluded %4d (%.2f %%)  decided hits %5d on %4d spheres  misses %5d   |n.d| observed / bound %.3f over %d" % (
            name, n_px, out["excluded"], 100.0 * out["excluded"] / n_px, out["hits"], out["spheres_seen"], out["misses"], out["nd_ratio"],
            out["nd_compared"]))
    wrong = dec & (got["hit"] != ref["any_hit"])
    assert not wrong.any(), (name, "hit / miss differs from binary64 away from a tie", np.nonzero(wrong)[0][:4].tolist())
    bad = sel & ~got["usable"]
    assert not bad.any(), (name, "a decided hit with zero, subnormal or non-finite channels", np.nonzero(bad)[0][:4].tolist(), got["c"][bad][:4].tolist())
    bad = sel & ~got["valid"]
    assert not bad.any(), (name, "a decided hit whose channels are no index's code", np.nonzero(bad)[0][:4].tolist(), got["c"][bad][:4].tolist())
    wrong = sel & (got["id"] != ref["id"])
    assert not wrong.any(), (name, "another sphere wins away from a tie: pixel, got, binary64", np.nonzero(wrong)[0][:4].tolist(),
                             got["id"][wrong][:4].tolist(), ref["id"][wrong][:4].tolist())
    assert not np.isnan(ratio).any() and out["nd_ratio"] <= 1.0, (name, "|n.d| outside its envelope", out["nd_ratio"], int(np.nanargmax(ratio)))
    # (id_decided implies a decided root; the envelope of |n.d| is infinite where that of the hit point reaches the sphere's radius --
    # a sphere of radius 0.3 at 100 units, one pixel in 5000 -- and says nothing there)
    assert out["nd_compared"] >= 0.99 * out["hits"], (name, "|n.d| is hardly compared", out)
    R.cap(name + " first hits", out["excluded"], n_px)
    assert out["hits"] > n_px // 8 and out["spheres_seen"] >= min(4, ref["n"] - 1), (name, "vacuous", out)
    return out


def tampered(colors, ref, share=0.01, seed=1):
    """the frame with `share` of the decided hits' indices replaced by a neighbouring index (the red channel kept)"""
    out = np.array(colors, F).reshape(H, W, 3)[::-1].reshape(-1, 3).copy()
    sel = np.nonzero(ref["id_decided"] & ref["any_hit"])[0]
    pick = np.random.default_rng(seed).choice(sel, max(1, int(round(share * len(sel)))), replace=False)
    other = np.where(ref["id"][pick] + 1 < ref["n"], ref["id"][pick] + 1, ref["id"][pick] - 1)
    out[pick, 1] = out[pick, 0] * (F(1) + (other & 127).astype(F) / F(128))
    out[pick, 2] = out[pick, 0] * (F(1) + (other >> 7).astype(F) / F(128))
    return out.reshape(H, W, 3)[::-1].reshape(-1).copy(), len(pick)


def render(name, diag=False, knobs=(), inst=None):
    """One pass of fast mode over scene `name` -> (colour plane, rt_last_kernel).  knobs: [(rt_debug_* setter, its arguments)], set before
    the scene as tests/test_gpu_bvh.py _render does; inst: an instance of the diagnostics library by its symbol."""
    sph, cam = scene(name)
    with api.RtContext(W, H, diag=diag or bool(knobs) or inst is not None) as ctx:
        for setter, args in knobs:
            ctx._check(getattr(ctx._lib, setter)(ctx._h, *args))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.set_mode(api.instance_mode(inst) if inst else api.RT_MODE_FAST)
        ctx.render_pass(1)
        return ctx.read_colors(), ctx.last_kernel
