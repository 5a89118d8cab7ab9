"""Feature planes (include/rt_api.h "feature planes", csrc/rt_features.hip), the part that needs no device: a numpy restatement of rules 10-12 in
whole-plane float32 operations, written independently of rt_host.cpp's loops; rt_features_planes against it bit for bit on the Demo scene, two
fixture scenes, a camera inside a sphere, identical spheres, sky, and records with NaN, infinite and zero radius; and the tie to the oracle's
pinned restatement of the reference's sphere test.  tests/test_gpu_feature_planes.py compares the device with rt_features_planes and imports the
scenes of this file."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host

F = np.float32
RT_ERR_ARG = -1
MISS = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the restatement ---------------------------------------------------------------------------------------------------
def rays_restated(cam, w, h):
    """Rule 10 for every pixel: (o, d), float32 [h, w, 3] each, IMAGE rows (row y = image row y); one float32 numpy operation per step."""
    cam = np.asarray(cam, F).reshape(5, 3)                   # orig, target, dir, x, y
    orig, cdir, cx, cy = cam[0], cam[2], cam[3], cam[4]
    kcx = ((np.arange(w).astype(F) + F(0.0)) * (F(1.0) / F(w)) - F(0.5))[None, :, None]
    kcy = ((np.arange(h).astype(F) + F(0.0)) * (F(1.0) / F(h)) - F(0.5))[:, None, None]
    rdir = (cx[None, None, :] * kcx + cy[None, None, :] * kcy) + cdir[None, None, :]
    o = F(0.1) * rdir + orig[None, None, :]
    dd = (rdir[..., 0] * rdir[..., 0] + rdir[..., 1] * rdir[..., 1]) + rdir[..., 2] * rdir[..., 2]
    d = rdir * (F(1.0) / np.sqrt(dd))[..., None]
    assert o.dtype == F and d.dtype == F
    return o, d


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def distances_restated(sph, o, d):
    """.cl:173-201 of every record for every ray: float32 [n, h, w], 0 = no hit."""
    out = np.zeros((len(sph),) + o.shape[:2], F)
    with np.errstate(all="ignore"):
        for i, s in enumerate(sph):
            op = np.asarray(s["p"], F)[None, None, :] - o
            b = _dot(op, d)
            det = b * b - _dot(op, op) + F(s["rad"]) * F(s["rad"])
            sq = np.sqrt(det)                                # NaN where det < 0 or det is a NaN
            t1, t2 = b - sq, b + sq
            dist = np.where(t1 > F(0.01), t1, np.where(t2 > F(0.01), t2, F(0.0)))
            out[i] = np.where(det < 0, F(0.0), dist)
    return out


def features_restated(sph, cam, w, h):
    """Rules 10-12: float32 [h, w, 8] in the colour plane's row order."""
    sph = api.as_spheres(sph)
    o, d = rays_restated(cam, w, h)
    t = np.full((h, w), F(1e20), F)
    idx = np.full((h, w), MISS, np.uint32)
    dist = distances_restated(sph, o, d)
    for i in range(len(sph)):                                # rule 11: scene order, a strict "<"
        nearer = (dist[i] != 0) & (dist[i] < t)
        t = np.where(nearer, dist[i], t)
        idx = np.where(nearer, np.uint32(i), idx)
    hit = t < F(1e20)
    out = np.zeros((h, w, 8), F)
    if len(sph):
        safe = np.where(hit, idx, 0)
        with np.errstate(all="ignore"):
            n = (o + d * t[..., None]) - sph["p"][safe].astype(F)
            n = n * (F(1.0) / np.sqrt(_dot(n, n)))[..., None]
            albedo = sph["c"][safe].astype(F) + sph["e"][safe].astype(F)
        out[..., 0:3] = np.where(hit[..., None], albedo, F(0.0))
        out[..., 3:6] = np.where(hit[..., None], n, F(0.0))
        out[..., 6] = np.where(hit, t, F(0.0))
    out[..., 7] = np.where(hit, idx, np.uint32(MISS)).astype(np.uint32).view(F)
    assert out.dtype == F
    return out[::-1].copy()                                  # image row y -> plane row h - 1 - y (.cl:579)


# ---- the scenes, shared with the device tests ------------------------------------------------------------------------------
def sphere(rad, p, e=(0, 0, 0), c=(0.5, 0.5, 0.5), refl=api.DIFF):
    return (rad, p, e, c, refl)


def records(rows):
    return np.array(rows, dtype=api.SPHERE_DT)


@functools.lru_cache(maxsize=None)
def fixture_scene(name, w, h):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cam = z["camera"].astype(F)
    return z["spheres"].view(api.SPHERE_DT).copy(), host.compute_camera(tuple(cam[0:3]), tuple(cam[3:6]), w, h)


def scene(name):
    """(records, camera, w, h) of a named case."""
    demo = host.demo_scene()
    if name.startswith("demo_"):
        w, h = (int(v) for v in name[5:].split("x"))
        return demo, host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h), w, h
    if name in ("cornell", "simple"):
        sph, cam = fixture_scene(name + "_96x96_4spp", 48, 32)
        return sph, cam, 48, 32
    w, h = 40, 24
    look = host.compute_camera((0.0, 0.0, 50.0), (0.0, 0.0, 0.0), w, h)
    if name == "inside":                                     # the camera inside a sphere: every ray takes the second root
        return records([sphere(100.0, (0, 0, 40), c=(0.2, 0.4, 0.6)), sphere(5.0, (0, 0, 0), e=(1, 2, 3))]), look, w, h
    if name == "identical":                                  # records 1 and 2 are one sphere: equal distances, the lower index wins
        return records([sphere(4.0, (-12, 0, 0)), sphere(8.0, (3, 1, 0), c=(0.9, 0.1, 0.1)), sphere(8.0, (3, 1, 0), c=(0.1, 0.9, 0.1))]), look, w, h
    if name == "sky":                                        # one small sphere: most rays miss
        return records([sphere(3.0, (2, -1, 0), c=(0.3, 0.3, 0.9))]), look, w, h
    if name == "empty":
        return records([])[:0], look, w, h
    if name == "nonfinite":                                  # NaN, infinite and zero radius, a NaN centre; the zero radius IS hit by the centre ray
        nan, inf = float("nan"), float("inf")
        o, d = rays_restated(look, w, h)
        for along in np.arange(20, 80, 0.25, dtype=F):       # a centre ON the ray of image pixel (0, 0) that the rounded test hits, and exactly AT the hit point
            p0 = o[0, 0] + d[0, 0] * along
            t = distances_restated(records([sphere(0.0, tuple(float(v) for v in p0))]), o[:1, :1], d[:1, :1])[0, 0, 0]
            if t != 0 and np.array_equal(o[0, 0] + d[0, 0] * t, p0):
                break
        else:
            raise AssertionError("no zero-radius centre with a NaN normal found")
        return records([sphere(nan, (0, 0, 0)), sphere(6.0, (nan, 0, 0)), sphere(inf, (0, 0, -10), c=(0.7, 0.7, 0.1)), sphere(0.0, tuple(float(v) for v in p0)),
                        sphere(5.0, (-8, 2, 0), c=(0.2, 0.8, 0.2)), sphere(-4.0, (9, -3, 0), e=(2, 2, 2))]), look, w, h
    raise KeyError(name)


SCENES = ["demo_1x1", "demo_41x23", "demo_70x19", "cornell", "simple", "inside", "identical", "sky", "empty", "nonfinite"]


def assert_same_plane(got, want):
    """Bit for bit, NaNs by position (a NaN normal's payload is not part of the rules)."""
    got, want = np.asarray(got, F).reshape(-1, 8), np.asarray(want, F).reshape(-1, 8)
    assert np.array_equal(got[:, 7].view(np.uint32), want[:, 7].view(np.uint32))
    g, w_ = got[:, :7], want[:, :7]
    assert np.array_equal(np.isnan(g), np.isnan(w_))
    ok = ~np.isnan(w_)
    assert np.array_equal(g[ok].view(np.uint32), w_[ok].view(np.uint32))


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    for name in ("rt_features_async", "rt_read_features", "rt_features_planes", "rt_set_denoise_guide", "rt_guide_defaults"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    assert callable(api.RtContext.features_async) and callable(api.RtContext.read_features) and callable(api.features_planes)


@pytest.mark.parametrize("name", SCENES)
def test_features_planes_equals_the_restatement_bit_for_bit(name):
    sph, cam, w, h = scene(name)
    got = api.features_planes(sph, cam, w, h)
    want = features_restated(sph, cam, w, h)
    assert got.shape == (h, w, 8)
    assert_same_plane(got, want)
    ids = got[..., 7].view(np.uint32)
    hit = ids != MISS
    assert ((ids < len(sph)) | ~hit).all()
    assert not got[~hit][:, :7].view(np.uint32).any()        # a miss: seven +0.0f
    if name == "inside":
        assert hit.all() and (got[..., 6] > 0).all()
    if name == "identical":
        assert (ids == 1).any() and not (ids == 2).any()
    if name in ("sky", "demo_41x23"):
        assert hit.any() and (~hit).any()
    if name == "empty":
        assert not hit.any()
    if name == "nonfinite":
        assert not np.isin(ids, (0, 1)).any()                # a NaN discriminant never hits
        assert set(np.unique(ids)) >= {3, 4, 5}              # the zero radius, the plain sphere, the negative radius (its square counts)
        zero = got[ids == 3]
        assert len(zero) == 1 and np.isnan(zero[0, 3:6]).all() and np.isfinite(zero[0, 6])      # a zero-radius hit: a NaN normal, stored as it is


def test_the_plane_is_in_the_colour_planes_row_order():
    """Row h - 1 - y of the plane is image row y: the ground (record 0) lies at the bottom of the Demo image, which is the plane's LAST rows."""
    sph, cam, w, h = scene("demo_41x23")
    ids = api.features_planes(sph, cam, w, h)[..., 7].view(np.uint32)
    assert (ids[h - 1] == 0).all() and (ids[0] != 0).any()


def test_index_and_distance_are_the_oracles_nearest_sphere():
    """Words 7 and 6 of every pixel of Demo 41x23 against the arg-min and minimum of the oracle's orc_sphere_intersect (the pinned restatement of the
    reference's SphereIntersect) over the scene, for the restated ray."""
    sph, cam, w, h = scene("demo_41x23")
    got = api.features_planes(sph, cam, w, h)[::-1]          # image rows
    o, d = rays_restated(cam, w, h)
    lib = O.oracle()
    recs = np.ascontiguousarray(sph).view(O.SPHERE_DT)
    for y in range(h):
        for x in range(w):
            oo, dd = (C.c_float * 3)(*o[y, x]), (C.c_float * 3)(*d[y, x])
            dist = np.array([lib.orc_sphere_intersect(C.c_void_p(recs[i:i + 1].ctypes.data), oo, dd) for i in range(len(recs))], F)
            cand = np.where(dist != 0, dist, F(np.inf))
            if np.isinf(cand.min()):
                assert got[y, x, 7].view(np.uint32) == MISS and got[y, x, 6] == 0
            else:
                assert got[y, x, 7].view(np.uint32) == int(cand.argmin()) and got[y, x, 6] == cand.min()


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    sph, cam, w, h = scene("sky")
    out = np.zeros((h, w, 8), F)
    p = api._ptr
    cam_a = api.as_camera(cam)
    for args in ((None, p(sph), 1, p(cam_a), w, h), (p(out), None, 1, p(cam_a), w, h), (p(out), p(sph), 1, None, w, h),
                 (p(out), p(sph), 1, p(cam_a), 0, h), (p(out), p(sph), 1, p(cam_a), w, -1)):
        assert lib.rt_features_planes(*args) == RT_ERR_ARG and lib.rt_last_error() != b""
    assert lib.rt_features_planes(p(out), None, 0, p(cam_a), w, h) == 0      # no records need no pointer
    assert lib.rt_features_async(None, None) == RT_ERR_ARG and lib.rt_read_features(None, p(out)) == RT_ERR_ARG
    assert lib.rt_set_denoise_guide(None, None) == RT_ERR_ARG
