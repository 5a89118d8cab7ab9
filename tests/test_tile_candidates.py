"""The tile certificate of the direct camera rays (csrc/rt_candidates.h, through rt_debug_tile_candidates: the text the
kernels' prologue runs, on the CPU): no sphere it certifies as a MISS for a tile may show a non-negative discriminant on
any camera ray of that tile, with the rays and the discriminant formed in binary32 by the kernel's own arithmetic
(rt_shade.inc.h camera_direction / camera_origin, rt_trace.inc.h unit / hit_pre).  Per tile: the four jitter corners of
every pixel and 64 random (pixel, jitter) pairs.  Prints the smallest margin it sees (run with -s)."""
import ctypes as C
import os

import numpy as np
import pytest

from raytracing_simple_amd import api, host, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


def masks_of(sph, cam, w, h, rank=0, nranks=1, tile_rows=8):
    lib = api.load_library(diag=True)
    sph = api.as_spheres(sph)
    cam = np.ascontiguousarray(cam, np.float32)
    rows = len(api.local_rows_of(h, rank, nranks, tile_rows))
    out = np.zeros(((rows + 7) // 8) * ((w + 7) // 8), np.uint64)
    rc = lib.rt_debug_tile_candidates(cam.ctypes.data_as(C.c_void_p), w, h, sph.ctypes.data_as(C.c_void_p), len(sph), rank, nranks, tile_rows,
                                      out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.rt_last_error()
    return out.reshape((rows + 7) // 8, (w + 7) // 8)


def tile_rays(cam, w, h, tx, ty, rng):
    """(o, d) of the tile's test rays, float32 [R, 3]: every pixel with the four jitter corners, 64 random ones."""
    px, py = np.meshgrid(np.arange(8 * tx, 8 * tx + 8), np.arange(8 * ty, 8 * ty + 8))
    px, py = px.ravel(), py.ravel()
    lo, hi = F(-0.5), F(0.5) - F(2.0 ** -23)                    # next_random_centred: k / 2^23 - 0.5, k in [0, 2^23)
    xs = np.concatenate([np.repeat(px, 4), rng.integers(8 * tx, 8 * tx + 8, 64)]).astype(F)
    ys = np.concatenate([np.repeat(py, 4), rng.integers(8 * ty, 8 * ty + 8, 64)]).astype(F)
    j1 = np.concatenate([np.tile(np.array([lo, hi, lo, hi], F), 64), (rng.integers(0, 1 << 23, 64) / F(1 << 23) - 0.5).astype(F)])
    j2 = np.concatenate([np.tile(np.array([lo, lo, hi, hi], F), 64), (rng.integers(0, 1 << 23, 64) / F(1 << 23) - 0.5).astype(F)])
    inv_w, inv_h = F(1) / F(w), F(1) / F(h)
    kcx = (xs + j1) * inv_w - F(0.5)
    kcy = (ys + j2) * inv_h - F(0.5)
    co, cd, cx, cy = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    rd = np.stack([cx[k] * kcx + cy[k] * kcy + cd[k] for k in range(3)], 1).astype(F)
    o = (rd * F(0.1) + co[None, :]).astype(F)
    dd = (rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2]
    d = (rd * (F(1) / np.sqrt(dd))[:, None]).astype(F)
    return o, d


def discriminants(o, d, p, r2):
    """hit_pre's det of every ray against one sphere, binary32, the kernel's association order"""
    op = (p[None, :] - o).astype(F)
    b = (op[:, 0] * d[:, 0] + op[:, 1] * d[:, 1]) + op[:, 2] * d[:, 2]
    return (b * b - ((op[:, 0] * op[:, 0] + op[:, 1] * op[:, 1]) + op[:, 2] * op[:, 2])) + r2


def check(sph, cam, w, h, seed=0):
    """-> (histogram of candidates per tile, largest det of a certified miss, smallest -det / L^2 of one)"""
    sph = api.as_spheres(sph)
    rng = np.random.default_rng(seed)
    masks = masks_of(sph, cam, w, h)
    hist = {}
    worst, tightest = -np.inf, np.inf
    with np.errstate(all="ignore"):
        r2 = (sph["rad"] * sph["rad"]).astype(F)
        for ty in range(masks.shape[0]):
            for tx in range(masks.shape[1]):
                m = int(masks[ty, tx])
                k = bin(m).count("1")
                hist[k] = hist.get(k, 0) + 1
                if k == len(sph):
                    continue
                o, d = tile_rays(cam, w, h, tx, ty, rng)
                for i in range(len(sph)):
                    if m >> i & 1:
                        continue
                    det = discriminants(o, d, sph["p"][i].astype(F), r2[i])
                    assert not np.isnan(det).any() and (det < 0).all(), (tx, ty, i, float(np.nanmax(det)))
                    worst = max(worst, float(det.max()))
                    L2 = float(((sph["p"][i].astype(np.float64) - cam[0:3]) ** 2).sum())
                    tightest = min(tightest, float(-det.max()) / L2)
    return hist, worst, tightest


@pytest.mark.parametrize("w,h", [(320, 184), (200, 120), (323, 181)])
def test_demo_scene_no_certified_miss_is_hit(w, h):
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    hist, worst, tightest = check(host.demo_scene(), cam, w, h)
    print("demo %dx%d: tiles by candidates %s, largest det of a certified miss %.4g, smallest -det / L^2 %.3g" % (w, h, sorted(hist.items()), worst, tightest))
    assert worst < 0
    if (w, h) == (320, 184):                                   # not vacuous: the certificate does clear most tiles of most spheres
        assert all(hist.get(k, 0) > 0 for k in (0, 1, 2, 3)), hist
        assert hist[0] >= 100 and hist[1] >= 400, hist
        assert max(hist) <= 3, hist


def test_sixteen_sphere_scene():
    sph, orig, target = scenes.demo_plus(16)
    cam = host.compute_camera(orig, target, 200, 120)
    hist, worst, tightest = check(sph, cam, 200, 120)
    print("16 spheres: tiles by candidates %s, largest det %.4g, smallest -det / L^2 %.3g" % (sorted(hist.items()), worst, tightest))
    assert worst < 0 and min(hist) < 16


def test_adversarial_fixtures():
    """cameras inside and on spheres, zero / tiny / huge / negative radii, far-away spheres, NaN and infinite records"""
    z = np.load(os.path.join(GOLDEN, "fuzz_candidates.npy"))
    cleared = 0
    for k, rec in enumerate(z):
        sph = rec["spheres"][:int(rec["n"])].copy()
        cam = host.compute_camera(tuple(float(v) for v in rec["orig"]), tuple(float(v) for v in rec["target"]), 64, 40)
        masks = masks_of(sph, cam, 64, 40)
        with np.errstate(all="ignore"):
            never = ~(np.isfinite(sph["p"]).all(1) & np.isfinite(sph["rad"]) & (sph["rad"] * sph["rad"] > 0))     # records that can never be certified
            inside = ((sph["p"].astype(np.float64) - cam[0:3]) ** 2).sum(1) <= sph["rad"].astype(np.float64) ** 2
        for i in np.nonzero(never | inside)[0]:
            assert ((masks >> np.uint64(i)) & np.uint64(1)).all(), (k, i)
        hist, worst, tightest = check(sph, cam, 64, 40, seed=k)
        print("fixture %d (%d spheres): tiles by candidates %s, largest det %.4g" % (k, len(sph), sorted(hist.items()), worst))
        cleared += sum(v for c, v in hist.items() if c < len(sph))
    assert cleared >= 100, cleared          # not vacuous: the certificate does clear spheres on these scenes (8 scenes of 40 tiles)


def test_random_cameras():
    rng = np.random.default_rng(7)
    sph = host.demo_scene()
    cleared, tightest_all = 0, np.inf
    for k in range(50):
        orig = tuple(float(v) for v in rng.uniform(-150, 150, 3))
        target = tuple(float(v) for v in rng.uniform(-30, 60, 3))
        w, h = [(64, 40), (72, 48), (41, 27)][k % 3]
        cam = host.compute_camera(orig, target, w, h)
        hist, worst, tightest = check(sph, cam, w, h, seed=k)
        cleared += sum(v for c, v in hist.items() if c < 6)
        tightest_all = min(tightest_all, tightest)
    print("50 random cameras: %d tiles with a certified miss, smallest -det / L^2 %.3g" % (cleared, tightest_all))
    assert cleared > 1000


def test_sharded_masks_are_the_unsharded_ones():
    """a rank's tiles are classified in IMAGE coordinates: two shards of 8-row tiles, reassembled, give the unsharded masks"""
    w, h = 200, 120
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    whole = masks_of(host.demo_scene(), cam, w, h)
    for rank in range(2):
        part = masks_of(host.demo_scene(), cam, w, h, rank=rank, nranks=2, tile_rows=8)
        assert np.array_equal(part, whole[rank::2])
