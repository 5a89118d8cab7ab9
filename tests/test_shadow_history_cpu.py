"""Shadow-aware history (include/rt_api.h "shadow-aware history", csrc/rt_reproject.hip), the part that needs no device: a numpy restatement of
rules 29-32 in whole-plane float32 operations, written independently of rt_host.cpp's loops; rt_reproject_shadow_planes against it bit for bit on the
geometries of tests/test_reproject_cpu.py with records moved, resized and broken; the invariants; the pair order; the refusals; and the quality the
header quotes, with frames of the oracle alone.  tests/test_gpu_shadow_history.py compares the device with the host function."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import _build, api, host
from test_atrous_cpu import assert_same_plane, lum
from test_features_cpu import _dot, rays_restated
from test_moments_cpu import synthetic_moments
from test_reproject_cpu import F, _image, geometry, psnr8, quality_setup, synthetic

RT_ERR_ARG = -1
LIGHT = 5                                                        # the Demo scene's emitter


# ---- the restatement ---------------------------------------------------------------------------------------------------
def pairs_restated(sphS, sphD):
    """Rule 29: [(l, j)] in order.  Words are compared as bits."""
    sphS, sphD = api.as_spheres(sphS), api.as_spheres(sphD)
    words = lambda s: np.concatenate([s["p"].astype(F).reshape(-1, 3), s["rad"].astype(F).reshape(-1, 1)], axis=1).view(np.uint32)      # noqa: E731
    changed = (words(sphS) != words(sphD)).any(axis=1)
    phantom = (sphS["rad"] == 0) & (sphD["rad"] == 0)
    light = ~((sphD["e"][:, 0] == 0) & (sphD["e"][:, 2] == 0)) & ~phantom
    return [(l, j) for l in range(len(sphD)) if light[l] for j in range(len(sphD)) if j != l and not phantom[j] and (changed[l] or changed[j])]


def state_restated(X, L, rl, c, r):
    """Rule 30 at every point of X [h, w, 3]: int [h, w]."""
    L, c, rl, r = np.asarray(L, F), np.asarray(c, F), F(rl), F(r)
    seg = L[None, None, :] - X
    ll = _dot(seg, seg)
    s = _dot(c[None, None, :] - X, seg) / ll
    s = np.where(s > F(0.0), s, F(0.0))
    s = np.where(s > F(1.0), F(1.0), s)
    e = (X + seg * s[..., None]) - c[None, None, :]
    d2, pen = _dot(e, e), rl * s
    a, b = r + pen, r - pen
    state = np.where(d2 > a * a, 0, np.where((b > F(0.0)) & (d2 < b * b), 2, 1))
    assert d2.dtype == F and a.dtype == F
    return np.where(ll > F(0.0), state, 0)


def shadow_restated(dst, src, w, h, src_m=None, keep=2.0, k_pos=4.0, max_history=64.0):
    """Rules 15-19, 25-27 and 29-32 for every pixel at once: (T, M, K) in the colour plane's row order.  The taps are written out once more: the
    restatements of tests/test_reproject_cpu.py and tests/test_moments_cpu.py keep their sums to themselves."""
    k_pos, max_history, keep = F(k_pos), F(max_history), F(keep)
    sphD, sphS = api.as_spheres(dst["spheres"]), api.as_spheres(src["spheres"])
    count = len(sphD)
    camS = np.asarray(src["cam"], F).reshape(5, 3)
    origS, dirS, cxS, cyS = camS[0], camS[2], camS[3], camS[4]
    FD, FS = _image(dst["feat"], w, h), _image(src["feat"], w, h)
    U = _image(src["plane"], w, h)
    MS = _image(src_m, w, h) if src_m is not None else None
    nd = F(dst["passes"])
    with np.errstate(all="ignore"):
        idD, tD = FD[..., 7].view(np.uint32), FD[..., 6]
        known = idD < np.uint32(count)
        safe = np.where(known, idD, 0).astype(np.int64)
        oD, dD = rays_restated(dst["cam"], w, h)
        P = oD + dD * tD[..., None]
        Pp = P - (sphD["p"][safe].astype(F) - sphS["p"][safe].astype(F))
        v = Pp - origS[None, None, :]
        z = _dot(v, dirS)
        kx = (_dot(v, cxS) * _dot(dirS, dirS)) / (z * _dot(cxS, cxS))
        ky = (_dot(v, cyS) * _dot(dirS, dirS)) / (z * _dot(cyS, cyS))
        fx, fy = (kx + F(0.5)) * F(w), (ky + F(0.5)) * F(h)
        seen = known & (z > F(0.0)) & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix0, iy0 = np.where(seen, x0, F(0.0)).astype(np.int64), np.where(seen, y0, F(0.0)).astype(np.int64)
        oS, dS = rays_restated(src["cam"], w, h)
        foot = np.sqrt(_dot(cxS, cxS)) * (F(1.0) / F(w))
        zero = np.zeros((h, w), F)
        sw, sn, s1, s2, sk, sc = zero, zero, zero, zero, zero, np.zeros((h, w, 3), F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix0 + i, iy0 + j
                b = (ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Fq, Uq = FS[cy, cx], U[cy, cx]
                tq = Fq[..., 6]
                e = (oS[cy, cx] + dS[cy, cx] * tq[..., None]) - Pp
                r = k_pos * (tq * foot)
                un = Uq[..., 3] if U.shape[-1] == 4 else np.full((h, w), F(src["passes"]), F)
                take = (seen & inside & (Fq[..., 7].view(np.uint32) == idD) & (_dot(e, e) <= r * r) & np.isfinite(Uq[..., 0:3]).all(axis=-1)
                        & (un > F(0.0)))
                if MS is not None:
                    m1q, m2q, kq = MS[cy, cx][..., 0], MS[cy, cx][..., 1], MS[cy, cx][..., 2]
                else:
                    lq = lum(Uq)
                    m1q, m2q, kq = lq, lq * lq, np.ones((h, w), F)
                sw = np.where(take, sw + b, sw)
                sn = np.where(take, sn + b * un, sn)
                sc = np.where(take[..., None], sc + b[..., None] * Uq[..., 0:3], sc)
                s1 = np.where(take, s1 + b * m1q, s1)
                s2 = np.where(take, s2 + b * m2q, s2)
                sk = np.where(take, sk + b * kq, sk)
        have = sw > F(0.0)
        # 31. the flag
        K = np.zeros((h, w), bool)
        if dst["passes"] != 0:
            for l, j in pairs_restated(sphS, sphD):
                before = state_restated(Pp, sphS["p"][l], sphS["rad"][l], sphS["p"][j], sphS["rad"][j])
                after = state_restated(P, sphD["p"][l], sphD["rad"][l], sphD["p"][j], sphD["rad"][j])
                K |= have & (idD != np.uint32(l)) & (idD != np.uint32(j)) & ((before != after) | (before == 1) | (after == 1))
        # 18, 26: the caps; 32: the cap of a flagged pixel
        H, h1, h2, hk, nh = sc / sw[..., None], s1 / sw, s2 / sw, sk / sw, sn / sw
        over = nh > max_history
        hk = np.where(over, hk * (max_history / nh), hk)
        nh = np.where(over, max_history, nh)
        cut = K & (nh > keep)
        hk = np.where(cut, hk * (keep / nh), hk)
        nh = np.where(cut, keep, nh)
        # 19, 27: the blends
        T = np.zeros((h, w, 4), F)
        if dst["passes"] == 0:
            T[..., 0:3] = np.where(have[..., None], H, F(0.0))
            T[..., 3] = np.where(have, nh, nd)
            m1, m2, k = np.where(have, h1, F(0.0)), np.where(have, h2, F(0.0)), np.where(have, hk, F(0.0))
        else:
            CD = _image(dst["plane"], w, h)[..., 0:3]
            lD = lum(CD)
            inv = F(1.0) / (nd + nh)
            T[..., 0:3] = np.where(have[..., None], (CD * nd + H * nh[..., None]) * inv[..., None], CD)
            T[..., 3] = np.where(have, nd + nh, nd)
            m1 = np.where(have, (lD * nd + h1 * nh) * inv, lD)
            m2 = np.where(have, ((lD * lD) * nd + h2 * nh) * inv, lD * lD)
            k = np.where(have, hk + F(1.0), F(1.0))
        d = m2 - m1 * m1
        var = np.where((k > F(1.0)) & (d > F(0.0)), d / (k - F(1.0)), F(0.0))
        M = np.stack([m1, m2, k, var], axis=-1)
    assert T.dtype == F and M.dtype == F
    return T[::-1].copy(), M[::-1].copy(), K[::-1].astype(np.uint8)


# ---- the cases, shared with the device tests ------------------------------------------------------------------------------
SIZES = ["demo_41x23_sphere", "demo_70x19_translated", "demo_1x1_translated"]
VARIANTS = ["moved", "radius", "light", "nan"]


def records(name, variant="moved"):
    """(records of D, records of S, camera of D, camera of S, w, h): tests/test_reproject_cpu.py's geometry with D's records changed --
    moved: record 3 moved (the `sphere` geometry moves it itself); radius: record 3 grown where it stood; light: the emitter moved, so that every
    record pairs with it; nan: record 4's centre broken in D; none: nothing changed."""
    sphD, sphS, camD, camS, w, h = geometry(name)
    sphD = sphS.copy() if variant != "moved" else sphD.copy()
    if variant == "moved":
        if not name.endswith("_sphere"):
            sphD["p"][3] += np.array((7.0, 1.5, -2.0), F)
    elif variant == "radius":
        sphD["rad"][3] = F(14.0)
    elif variant == "light":
        sphD["p"][LIGHT] += np.array((-9.0, 3.0, 4.0), F)
    elif variant == "nan":
        sphD["p"][4][0] = np.nan
    elif variant != "none":
        raise KeyError(variant)
    return sphD, sphS, camD, camS, w, h


@functools.lru_cache(maxsize=None)
def shadow_sides(name, variant, channels, passes_d, src_passes=16):
    """The two dicts api.reproject_shadow_planes takes, with synthetic planes (tests/test_reproject_cpu.py's sides, with these records)."""
    sphD, sphS, camD, camS, w, h = records(name, variant)
    dst = {"plane": synthetic(w, h, 3, False)[::-1, ::-1] if passes_d else None, "passes": passes_d, "feat": api.features_planes(sphD, camD, w, h), "cam": camD,
           "spheres": sphD}
    src = {"plane": synthetic(w, h, channels), "passes": src_passes, "feat": api.features_planes(sphS, camS, w, h), "cam": camS, "spheres": sphS}
    return dst, src, w, h


def dust(n_small, w=41, h=23):
    """A scene of `n_small` small spheres above a ground sphere under one light, every small sphere moved in D: n_small pairs with the light
    (the ground, which stays, pairs with nothing).  (records of D, records of S, camera, w, h)"""
    rng = np.random.default_rng(5 + n_small)
    sph = np.zeros(n_small + 2, api.SPHERE_DT)
    sph[0] = (1000.0, (0.0, -1000.0, 0.0), (0.0, 0.0, 0.0), (0.7, 0.7, 0.7), 0)
    sph[1] = (7.0, (0.0, 60.0, 0.0), (12.0, 12.0, 12.0), (0.0, 0.0, 0.0), 0)
    for k in range(n_small):
        sph[2 + k] = (1.5, (rng.uniform(-45, 45), rng.uniform(4, 30), rng.uniform(-30, 10)), (0.0, 0.0, 0.0), tuple(rng.uniform(0.2, 0.9, 3)), 0)
    moved = sph.copy()
    moved["p"][2:] += np.array((3.0, 0.0, 0.0), F)
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    return moved, sph, cam, w, h


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    lib = api.load_library()
    for name in ("rt_shadow_history_defaults", "rt_set_shadow_history", "rt_read_history_flags", "rt_reproject_shadow_planes", "rt_shadow_history_pairs"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    for name in ("set_shadow_history", "read_history_flags", "shadow_history_defaults"):
        assert callable(getattr(api.RtContext, name))
    assert callable(api.reproject_shadow_planes) and callable(api.shadow_history_pairs)
    d = api.shadow_history_defaults()
    assert C.sizeof(d) == 16 and d.as_dict() == {"keep": 2.0, "reserved": [0, 0, 0]}
    header = open(_build.ROOT + "/include/rt_api.h").read()
    assert "#define RT_SHADOW_PAIR_CHUNK %d " % api.SHADOW_PAIR_CHUNK in header


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SIZES)
def test_reproject_shadow_planes_equals_the_restatement_bit_for_bit(name, variant, channels):
    """Every geometry with every change of the records, src_m none and synthetic, keep 0, 2 and 100 (above max_history), nd 2."""
    dst, src, w, h = shadow_sides(name, variant, channels, 2)
    flagged = 0
    for src_m in (None, synthetic_moments(w, h)):
        for keep in (0.0, 2.0, 100.0):
            T, M, K = api.reproject_shadow_planes(dst, src, w, h, src_m, None, {"keep": keep})
            rT, rM, rK = shadow_restated(dst, src, w, h, src_m, keep)
            assert np.array_equal(K, rK) and set(np.unique(K)) <= {0, 1}
            assert_same_plane(T, rT)
            assert_same_plane(M, rM)
            flagged += int(K.sum())
            if keep == 0.0 and K.any():                          # rule 32: with keep 0 a flagged pixel comes out as (CD, nd)
                CD = np.asarray(dst["plane"], F).reshape(h, w, 3)
                assert np.array_equal(T[K == 1][:, 0:3], CD[K == 1]) and (T[K == 1][:, 3] == F(2.0)).all()
    if w > 8:
        assert flagged > 0                                       # (no case is vacuous)


def test_flagged_and_unflagged_pixels_exist_and_lie_where_the_shadow_moved():
    dst, src, w, h = shadow_sides("demo_41x23_sphere", "moved", 4, 2)
    T, M, K = api.reproject_shadow_planes(dst, src, w, h, None, None, {})
    plain = api.reproject_planes(dst, src, w, h)
    took = plain[..., 3] != F(2.0)
    assert K.any() and (took & (K == 0)).any() and not (K[~took]).any()          # only pixels with history are flagged
    ids = np.asarray(dst["feat"], F).reshape(h, w, 8)[..., 7].view(np.uint32)
    assert not (K[(ids == 3) | (ids == LIGHT)]).any()            # neither the moved sphere nor the light flags itself (its only pairs hold it)
    assert (ids[K == 1] == 0).any()                              # the ground under the sphere is among the flagged
    differs = (T.view(np.uint32) != plain.view(np.uint32)).any(axis=-1)
    assert differs.any() and not differs[K == 0].any()           # rule 32 touches flagged pixels only


def test_a_nan_centre_gives_state_1_everywhere():
    """Rule 30: a NaN fails every comparison.  D's record 4 has a NaN centre: `after` is 1 for its pair, so every pixel with history that shows
    neither the light nor record 4 is flagged."""
    dst, src, w, h = shadow_sides("demo_41x23_sphere", "nan", 4, 2)
    X = np.zeros((2, 2, 3), F)
    assert (state_restated(X, (0, 60, 0), 7.0, (np.nan, 10, -5), 9.0) == 1).all()
    T, M, K = api.reproject_shadow_planes(dst, src, w, h, None, None, {})
    ids = np.asarray(dst["feat"], F).reshape(h, w, 8)[..., 7].view(np.uint32)
    took = api.reproject_planes(dst, src, w, h)[..., 3] != F(2.0)
    assert np.array_equal(K == 1, took & (ids != 4) & (ids != LIGHT)) and K.any()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", SIZES)
def test_invariant_a_no_changed_record_is_the_setting_off(name, channels):
    dst, src, w, h = shadow_sides(name, "none", channels, 2)
    assert len(api.shadow_history_pairs(src["spheres"], dst["spheres"])) == 0
    for src_m in (None, synthetic_moments(w, h)):
        T, M, K = api.reproject_shadow_planes(dst, src, w, h, src_m, None, {"keep": 0.0})
        pT, pM = api.reproject_moments_planes(dst, src, w, h, src_m)
        assert_same_plane(T, pT)
        assert_same_plane(T, api.reproject_planes(dst, src, w, h))
        assert_same_plane(M, pM)
        assert not K.any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_invariant_b_keep_at_max_history_is_the_plain_planes_with_flags(variant):
    dst, src, w, h = shadow_sides("demo_41x23_sphere", variant, 4, 2)
    for src_m in (None, synthetic_moments(w, h)):
        for keep, params in ((64.0, None), (1e6, None), (10.0, {"max_history": 10.0})):
            T, M, K = api.reproject_shadow_planes(dst, src, w, h, src_m, params, {"keep": keep})
            pT, pM = api.reproject_moments_planes(dst, src, w, h, src_m, params)
            assert_same_plane(T, pT)
            assert_same_plane(M, pM)
            assert K.any()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SIZES)
def test_invariant_c_at_pass_0_nothing_is_flagged(name, variant):
    dst, src, w, h = shadow_sides(name, variant, 4, 0)
    T, M, K = api.reproject_shadow_planes(dst, src, w, h, None, None, {"keep": 0.0})
    assert not K.any()
    assert_same_plane(T, api.reproject_planes(dst, src, w, h))
    rT, rM, rK = shadow_restated(dst, src, w, h, None, 0.0)
    assert_same_plane(T, rT)
    assert_same_plane(M, rM)


def test_without_shadow_parameters_it_is_the_two_older_functions():
    dst, src, w, h = shadow_sides("demo_41x23_sphere", "moved", 4, 2)
    src_m = synthetic_moments(w, h)
    T, M, K = api.reproject_shadow_planes(dst, src, w, h, src_m, None, None)
    pT, pM = api.reproject_moments_planes(dst, src, w, h, src_m)
    assert_same_plane(T, pT)
    assert_same_plane(M, pM)
    assert not K.any()
    T2, none, K2 = api.reproject_shadow_planes(dst, src, w, h, None, None, {}, moments=False)
    assert none is None and K2.any()
    assert_same_plane(T2, api.reproject_shadow_planes(dst, src, w, h, src_m, None, {})[0])      # the colour does not depend on the moments arm


def test_the_pair_order():
    """Rule 29: l ascending outer, j ascending inner; phantoms in no pair; an unchanged light pairs with changed records only, a changed one with all."""
    sph = np.zeros(8, api.SPHERE_DT)
    for k in range(8):
        sph[k] = (2.0 + k, (10.0 * k, 5.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 0)
    sph["rad"][2] = 0.0                                          # a phantom
    sph["e"][1] = (0.0, 0.0, 3.0)                                # lights: the test reads words x and z of the emission
    sph["e"][6] = (3.0, 0.0, 0.0)
    sph["e"][4] = (0.0, 9.0, 0.0)                                # (y alone makes no light)
    new = sph.copy()
    new["p"][3][1] = 6.0                                         # a moved record
    new["rad"][7] = 1.0                                          # a resized one
    new["c"][0] = (0.1, 0.1, 0.1)                                # a colour is not among the four words
    got = api.shadow_history_pairs(sph, new)
    assert got.tolist() == [[1, 3], [1, 7], [6, 3], [6, 7]] == [list(p) for p in pairs_restated(sph, new)]
    new["p"][6][0] = np.nextafter(new["p"][6][0], F(0.0))        # the second light moved by one unit in the last place: it pairs with every record
    got = api.shadow_history_pairs(sph, new)
    assert got.tolist() == [[1, 3], [1, 6], [1, 7], [6, 0], [6, 1], [6, 3], [6, 4], [6, 5], [6, 7]] == [list(p) for p in pairs_restated(sph, new)]
    new = sph.copy()
    new["p"][0][0] = F(-0.0)                                     # +0.0f against -0.0f: equal as numbers, changed as words
    new["rad"][2] = 1.0                                          # a phantom on one side only is a record
    assert api.shadow_history_pairs(sph, new).tolist() == [[1, 0], [1, 2], [6, 0], [6, 2]] == [list(p) for p in pairs_restated(sph, new)]
    assert len(api.shadow_history_pairs(sph, sph)) == 0 and len(api.shadow_history_pairs(sph[:0], sph[:0])) == 0
    for n in (api.SHADOW_PAIR_CHUNK, api.SHADOW_PAIR_CHUNK + 1):   # the device tests' scenes: exactly one chunk, and one pair more
        sphD, sphS, _, _, _ = dust(n)
        assert len(api.shadow_history_pairs(sphS, sphD)) == n


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    dst, src, w, h = shadow_sides("demo_41x23_sphere", "moved", 4, 2)
    nan, inf = float("nan"), float("inf")
    for bad in (-1.0, -1e-30, nan, inf, -inf):
        with pytest.raises(api.RtError) as err:
            api.reproject_shadow_planes(dst, src, w, h, None, None, {"keep": bad})
        assert err.value.code == RT_ERR_ARG and "keep" in str(err.value)
    for slot in range(3):
        p = api.shadow_history_defaults()
        p.reserved[slot] = 1
        with pytest.raises(api.RtError) as err:
            api.reproject_shadow_planes(dst, src, w, h, None, None, p)
        assert err.value.code == RT_ERR_ARG and "reserved" in str(err.value)
    api.reproject_shadow_planes(dst, src, w, h, None, None, {"keep": 0.0})         # the smallest keep there is
    for name, bad in (("k_pos", 0.0), ("max_history", nan)):
        with pytest.raises(api.RtError) as err:
            api.reproject_shadow_planes(dst, src, w, h, None, {name: bad}, {})
        assert err.value.code == RT_ERR_ARG and name in str(err.value)
    with pytest.raises(ValueError):
        api.reproject_shadow_planes(dst, src, w, h, None, None, {"kept": 2.0})
    with pytest.raises(ValueError):
        api.reproject_shadow_planes(dst, src, w, h, synthetic_moments(w, h)[..., 0:2])
    with pytest.raises(ValueError):
        api.shadow_history_pairs(dst["spheres"], src["spheres"][:3])
    # null arguments, straight at the C functions
    keep, views, count = api._reproject_views(dst, src, w, h)
    T, K = np.zeros((h, w, 4), F), np.zeros((h, w), np.uint8)
    sp = api.shadow_history_defaults()
    call = lambda o, k, d, s: lib.rt_reproject_shadow_planes(o, None, k, d, s, None, count, w, h, None, C.byref(sp))      # noqa: E731
    assert call(None, api._ptr(K), C.byref(views[0]), C.byref(views[1])) == RT_ERR_ARG and b"rt_reproject_shadow_planes" in lib.rt_last_error()
    assert call(api._ptr(T), api._ptr(K), None, C.byref(views[1])) == RT_ERR_ARG and call(api._ptr(T), api._ptr(K), C.byref(views[0]), None) == RT_ERR_ARG
    assert not T.any() and not K.any()
    assert call(api._ptr(T), None, C.byref(views[0]), C.byref(views[1])) == 0 and T.any()          # K and M are optional
    assert lib.rt_set_shadow_history(None, None) == RT_ERR_ARG and lib.rt_set_shadow_history(None, C.byref(sp)) == RT_ERR_ARG
    assert lib.rt_read_history_flags(None, api._ptr(K)) == RT_ERR_ARG
    assert lib.rt_shadow_history_pairs(None, None, 3, None, 0) == -1 and lib.rt_shadow_history_pairs(None, None, 0, None, 0) == 0
    lib.rt_shadow_history_defaults(None)                         # a null pointer is ignored


# ---- what it is for ---------------------------------------------------------------------------------------------------
FRAMES, LEVELS = 12, 3
# scene -> (the record that moves, its step per frame)
MOVES = {"cornell": (16, (-1.5, 0.0, 0.0)), "demo": (4, (-2.0, 0.0, 0.0)), "simple": (6, (-2.5, 0.0, 0.0))}


@functools.lru_cache(maxsize=None)
def quality(name, w=96, h=96, truth=512, keep=2.0):
    """The interactive loop on the CPU with a moving sphere: FRAMES frames of 2 oracle passes, frame f on seed stream f with the record moved by
    (f - 1) steps, the camera still, each reprojected (defaults) from the frame before -- two sides taking turns -- once with the setting off and
    once with it on, then filtered at LEVELS levels.  Returns a dict of PSNRs against `truth` oracle passes of the last frame's scene: T and A, off
    and on; A over the CHANGED REGION -- pixels whose first hit is the same record as with the sphere where it stood six frames earlier, both truth
    luminances below 1 and differing by more than 25 % of the larger: where the direct light changed -- with that region's share; and the share of
    pixels the last frame flagged."""
    sph0, o, _, t = quality_setup(name, w, h)
    record, step = MOVES[name]
    cam = host.compute_camera(o, t, w, h)
    T = {False: None, True: None}
    feat = sph = K = None
    for f in range(1, FRAMES + 1):
        sph_f = sph0.copy()
        sph_f["p"][record] += (f - 1) * np.asarray(step, F)
        D = O.render(sph_f, cam, w, h, 2, seeds_in=api.stream_seeds(f, 2 * w * h), threads=16)["colors"]
        feat_f = api.features_planes(sph_f, cam, w, h)
        for on in (False, True):
            if f == 1:
                T[on] = D                                        # the first frame has nothing to reproject from: its colour plane stands
            else:
                dst = {"plane": D, "passes": 2, "feat": feat_f, "cam": cam, "spheres": sph_f}
                src = {"plane": T[on], "passes": 2, "feat": feat, "cam": cam, "spheres": sph}
                T[on], _, K = api.reproject_shadow_planes(dst, src, w, h, None, None, {"keep": keep} if on else None, moments=False)
        feat, sph = feat_f, sph_f
    ref3 = np.asarray(O.render(sph, cam, w, h, truth, threads=16)["colors"], F).reshape(h, w, 3)
    earlier = sph0.copy()
    earlier["p"][record] += (FRAMES - 7) * np.asarray(step, F)
    was3 = np.asarray(O.render(earlier, cam, w, h, truth, threads=16)["colors"], F).reshape(h, w, 3)
    ids = lambda f: np.asarray(f, F).reshape(h, w, 8)[..., 7].view(np.uint32)      # noqa: E731
    l_now, l_was = lum(ref3).astype(np.float64), lum(was3).astype(np.float64)
    hi = np.maximum(l_now, l_was)
    changed = (ids(feat) == ids(api.features_planes(earlier, cam, w, h))) & (hi < 1.0) & (np.abs(l_now - l_was) > 0.25 * hi)
    out = {"flagged": float(K.mean()), "changed": float(changed.mean())}
    for on in (False, True):
        A = api.atrous_planes(T[on], feat, w, h, 0, {"levels": LEVELS})
        out["T", on], out["A", on] = psnr8(T[on][..., 0:3], ref3), psnr8(A[..., 0:3], ref3)
        out["A_changed", on] = psnr8(A[..., 0:3][changed], ref3[changed])
    return out


# what this set-up measured with the defaults (include/rt_api.h quotes it), dB: A at three levels over the whole frame, the setting off and on
MEASURED = {"cornell": (24.56, 25.52), "demo": (25.58, 26.65), "simple": (28.26, 28.53)}


@pytest.mark.parametrize("name", ["cornell", "demo", "simple"])
def test_the_filtered_frame_is_closer_to_the_truth_with_the_setting_on(name, capsys):
    q = quality(name)
    with capsys.disabled():
        print("\n[shadow history] %s 96x96, %d frames of 2 passes, record %d moving: T %.2f -> %.2f dB, A at %d levels %.2f -> %.2f dB (%+.2f); "
              "over the changed region (%.1f %% of the frame) %.2f -> %.2f dB; %.1f %% of pixels flagged in the last frame"
              % (name, FRAMES, MOVES[name][0], q["T", False], q["T", True], LEVELS, q["A", False], q["A", True], q["A", True] - q["A", False],
                 100 * q["changed"], q["A_changed", False], q["A_changed", True], 100 * q["flagged"]))
    m_off, m_on = MEASURED[name]
    off, on = q["A", False], q["A", True]
    if m_on - m_off >= 0.3:
        assert on - off >= 0.5 * (m_on - m_off)
    else:
        assert on >= off - 0.3
