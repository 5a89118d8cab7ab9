"""Temporal reprojection (include/rt_api.h "temporal reprojection", csrc/rt_reproject.hip), the part that needs no device: a numpy restatement of
rules 15-19 in whole-plane float32 operations, written independently of rt_host.cpp's loops; rt_reproject_planes against it bit for bit on moved
cameras, a moved sphere, a camera turned round, non-finite records and planted texels; the identity, the disocclusion and the quality the header
quotes, with frames of the oracle alone; the frame record's new field; the refusals.  tests/test_gpu_reproject.py compares the device with
rt_reproject_planes and imports the cases of this file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import _build, api, host
from test_features_cpu import F, MISS, _dot, rays_restated, records, sphere
from test_features_cpu import scene as feature_scene

RT_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _image(plane, w, h):
    """A plane in the colour plane's row order -> IMAGE rows (row y = image row y), [h, w, channels]."""
    return np.asarray(plane, F).reshape(h, w, -1)[::-1]


def reproject_restated(dst, src, w, h, k_pos=4.0, max_history=64.0):
    """Rules 15-19 for every pixel at once: float32 [h, w, 4] in the colour plane's row order.  `dst` and `src` as api.reproject_planes takes them."""
    k_pos, max_history = F(k_pos), F(max_history)
    sphD, sphS = api.as_spheres(dst["spheres"]), api.as_spheres(src["spheres"])
    count = len(sphD)
    camS = np.asarray(src["cam"], F).reshape(5, 3)
    origS, dirS, cxS, cyS = camS[0], camS[2], camS[3], camS[4]
    FD, FS = _image(dst["feat"], w, h), _image(src["feat"], w, h)
    U = _image(src["plane"], w, h)
    nd = F(dst["passes"])
    with np.errstate(all="ignore"):
        # 15. the point and where it was
        idD, tD = FD[..., 7].view(np.uint32), FD[..., 6]
        known = idD < np.uint32(count) if count else np.zeros((h, w), bool)
        safe = np.where(known, idD, 0).astype(np.int64)
        oD, dD = rays_restated(dst["cam"], w, h)
        P = oD + dD * tD[..., None]
        if count:
            m = sphD["p"][safe].astype(F) - sphS["p"][safe].astype(F)
        else:
            m = np.zeros((h, w, 3), F)
        Pp = P - m
        # 16. where S saw it
        v = Pp - origS[None, None, :]
        z = _dot(v, dirS)
        kx = (_dot(v, cxS) * _dot(dirS, dirS)) / (z * _dot(cxS, cxS))
        ky = (_dot(v, cyS) * _dot(dirS, dirS)) / (z * _dot(cyS, cyS))
        fx, fy = (kx + F(0.5)) * F(w), (ky + F(0.5)) * F(h)
        seen = known & (z > F(0.0)) & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix0, iy0 = np.where(seen, x0, F(0.0)).astype(np.int64), np.where(seen, y0, F(0.0)).astype(np.int64)
        # 17. the taps, 18. the history
        oS, dS = rays_restated(src["cam"], w, h)
        foot = np.sqrt(_dot(cxS, cxS)) * (F(1.0) / F(w))
        sw, sn, sc = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
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
                sw = np.where(take, sw + b, sw)
                sn = np.where(take, sn + b * un, sn)
                sc = np.where(take[..., None], sc + b[..., None] * Uq[..., 0:3], sc)
        have = sw > F(0.0)
        H, nh = sc / sw[..., None], sn / sw
        nh = np.where(nh > max_history, max_history, nh)
        # 19. the blend
        T = np.zeros((h, w, 4), F)
        if dst["passes"] == 0:
            T[..., 0:3] = np.where(have[..., None], H, F(0.0))
            T[..., 3] = np.where(have, nh, nd)
        else:
            CD = _image(dst["plane"], w, h)[..., 0:3]
            inv = F(1.0) / (nd + nh)
            T[..., 0:3] = np.where(have[..., None], (CD * nd + H * nh[..., None]) * inv[..., None], CD)
            T[..., 3] = np.where(have, nd + nh, nd)
    assert T.dtype == F and sw.dtype == F and fx.dtype == F
    return T[::-1].copy()


# ---- the cases, shared with the device tests ------------------------------------------------------------------------------
def sideways(orig, target, share):
    """`orig` moved sideways (along dir x up) by `share` of its distance to `target`."""
    o, t = np.asarray(orig, np.float64), np.asarray(target, np.float64)
    d = t - o
    side = np.cross(d, (0.0, 1.0, 0.0))
    return tuple(float(v) for v in o + side / np.linalg.norm(side) * np.linalg.norm(d) * share)


def geometry(name):
    """(records of D, records of S, camera of D, camera of S, w, h) of a named case: S is the old view, D the new one."""
    demo = host.demo_scene()
    o, t = host.DEMO_ORIG, host.DEMO_TARGET
    if name.startswith("demo_"):
        size, kind = name[5:].split("_")
        w, h = (int(v) for v in size.split("x"))
        camS = host.compute_camera(o, t, w, h)
        moved = demo.copy()
        if kind == "same":
            camD = camS.copy()
        elif kind == "translated":
            camD = host.compute_camera(sideways(o, t, 0.02), t, w, h)
        elif kind == "rotated":                              # the target far to the right: a band of D's frame lies outside S's
            camD = host.compute_camera(o, (t[0] + 70.0, t[1], t[2]), w, h)
        elif kind == "turned":                               # looking the other way: everything D sees lies behind S's camera
            camD = host.compute_camera(o, (2 * o[0] - t[0], 2 * o[1] - t[1] - 150.0, 2 * o[2] - t[2]), w, h)
        elif kind == "sphere":                               # record 3, the blue sphere in the middle, moved; the camera stays
            camD = camS.copy()
            moved["p"][3] += np.array((7.0, 1.5, -2.0), F)
        else:
            raise KeyError(name)
        return moved, demo, camD, camS, w, h
    if name == "nonfinite":
        sph, camS, w, h = feature_scene("nonfinite")
        camD = host.compute_camera(sideways((0.0, 0.0, 50.0), (0.0, 0.0, 0.0), 0.03), (0.0, 0.0, 0.0), w, h)
        return sph, sph, camD, camS, w, h
    if name == "disocclusion":                               # a small sphere in front of a wall sphere, moved sideways by more than its width
        w, h = 64, 48
        cam = host.compute_camera((0.0, 0.0, 60.0), (0.0, 0.0, 0.0), w, h)
        old = records([sphere(500.0, (0, 0, -520), c=(0.6, 0.6, 0.6)), sphere(4.0, (-6, 0, 0), c=(0.9, 0.2, 0.2))])
        new = old.copy()
        new["p"][1] += np.array((12.0, 0.0, 0.0), F)
        return new, old, cam, cam, w, h
    raise KeyError(name)


GEOMETRIES = ["demo_41x23_translated", "demo_70x19_translated", "demo_1x1_translated", "demo_41x23_rotated", "demo_41x23_turned", "demo_41x23_sphere",
              "nonfinite"]
# (geometry, channels of the source plane, passes of the destination)
CASES = [(g, ch, nd) for g in GEOMETRIES for ch, nd in ((3, 2), (4, 2), (4, 0))] + [("demo_41x23_translated", 3, 0)]
CASE_IDS = ["%s-%dch-nd%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def synthetic(w, h, channels, planted=True):
    """A source plane [h, w, channels] of random colours in [0, 2) and sample counts in [1, 100), one texel with a NaN colour word and (4 channels)
    one with n == 0 planted (`planted`) where the frame is large enough; read-only."""
    rng = np.random.default_rng(1000 * channels + 31 * w + h)
    U = rng.uniform(0.0, 2.0, (h, w, channels)).astype(F)
    if channels == 4:
        U[..., 3] = rng.uniform(1.0, 100.0, (h, w)).astype(F)
    if planted and w > 8 and h > 8:
        U[h - 4, w // 2, 1] = np.nan                         # (the ground fills the bottom rows of the Demo frame)
        if channels == 4:
            U[h - 3, w // 3, 3] = 0.0
    U.setflags(write=False)
    return U


def sides(name, channels, passes_d, src_passes=16):
    """The two dicts api.reproject_planes takes, with synthetic planes."""
    sphD, sphS, camD, camS, w, h = geometry(name)
    dst = {"plane": synthetic(w, h, 3, False)[::-1, ::-1] if passes_d else None, "passes": passes_d, "feat": api.features_planes(sphD, camD, w, h), "cam": camD,
           "spheres": sphD}
    src = {"plane": synthetic(w, h, channels), "passes": src_passes, "feat": api.features_planes(sphS, camS, w, h), "cam": camS, "spheres": sphS}
    return dst, src, w, h


def assert_same_temporal(got, want):
    """Bit for bit, NaNs by position (a NaN's payload is not part of the rules)."""
    got, want = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def history(T, passes_d):
    """Which pixels of a temporal plane took history (rule 19: their n is not nd), [h, w] in the plane's row order."""
    return T[..., 3] != F(passes_d)


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    lib = api.load_library()
    for name in ("rt_reproject_defaults", "rt_reproject_async", "rt_read_temporal", "rt_reproject_planes"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    for name in ("reproject_async", "read_temporal", "reproject_defaults"):
        assert callable(getattr(api.RtContext, name))
    assert callable(api.reproject_planes)
    d = api.reproject_defaults()
    assert C.sizeof(d) == 16 and d.as_dict() == {"k_pos": 4.0, "max_history": 64.0, "reserved": [0, 0]}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reproject_planes_equals_the_restatement_bit_for_bit(case):
    name, channels, passes_d = case
    dst, src, w, h = sides(name, channels, passes_d)
    for params in ({}, {"k_pos": 1.5, "max_history": 10.0}):
        got = api.reproject_planes(dst, src, w, h, params or None)
        want = reproject_restated(dst, src, w, h, **params)
        assert got.shape == (h, w, 4)
        assert_same_temporal(got, want)
    T = api.reproject_planes(dst, src, w, h)
    took = history(T, passes_d)
    hit = dst["feat"].reshape(h, w, 8)[..., 7].view(np.uint32) != MISS
    assert not took[~hit].any()                              # the sky has no history
    if not passes_d:
        assert not T[~took].view(np.uint32).any()            # rule 19: four +0.0f
    if "translated" in name and w > 1:
        assert took.mean() > 0.5
    if name.endswith("rotated"):
        cols = took.any(axis=0)
        assert cols.any() and not cols.all()                 # a band of columns fell outside S
    if name.endswith("turned"):
        assert hit.any() and not took.any()                  # every z <= 0
    if name.endswith("sphere"):
        ids = dst["feat"].reshape(h, w, 8)[..., 7].view(np.uint32)
        assert (took & (ids == 3)).any()                     # the moved sphere carries its own history
    if channels == 4 and "translated" in name and w > 8:
        assert (T[..., 3][took] <= F(passes_d) + F(64.0)).all() and (T[..., 3][took] == F(passes_d) + F(64.0)).any()      # max_history caps, and does cap somewhere


def test_a_planted_nan_and_an_empty_texel_are_left_out():
    """The same source with and without the two planted texels: pixels whose taps touch neither are the same bits; the NaN spreads nowhere."""
    name = "demo_41x23_translated"
    dst, src, w, h = sides(name, 4, 2)
    clean = dict(src, plane=np.where(np.isnan(src["plane"]), F(0.5), src["plane"]))
    clean["plane"][h - 3, w // 3, 3] = F(7.0)
    with_, without = api.reproject_planes(dst, src, w, h), api.reproject_planes(dst, clean, w, h)
    assert np.isfinite(with_).all() and np.isfinite(without).all()
    differ = (with_.view(np.uint32) != without.view(np.uint32)).any(axis=-1)
    assert 1 <= differ.sum() <= 8                            # each texel is a tap of at most four pixels


def test_the_same_view_gives_the_source_back():
    """Same camera, same records, D at pass 0: every pixel with a hit has history, and T is U within the rounding of the reprojected position."""
    for channels in (3, 4):
        dst, src, w, h = sides("demo_41x23_same", channels, 0, src_passes=16)
        U = np.where(np.isnan(src["plane"]), F(0.25), src["plane"])     # (finite, so that every tap counts)
        if channels == 4:
            U[h - 3, w // 3, 3] = F(9.0)
        src = dict(src, plane=U)
        T = api.reproject_planes(dst, src, w, h)
        hit = dst["feat"].reshape(h, w, 8)[..., 7].view(np.uint32) != MISS
        assert hit.any() and np.array_equal(history(T, 0), hit)
        bound = 64 * 2.0 ** -23 * w
        assert (np.abs(T[..., 0:3] - U[..., 0:3])[hit] <= bound * np.abs(U[..., 0:3]).max()).all()
        n = np.minimum(U[..., 3], F(64.0)) if channels == 4 else np.full((h, w), F(16.0), F)
        slack = bound * (np.abs(U[..., 3]).max() if channels == 4 else 16.0)
        assert (np.abs(T[..., 3] - n)[hit] <= slack).all()


def test_a_moved_sphere_uncovers_pixels_without_history_and_carries_its_own():
    dst, src, w, h = sides("disocclusion", 3, 2)
    T = api.reproject_planes(dst, src, w, h)
    idD = dst["feat"].reshape(h, w, 8)[..., 7].view(np.uint32)
    idS = src["feat"].reshape(h, w, 8)[..., 7].view(np.uint32)
    inner = np.zeros((h, w), bool)                           # pixels whose 3x3 neighbourhood of S shows the small sphere only: no tap can reach the wall
    inner[1:-1, 1:-1] = np.all([np.roll(np.roll(idS == 1, dy, 0), dx, 1)[1:-1, 1:-1] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    uncovered = inner & (idD == 0)
    covered = idD == 1
    assert uncovered.sum() >= 20 and covered.sum() >= 20 and not (covered & (idS == 1)).any()       # moved by more than its width
    assert (T[..., 3][uncovered] == F(2.0)).all()
    assert np.array_equal(T[..., 0:3][uncovered].view(np.uint32), np.asarray(dst["plane"], F)[uncovered].view(np.uint32))
    assert (T[..., 3][covered] > F(2.0)).mean() > 0.8        # (its silhouette pixels may fail the footprint test)


# ---- what it is for ---------------------------------------------------------------------------------------------------
# what rt_reproject_planes measured in this set-up (include/rt_api.h quotes it): PSNR in dB of D alone and of T, and the share of hit pixels
# without history
MEASURED = {"cornell": (11.60, 20.77, 0.0209), "demo": (13.19, 24.51, 0.0094)}


def psnr8(img, ref):
    """PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5 (the pack of tests/test_guided_cpu.py's table)."""
    pack = lambda c: (np.clip(np.asarray(c, np.float64), 0.0, 1.0) ** (1 / 2.2) * 255 + .5).astype(np.int64)      # noqa: E731
    d = pack(img) - pack(ref)
    return 10 * np.log10(255.0 ** 2 / np.mean(d.astype(np.float64) ** 2))


def quality_setup(name, w=96, h=96):
    """(records, old origin, new origin, target): the new origin moved sideways by 2 % of its distance to the target."""
    if name == "demo":
        sph, o, t = host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET
    else:
        z = np.load(os.path.join(GOLDEN, name + "_96x96_4spp.npz"))
        sph, c = z["spheres"].view(api.SPHERE_DT).copy(), z["camera"].astype(F)
        o, t = tuple(float(v) for v in c[0:3]), tuple(float(v) for v in c[3:6])
    return sph, o, sideways(o, t, 0.02), t


@functools.lru_cache(maxsize=None)
def quality(name, w=96, h=96, n_src=16, n_dst=2, truth=1024, restated=False):
    """(PSNR of D alone, PSNR of T, share of hit pixels without history): S at n_src passes of seed stream 1 from the old origin, D at n_dst passes of
    stream 2 from the new one, against `truth` oracle passes of the new one."""
    sph, o_old, o_new, t = quality_setup(name, w, h)
    camS, camD = host.compute_camera(o_old, t, w, h), host.compute_camera(o_new, t, w, h)
    S = O.render(sph, camS, w, h, n_src, seeds_in=api.stream_seeds(1, 2 * w * h), threads=16)["colors"]
    D = O.render(sph, camD, w, h, n_dst, seeds_in=api.stream_seeds(2, 2 * w * h), threads=16)["colors"]
    ref = O.render(sph, camD, w, h, truth, threads=16)["colors"]
    dst = {"plane": D, "passes": n_dst, "feat": api.features_planes(sph, camD, w, h), "cam": camD, "spheres": sph}
    src = {"plane": S, "passes": n_src, "feat": api.features_planes(sph, camS, w, h), "cam": camS, "spheres": sph}
    T = reproject_restated(dst, src, w, h) if restated else api.reproject_planes(dst, src, w, h)
    hit = dst["feat"].reshape(h, w, 8)[..., 7].view(np.uint32) != MISS
    return psnr8(D, ref), psnr8(T[..., 0:3].reshape(-1), ref), float((~history(T, n_dst) & hit).sum() / hit.sum())


@pytest.mark.parametrize("name", ["cornell", "demo"])
def test_reprojection_is_closer_to_the_truth_than_the_new_view_alone(name, capsys):
    alone, temporal, lost = quality(name)
    with capsys.disabled():
        print("\n[reproject] %s 96x96, S 16 passes, D 2 passes: D alone %.2f dB, T %.2f dB (gain %.2f dB), %.2f %% of hit pixels without history"
              % (name, alone, temporal, temporal - alone, 100 * lost))
    m_alone, m_temporal, m_lost = MEASURED[name]
    assert m_temporal - m_alone >= 1.0                       # (below that, something differs from the prototype)
    assert temporal - alone >= 0.5 * (m_temporal - m_alone)
    if name == "cornell":
        assert lost < 2 * m_lost


# ---- the frame record ----------------------------------------------------------------------------------------------------
PROGRAM = r'''
#include <cstdio>
#include "rt_frame_state.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

template <class Event> static void ends(const char *what, Event event) {
    rt::FrameState f;
    f.launched(2, true);
    f.reprojected();
    EXPECT(f.temporal_current);
    event(f);
    if (f.temporal_current) { std::printf("%s leaves the temporal plane current\n", what); ++failures; }
}

template <class Event> static void keeps(const char *what, Event event) {
    rt::FrameState f;
    f.launched(2, true);
    f.reprojected();
    event(f);
    if (!f.temporal_current) { std::printf("%s ends the temporal plane\n", what); ++failures; }
}

int main() {
    rt::FrameState f;
    EXPECT(!f.temporal_current);
    f.reprojected();                                        // (a pure warp: the destination holds no pass)
    EXPECT(f.temporal_current && f.current_sample == 0 && f.launches == 0 && f.pixels_current && !f.ragged && f.filtered_pair == 0);
    rt::FrameState g;
    g.launched(3, false);
    g.pair_filtered(7);
    const rt::FrameState before = g;
    g.reprojected();                                        // nothing else of the frame changes
    EXPECT(g.temporal_current && g.current_sample == before.current_sample && g.launches == before.launches && g.pixels_current == before.pixels_current
           && g.filtered_pair == 7 && g.seeds_default == before.seeds_default && g.seeds_custom == before.seeds_custom && g.have_selection == before.have_selection);

    ends("a launch", [](rt::FrameState &s) { s.launched(1, true); });
    ends("a subset launch", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(2, 6); s.launched_subset(1, true, false); });
    ends("a subset launch of every group", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(6, 18); s.launched_subset(1, true, true); });
    ends("a reset", [](rt::FrameState &s) { s.reset_blocking(); });
    ends("an in-place reset", [](rt::FrameState &s) { s.reset_in_place(); });
    ends("a seed stream", [](rt::FrameState &s) { s.reset_in_place(); s.custom_seeds_written(); });
    ends("a written state", [](rt::FrameState &s) { s.state_written(5, true); });
    ends("a written state without seeds", [](rt::FrameState &s) { s.state_written(5, false); });
    ends("a merge", [](rt::FrameState &s) { s.merged(9); });
    ends("a merge by tile", [](rt::FrameState &s) { s.merged_by_tile(9); });
    ends("a filter into the context", [](rt::FrameState &s) { s.colours_replaced(); });
    ends("a feature plane formed again", [](rt::FrameState &s) { s.features_reformed(); });

    keeps("packing the frame", [](rt::FrameState &s) { s.pixels_packed(); });
    keeps("a selection", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(2, 6); });
    keeps("cross-filtering the halves", [](rt::FrameState &s) { s.pair_filtered(3); });
    keeps("a timed launch's figure", [](rt::FrameState &s) { s.timed(1.0); });
    keeps("reprojecting again", [](rt::FrameState &s) { s.reprojected(); });
    std::printf("%d failures\n", failures);
    return failures != 0;
}
'''


def test_the_frame_record_knows_when_the_temporal_plane_is_current(tmp_path):
    """reprojected() sets the field and nothing else; a launch, a subset launch, both resets, a seed stream, a written state, both merges and a
    replaced colour plane clear it -- the events that clear filtered_pair -- and so does a feature plane formed anew."""
    src = tmp_path / "reproject_record.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "reproject_record"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    dst, src, w, h = sides("demo_41x23_translated", 3, 2)
    good = api.reproject_planes(dst, src, w, h)
    nan, inf = float("nan"), float("inf")
    for name in ("k_pos", "max_history"):
        for bad in (0.0, -1.0, nan, inf, -inf):
            with pytest.raises(api.RtError) as err:
                api.reproject_planes(dst, src, w, h, {name: bad})
            assert err.value.code == RT_ERR_ARG and name in str(err.value)
    for word in (0, 1):
        p = api.reproject_defaults()
        p.reserved[word] = 1
        with pytest.raises(api.RtError) as err:
            api.reproject_planes(dst, src, w, h, p)
        assert err.value.code == RT_ERR_ARG and "reserved" in str(err.value)
    with pytest.raises(ValueError):
        api.reproject_planes(dst, src, w, h, {"k_colour": 1.0})

    def view(side, **over):
        keep = [np.ascontiguousarray(side["plane"], F), np.ascontiguousarray(side["feat"], F), api.as_camera(side["cam"]), api.as_spheres(side["spheres"])]
        fields = {"plane": keep[0].ctypes.data, "channels": 3, "passes": side["passes"], "feat": keep[1].ctypes.data, "cam": keep[2].ctypes.data,
                  "spheres": keep[3].ctypes.data}
        fields.update(over)
        v = api.ReprojectView(*(fields[k] for k in ("plane", "channels", "passes", "feat", "cam", "spheres")))
        v._keep = keep
        return v

    out = np.zeros((h, w, 4), F)
    p_out, count = api._ptr(out), len(dst["spheres"])
    call = lambda o, d, s, n=count, ww=w, hh=h: lib.rt_reproject_planes(o, C.byref(d) if d is not None else None, C.byref(s) if s is not None else None, n, ww, hh, None)      # noqa: E731
    assert call(p_out, view(dst), view(src)) == 0 and np.array_equal(out.view(np.uint32), good.view(np.uint32))
    out[...] = 0
    refused = [(None, view(dst), view(src)), (p_out, None, view(src)), (p_out, view(dst), None),
               (p_out, view(dst), view(src, plane=None)), (p_out, view(dst, plane=None), view(src)),          # (dst holds two passes)
               (p_out, view(dst, feat=None), view(src)), (p_out, view(dst), view(src, feat=None)),
               (p_out, view(dst, cam=None), view(src)), (p_out, view(dst), view(src, cam=None)),
               (p_out, view(dst, spheres=None), view(src)), (p_out, view(dst), view(src, spheres=None)),
               (p_out, view(dst, channels=2), view(src)), (p_out, view(dst), view(src, channels=5)), (p_out, view(dst), view(src, channels=0)),
               (p_out, view(dst, passes=-1), view(src)), (p_out, view(dst), view(src, passes=-1))]
    for args in refused:
        assert call(*args) == RT_ERR_ARG and lib.rt_last_error() != b""
    for ww, hh in ((0, h), (w, 0), (-3, h)):
        assert call(p_out, view(dst), view(src), count, ww, hh) == RT_ERR_ARG
    assert not out.any()
    assert call(p_out, view(dst, plane=None, passes=0), view(src)) == 0      # a null colour plane at pass 0 is the pure warp
    assert lib.rt_reproject_async(None, None, None, None) == RT_ERR_ARG and lib.rt_read_temporal(None, p_out, None) == RT_ERR_ARG
    lib.rt_reproject_defaults(None)                          # a null pointer is ignored
