"""The edge-avoiding wavelet filter (include/rt_api.h "edge-avoiding wavelet filter", csrc/rt_atrous.hip), the part that needs no device: a numpy
restatement of rules 20-23 in whole-plane float32 operations, written independently of rt_host.cpp's loops; rt_atrous_planes against it bit for bit on
the geometries of tests/test_reproject_cpu.py with planted texels; the properties the rules promise; the quality the header quotes, with frames of the
oracle alone; the frame record's new field; the refusals.  tests/test_gpu_atrous.py compares the device with rt_atrous_planes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import _build, api, host
from test_reproject_cpu import F, GEOMETRIES, geometry, psnr8, quality_setup, synthetic

RT_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HK = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
PARAMS = [{}, {"levels": 5, "k_lum": 0.7, "k_normal": 0.1}]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _taps(w, h, dx, dy):
    """For every pixel p the array neighbour q = p + (dx, dy): (inside the image, its row, its column) -- row and column clipped where outside."""
    ys, xs = np.mgrid[0:h, 0:w]
    qx, qy = xs + dx, ys + dy
    return (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h), np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)


def atrous_restated(plane, feat, w, h, passes=0, levels=3, k_lum=1.5, k_normal=0.3):
    """Rules 20-23 for every pixel at once: float32 [h, w, 4] (rgb, variance).  `plane` and `feat` as api.atrous_planes takes them."""
    U = np.asarray(plane, F).reshape(h, w, -1)
    feat = np.asarray(feat, F).reshape(h, w, 8)
    ids, N = feat[..., 7].view(np.uint32), feat[..., 3:6]
    n = U[..., 3] if U.shape[-1] == 4 else np.full((h, w), F(passes), F)
    k_lum, k_normal = F(k_lum), F(k_normal)
    with np.errstate(all="ignore"):
        Cc = U[..., 0:3].copy()
        usable = np.isfinite(Cc).all(axis=-1) & (n > F(0.0))                 # 20
        s0, s1, s2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        l0 = lum(Cc)
        for dy in (-1, 0, 1):                                                # 21
            for dx in (-1, 0, 1):
                inside, ry, rx = _taps(w, h, dx, dy)
                take = inside & usable[ry, rx] & (ids[ry, rx] == ids)
                lq = l0[ry, rx]
                s0 = np.where(take, s0 + F(1.0), s0)
                s1 = np.where(take, s1 + lq, s1)
                s2 = np.where(take, s2 + lq * lq, s2)
        m = s1 / s0
        v = s2 / s0 - m * m
        V = np.where((s0 > F(0.0)) & (v > F(0.0)), v, F(0.0)).astype(F)
        inv, kl2 = F(1.0) / (k_normal * k_normal), k_lum * k_lum
        for level in range(levels):                                          # 22, 23
            s = 1 << level
            lp = lum(Cc)
            acc, aw, av = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    inside, ry, rx = _taps(w, h, s * i, s * j)
                    Cq, Vq, nq = Cc[ry, rx], V[ry, rx], n[ry, rx]
                    if i == 0 and j == 0:
                        take = np.ones((h, w), bool)
                        wgt = (F(0.375) * F(0.375)) * n
                    else:
                        take = inside & usable[ry, rx] & (ids[ry, rx] == ids)
                        a = N - N[ry, rx]
                        gn = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) * inv
                        d = lp - lum(Cq)
                        gl = (d * d) / (kl2 * (V + Vq) + F(1e-10))
                        g = np.zeros((h, w), F)
                        g = np.where(gn > g, gn, g)
                        g = np.where(gl > g, gl, g)
                        wgt = ((HK[j + 2] * HK[i + 2]) * (F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5))))) * nq
                    assert wgt.dtype == F
                    acc = np.where(take[..., None], acc + wgt[..., None] * Cq, acc)
                    aw = np.where(take, aw + wgt, aw)
                    av = np.where(take, av + (wgt * wgt) * Vq, av)
            Cn, Vn = acc / aw[..., None], av / (aw * aw)
            Cc = np.where(usable[..., None], Cn, Cc).astype(F)
            V = np.where(usable, Vn, V).astype(F)
    out = np.concatenate([Cc, V[..., None]], axis=-1)
    assert out.dtype == F
    return out


def assert_same_plane(got, want):
    """Bit for bit, NaNs by position (a NaN's payload is not part of the rules)."""
    got, want = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


@functools.lru_cache(maxsize=None)
def features_of(name):
    """(feature plane of the new view of a geometry of tests/test_reproject_cpu.py, w, h); read-only."""
    sphD, _, camD, _, w, h = geometry(name)
    feat = api.features_planes(sphD, camD, w, h)
    feat.setflags(write=False)
    return feat, w, h


def flat_features(ids, normal=(0.0, 0.0, 1.0)):
    """A feature plane that holds nothing but the scene indices `ids` [h, w] and one normal."""
    h, w = ids.shape
    feat = np.zeros((h, w, 8), F)
    feat[..., 3:6] = np.asarray(normal, F)
    feat[..., 7] = np.asarray(ids, np.uint32).view(F)
    return feat


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    lib = api.load_library()
    for name in ("rt_atrous_defaults", "rt_atrous_async", "rt_read_atrous", "rt_atrous_planes"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    for name in ("atrous_async", "read_atrous", "atrous_defaults"):
        assert callable(getattr(api.RtContext, name))
    assert callable(api.atrous_planes)
    d = api.atrous_defaults()
    assert C.sizeof(d) == 16 and C.sizeof(api.AtrousParams) == 16
    assert d.levels == 3 and d.k_lum == F(1.5) and d.k_normal == F(0.3) and d.reserved == 0
    assert d.as_dict() == {"levels": 3, "k_lum": 1.5, "k_normal": float(F(0.3)), "reserved": 0}


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_atrous_planes_equals_the_restatement_bit_for_bit(name, channels):
    """Levels 5 at 41x23 puts steps 8 and 16 beyond the image in one direction or both; 1x1 has no neighbour at all."""
    feat, w, h = features_of(name)
    plane = synthetic(w, h, channels)
    for params in PARAMS:
        got = api.atrous_planes(plane, feat, w, h, 16, params or None)
        want = atrous_restated(plane, feat, w, h, 16, **params)
        assert got.shape == (h, w, 4)
        assert_same_plane(got, want)
    if w > 8:
        assert np.isnan(plane).any() and np.isnan(got).sum() == 1            # the planted NaN word, and nothing else


def test_no_level_gives_the_input_and_the_variance_estimate():
    feat, w, h = features_of("demo_41x23_translated")
    for channels in (3, 4):
        plane = synthetic(w, h, channels)
        got = api.atrous_planes(plane, feat, w, h, 16, {"levels": 0})
        assert_same_plane(got[..., 0:3], plane[..., 0:3])
        assert_same_plane(got, atrous_restated(plane, feat, w, h, 16, levels=0))
        assert (got[..., 3] >= 0).all() and (got[..., 3] > 0).mean() > 0.5


def test_two_surfaces_of_one_colour_each_keep_their_colours():
    """Two ids, a constant colour each, random sample counts: a weighted mean of equal words is that word within the rounding of 25 products and sums,
    and nothing of the other side's colour arrives."""
    w, h = 24, 16
    ids = np.zeros((h, w), np.uint32)
    ids[:, w // 2:] = 0xFFFFFFFF                                             # (the sky's id is an id like any other)
    colours = np.array([(0.2, 0.7, 0.4), (0.9, 0.1, 0.6)], F)
    plane = np.zeros((h, w, 4), F)
    plane[..., 0:3] = colours[(ids != 0).astype(int)]
    plane[..., 3] = np.random.default_rng(5).uniform(1.0, 64.0, (h, w)).astype(F)
    out = api.atrous_planes(plane, flat_features(ids), w, h)
    for side, c in enumerate(colours):
        got = out[..., 0:3][(ids != 0) == bool(side)]
        assert (np.abs(got - c) <= 4 * np.spacing(c)).all()
    lo, hi = np.minimum(*colours), np.maximum(*colours)
    assert not ((out[..., 0:3] > lo + 4 * np.spacing(lo)) & (out[..., 0:3] < hi - 4 * np.spacing(hi))).any()       # never between the two
    # a constant surface has no variance but the rounding of nine squares of a luminance below 1: 9 * 2^-24 and a margin
    assert (out[..., 3] <= 1e-6).all()


def test_without_edge_stopping_it_is_the_b3_spline_blur_weighted_by_sample_counts():
    """One id, one normal, k_lum 1e18: gn == 0 and gl ~ 1e-36, every weight is hk[j] * hk[i] * n_q over the taps inside the image."""
    w, h = 29, 21
    rng = np.random.default_rng(11)
    plane = np.concatenate([rng.uniform(0.5, 2.0, (h, w, 3)), rng.uniform(1.0, 100.0, (h, w, 1))], axis=-1).astype(F)
    out = api.atrous_planes(plane, flat_features(np.full((h, w), 3, np.uint32)), w, h, 0, {"levels": 3, "k_lum": 1e18})
    want, n = plane[..., 0:3].astype(np.float64), plane[..., 3].astype(np.float64)
    hk = np.array(HK, np.float64)
    for level in range(3):
        acc, aw = np.zeros((h, w, 3)), np.zeros((h, w))
        for j in range(-2, 3):
            for i in range(-2, 3):
                inside, ry, rx = _taps(w, h, i * (1 << level), j * (1 << level))
                wgt = np.where(inside, hk[j + 2] * hk[i + 2] * n[ry, rx], 0.0)
                acc += wgt[..., None] * want[ry, rx]
                aw += wgt
        want = acc / aw[..., None]
    assert (np.abs(out[..., 0:3] - want) <= 1e-5 * np.abs(want)).all()


@pytest.mark.parametrize("levels", [1, 2])
def test_a_planted_nan_and_an_empty_texel_stay_and_spread_nowhere(levels):
    """The same plane with and without the two planted texels: they come back unchanged, everything else is finite, and the outputs differ only within
    the taps' reach -- 1 for the variance estimate, then 2 * 2^i per level."""
    feat, w, h = features_of("demo_41x23_translated")
    plane = synthetic(w, h, 4)
    bad = [(h - 4, w // 2), (h - 3, w // 3)]
    assert np.isnan(plane[bad[0]][1]) and plane[bad[1]][3] == 0.0
    clean = np.where(np.isnan(plane), F(0.5), plane)
    clean[bad[1]][3] = F(7.0)
    with_, without = api.atrous_planes(plane, feat, w, h, 0, {"levels": levels}), api.atrous_planes(clean, feat, w, h, 0, {"levels": levels})
    for at in bad:
        assert_same_plane(with_[at][0:3], plane[at][0:3])
        assert_same_plane(with_[at], api.atrous_planes(plane, feat, w, h, 0, {"levels": 0})[at])      # ... and its V0 word
    rest = np.ones((h, w), bool)
    for at in bad:
        rest[at] = False
    assert np.isfinite(with_[rest]).all() and np.isfinite(without).all()
    differ = (with_.view(np.uint32) != without.view(np.uint32)).any(axis=-1)
    reach = 1 + 2 * ((1 << levels) - 1)
    ys, xs = np.mgrid[0:h, 0:w]
    near = np.zeros((h, w), bool)
    for (y, x) in bad:
        near |= (np.abs(ys - y) <= reach) & (np.abs(xs - x) <= reach)
    assert differ[bad[0]] and differ[bad[1]] and differ.sum() > 2 and not differ[~near].any()


def test_a_pixel_alone_with_its_id_has_no_variance():
    w, h = 9, 7
    ids = np.zeros((h, w), np.uint32)
    ids[3, 4] = 5
    ids[0, 0] = 6                                                            # a corner: five of its nine neighbours lie outside
    plane = synthetic(w, h, 3, False)
    out = api.atrous_planes(plane, flat_features(ids), w, h, 4, {"levels": 0})
    assert out[3, 4, 3] == 0.0 and out[0, 0, 3] == 0.0 and (out[..., 3] > 0).sum() == w * h - 2
    out = api.atrous_planes(plane, flat_features(ids), w, h, 4)             # ... and no tap but the centre
    assert (np.abs(out[3, 4, 0:3] - plane[3, 4]) <= 3 * np.spacing(plane[3, 4])).all() and out[3, 4, 3] == 0.0       # (a product and a quotient per level)


# ---- what it is for ---------------------------------------------------------------------------------------------------
# what the prototype measured in this set-up at 96x96 with the defaults (include/rt_api.h quotes it), dB: T, T filtered, D alone, D alone filtered
MEASURED = {"cornell": (20.77, 27.13, 11.60, 21.57), "demo": (24.51, 27.16, 13.19, 23.05), "simple": (28.14, 29.13, 16.54, 25.97)}


@functools.lru_cache(maxsize=None)
def quality(name, w=96, h=96, n_src=16, n_dst=2, truth=1024):
    """(T, T filtered, D alone, D alone filtered) in dB against `truth` oracle passes, in the set-up of test_reproject_cpu.quality."""
    sph, o_old, o_new, t = quality_setup(name, w, h)
    camS, camD = host.compute_camera(o_old, t, w, h), host.compute_camera(o_new, t, w, h)
    S = O.render(sph, camS, w, h, n_src, seeds_in=api.stream_seeds(1, 2 * w * h), threads=16)["colors"]
    D = O.render(sph, camD, w, h, n_dst, seeds_in=api.stream_seeds(2, 2 * w * h), threads=16)["colors"]
    ref = O.render(sph, camD, w, h, truth, threads=16)["colors"]
    featD = api.features_planes(sph, camD, w, h)
    dst = {"plane": D, "passes": n_dst, "feat": featD, "cam": camD, "spheres": sph}
    src = {"plane": S, "passes": n_src, "feat": api.features_planes(sph, camS, w, h), "cam": camS, "spheres": sph}
    T = api.reproject_planes(dst, src, w, h)
    rgb = lambda plane: plane[..., 0:3].reshape(-1)      # noqa: E731
    return (psnr8(rgb(T), ref), psnr8(rgb(api.atrous_planes(T, featD, w, h)), ref), psnr8(D, ref), psnr8(rgb(api.atrous_planes(D, featD, w, h, n_dst)), ref))


@pytest.mark.parametrize("name", ["cornell", "demo", "simple"])
def test_the_filtered_frame_is_closer_to_the_truth(name, capsys):
    t, t_f, d, d_f = quality(name)
    with capsys.disabled():
        print("\n[atrous] %s 96x96, S 16 passes, D 2 passes, 3 levels: T %.2f -> %.2f dB (gain %.2f), D alone %.2f -> %.2f dB (gain %.2f)"
              % (name, t, t_f, t_f - t, d, d_f, d_f - d))
    m_t, m_tf, m_d, m_df = MEASURED[name]
    assert d_f - d >= 0.5 * (m_df - m_d)                     # 9.97, 9.86, 9.43 dB in the prototype
    if name == "simple":
        assert t_f >= t                                      # (the prototype gains 1 dB there: only "not worse")
    else:
        assert t_f - t >= 0.5 * (m_tf - m_t)                 # 6.36 and 2.65 dB in the prototype


# ---- the frame record ----------------------------------------------------------------------------------------------------
PROGRAM = r'''
#include <cstdio>
#include "rt_frame_state.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static rt::FrameState formed() {
    rt::FrameState f;
    f.launched(2, true);
    f.reprojected();
    f.atrous_filtered();
    return f;
}

template <class Event> static void ends(const char *what, Event event) {
    rt::FrameState f = formed();
    EXPECT(f.atrous_current);
    event(f);
    if (f.atrous_current) { std::printf("%s leaves the filtered plane current\n", what); ++failures; }
}

template <class Event> static void keeps(const char *what, Event event) {
    rt::FrameState f = formed();
    event(f);
    if (!f.atrous_current) { std::printf("%s ends the filtered plane\n", what); ++failures; }
    if (!f.temporal_current) { std::printf("%s ends the temporal plane\n", what); ++failures; }
}

int main() {
    rt::FrameState f;
    EXPECT(!f.atrous_current);
    rt::FrameState g;
    g.launched(3, false);
    g.pair_filtered(7);
    g.reprojected();
    const rt::FrameState before = g;
    g.atrous_filtered();                                    // the field and nothing else
    EXPECT(g.atrous_current && g.temporal_current && g.current_sample == before.current_sample && g.launches == before.launches
           && g.pixels_current == before.pixels_current && g.filtered_pair == 7 && g.filtered_behind == before.filtered_behind
           && g.seeds_default == before.seeds_default && g.seeds_custom == before.seeds_custom && g.have_selection == before.have_selection
           && g.ragged == before.ragged && g.list_valid == before.list_valid && g.selection_serial == before.selection_serial && g.last_ms == before.last_ms);
    rt::FrameState c;
    c.launched(1, true);
    c.atrous_filtered();                                    // from the colour plane: no temporal plane appears
    EXPECT(c.atrous_current && !c.temporal_current);

    // every event that ends the temporal plane
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
    // ... and the two of its own
    ends("a feature plane formed again", [](rt::FrameState &s) { s.features_reformed(); });
    ends("a new reprojection", [](rt::FrameState &s) { s.reprojected(); });
    {
        rt::FrameState s = formed();
        s.reprojected();
        EXPECT(s.temporal_current && !s.atrous_current);
    }

    keeps("packing the frame", [](rt::FrameState &s) { s.pixels_packed(); });
    keeps("a selection", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(2, 6); });
    keeps("cross-filtering the halves", [](rt::FrameState &s) { s.pair_filtered(3); });
    keeps("cross-filtering the selected groups again", [](rt::FrameState &s) { s.pair_tiles_refreshed(4); });
    keeps("a timed launch's figure", [](rt::FrameState &s) { s.timed(1.0); });
    keeps("filtering again", [](rt::FrameState &s) { s.atrous_filtered(); });
    std::printf("%d failures\n", failures);
    return failures != 0;
}
'''


def test_the_frame_record_knows_when_the_filtered_plane_is_current(tmp_path):
    """atrous_filtered() sets the field and nothing else; every event that ends the temporal plane clears it, and so do reprojected() and
    features_reformed(); packing, selecting, pair-filtering and timing keep it."""
    src = tmp_path / "atrous_record.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "atrous_record"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    feat, w, h = features_of("demo_41x23_translated")
    plane = synthetic(w, h, 3)
    good = api.atrous_planes(plane, feat, w, h, 2)
    nan, inf = float("nan"), float("inf")
    for name in ("k_lum", "k_normal"):
        for bad in (0.0, -1.0, nan, inf, -inf):
            with pytest.raises(api.RtError) as err:
                api.atrous_planes(plane, feat, w, h, 2, {name: bad})
            assert err.value.code == RT_ERR_ARG and name in str(err.value)
    for bad in (-1, 6, 1 << 20):
        with pytest.raises(api.RtError) as err:
            api.atrous_planes(plane, feat, w, h, 2, {"levels": bad})
        assert err.value.code == RT_ERR_ARG and "levels" in str(err.value)
    for levels in range(6):
        api.atrous_planes(plane, feat, w, h, 2, {"levels": levels})
    p = api.atrous_defaults()
    p.reserved = 1
    with pytest.raises(api.RtError) as err:
        api.atrous_planes(plane, feat, w, h, 2, p)
    assert err.value.code == RT_ERR_ARG and "reserved" in str(err.value)
    with pytest.raises(ValueError):
        api.atrous_planes(plane, feat, w, h, 2, {"k_depth": 1.0})
    with pytest.raises(ValueError):
        api.atrous_planes(plane[:, :, 0:2], feat, w, h, 2)
    with pytest.raises(ValueError):
        api.atrous_planes(plane, feat[..., 0:7], w, h, 2)

    out = np.zeros((h, w, 4), F)
    u, f = np.ascontiguousarray(plane), np.ascontiguousarray(feat)
    p_out, p_u, p_f = api._ptr(out), api._ptr(u), api._ptr(f)
    call = lambda o=p_out, pl=p_u, ch=3, n=2, ft=p_f, ww=w, hh=h: lib.rt_atrous_planes(o, pl, ch, n, ft, ww, hh, None)      # noqa: E731
    assert call() == 0 and np.array_equal(out.view(np.uint32)[~np.isnan(good)], good.view(np.uint32)[~np.isnan(good)])
    out[...] = 0
    refused = [dict(o=None), dict(pl=None), dict(ft=None), dict(ch=2), dict(ch=5), dict(ch=0), dict(n=-1), dict(ww=0), dict(hh=0), dict(ww=-3)]
    for over in refused:
        assert call(**over) == RT_ERR_ARG and lib.rt_last_error() != b"", over
    assert not out.any()
    assert call(n=0) == 0                                    # no pass: no pixel is usable, and that is no error
    assert lib.rt_atrous_async(None, None, None) == RT_ERR_ARG and lib.rt_read_atrous(None, p_out, None) == RT_ERR_ARG
    lib.rt_atrous_defaults(None)                             # a null pointer is ignored
