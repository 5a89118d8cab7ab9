"""NL-means guided by feature planes (include/rt_api.h "feature planes", rules 13-14), the part that needs no device: a numpy restatement of the
two rules on top of tests/test_denoise_cpu.py's and tests/test_denoise_pair_cpu.py's whole-plane pieces; rt_denoise_guided_planes and
rt_denoise_pair_guided_planes against it bit for bit; the identities the header states; the parameter refusals; and what the guide is for -- the
PSNR it gains over the unguided filter, with frames of the oracle alone.  tests/test_gpu_guided.py compares the device with the two host
functions and imports the planes of this file."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host
from test_denoise_cpu import F, _shift, _sum_window, assert_same_bits, denoise_restated, planes, smoothed_variance
from test_denoise_pair_cpu import pair_restated

RT_ERR_ARG = -1
PARAMS = [{"search_radius": 5, "patch_radius": 1}, {"search_radius": 8, "patch_radius": 2}, {"search_radius": 1, "patch_radius": 0}]
SIZES = [(8, 8), (41, 23), (70, 19)]
GUIDE = {"k_albedo": 0.15, "k_normal": 0.2, "k_depth": 0.05}
WIDE = {"k_albedo": 1e18, "k_normal": 1e18, "k_depth": 1e18}
CASES = [(w, h, p, kind) for w, h in SIZES for p in PARAMS for kind in ("noisy", "nonfinite")]
CASE_IDS = ["%dx%d-R%d-P%d-%s" % (w, h, p["search_radius"], p["patch_radius"], kind) for w, h, p, kind in CASES]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def feature_weight(Fp, oy, ox, k_albedo, k_normal, k_depth):
    """Rule 13 for every pixel p and q = cl(p + o) (the value at a q outside the image is never used): float32 [h, w]."""
    ia, in_, id_ = F(1.0) / (F(k_albedo) * F(k_albedo)), F(1.0) / (F(k_normal) * F(k_normal)), F(1.0) / (F(k_depth) * F(k_depth))
    Fq = _shift(Fp, oy, ox)
    a, n = Fp[..., 0:3] - Fq[..., 0:3], Fp[..., 3:6] - Fq[..., 3:6]
    pa = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) * ia
    pn = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) * in_
    r = (Fp[..., 6] - Fq[..., 6]) / ((Fp[..., 6] + Fq[..., 6]) + F(1e-10))
    pd = (r * r) * id_
    phi = np.zeros(Fp.shape[:2], F)
    for term in (pa, pn, pd):
        phi = np.where(term > phi, term, phi)                # (a NaN term: the comparison is false)
    wf = F(1.0) / (F(1.0) + phi * (F(1.0) + phi * F(0.5)))
    assert wf.dtype == F
    return wf


def cross_guided(X, G, V, Fp, guide, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """Rules 3-6 (8) with rule 14: X's values, the weights from G and the variance plane V, never above rule 13's of the feature plane Fp.
    guide None: rules 3-6 alone."""
    h, w = X.shape[:2]
    R, P = search_radius, patch_radius
    alpha, kk, inv = F(alpha), F(k) * F(k), F(1.0) / F(3 * (2 * P + 1) * (2 * P + 1))
    ys, xs = np.arange(h), np.arange(w)
    num, den = np.zeros((h, w, 3), F), np.zeros((h, w), F)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            if oy == 0 and ox == 0:
                num, den = num + F(1.0) * X, den + F(1.0)
                continue
            Xq, Gq, Vq = _shift(X, oy, ox), _shift(G, oy, ox), _shift(V, oy, ox)
            t = G - Gq
            m = np.where(Vq < V, Vq, V)
            dc = (t * t - alpha * (V + m)) / (F(1e-10) + kk * (V + Vq))
            T = _sum_window((dc[..., 0] + dc[..., 1]) + dc[..., 2], P) * inv
            inside = ((ys + oy >= 0) & (ys + oy < h))[:, None] & ((xs + ox >= 0) & (xs + ox < w))[None, :]
            take = inside & ~np.isnan(T) & np.isfinite(Xq).all(axis=-1)
            g = np.where(T > 0, T, F(0.0))
            wgt = F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5)))
            if guide is not None:
                wf = feature_weight(Fp, oy, ox, **guide)
                wgt = np.where(wf < wgt, wf, wgt)            # rule 14
            num = np.where(take[..., None], num + wgt[..., None] * Xq, num)
            den = np.where(take, den + wgt, den)
    out = num / den[..., None]
    assert out.dtype == F
    return out


def guided_restated(D, A, B, Fp, w, h, guide, **params):
    D, A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (D, A, B))
    with np.errstate(all="ignore"):
        return cross_guided(D, D, smoothed_variance(A, B), np.asarray(Fp, F).reshape(h, w, 8), guide, **params).reshape(-1)


def pair_guided_restated(A, B, Fp, w, h, guide, **params):
    A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (A, B))
    if params.get("search_radius", 5) == 0:
        return A.reshape(-1).copy(), B.reshape(-1).copy()
    Fp = np.asarray(Fp, F).reshape(h, w, 8)
    with np.errstate(all="ignore"):
        Vs = smoothed_variance(A, B)
        Vh = Vs + Vs
        return cross_guided(A, B, Vh, Fp, guide, **params).reshape(-1), cross_guided(B, A, Vh, Fp, guide, **params).reshape(-1)


# ---- the planes, shared with the device tests ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def features(w, h, kind="blocks"):
    """A synthetic feature plane [h, w, 8], read-only.  blocks: objects of 6x5 pixels with an albedo, a depth and a normal that turns slowly inside
    them, one object in four sky (seven zeros, index 0xFFFFFFFF); nan: the same with a NaN planted in an albedo, a normal and a depth word;
    constant: one record everywhere."""
    rng = np.random.default_rng(77 * w + h)
    by, bx = (h + 4) // 5, (w + 5) // 6
    up = lambda a: np.repeat(np.repeat(a, 5, axis=0), 6, axis=1)[:h, :w]      # noqa: E731
    ids = up(rng.integers(0, 4, (by, bx)).astype(np.uint32))
    Fp = np.zeros((h, w, 8), F)
    Fp[..., 0:3] = up(rng.uniform(0.0, 1.0, (by, bx, 3)))
    n = up(rng.normal(0.0, 1.0, (by, bx, 3))) + rng.normal(0.0, 0.05, (h, w, 3))
    Fp[..., 3:6] = n / np.sqrt((n * n).sum(axis=-1))[..., None]
    Fp[..., 6] = up(rng.uniform(20.0, 400.0, (by, bx))) * (1.0 + rng.normal(0.0, 0.002, (h, w)))
    sky = ids == 3
    Fp[sky, :7] = 0.0
    Fp[..., 7] = np.where(sky, np.uint32(0xFFFFFFFF), ids).astype(np.uint32).view(F)
    if kind == "constant":
        Fp[...] = Fp[h // 2, w // 2]
        Fp[..., 0:7] = np.where(Fp[..., 0:7] == 0, F(0.25), Fp[..., 0:7])
    if kind == "nan":
        for (y, x), c in zip(((h // 3, w // 2), (h // 2, w // 3), (h - 1, w - 1)), (1, 4, 6)):
            Fp[y, x, c] = np.nan
    Fp.setflags(write=False)
    return Fp


def feature_kind(kind):
    return "nan" if kind == "nonfinite" else "blocks"


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    for name in ("rt_guide_defaults", "rt_set_denoise_guide", "rt_denoise_guided_planes", "rt_denoise_pair_guided_planes"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    assert callable(api.RtContext.set_denoise_guide) and callable(api.denoise_guided_planes) and callable(api.denoise_pair_guided_planes)


def test_the_struct_is_16_bytes_and_the_defaults_are_015_02_005():
    assert C.sizeof(api.GuideParams) == 16
    assert {n: getattr(api.GuideParams, n).offset for n, _ in api.GuideParams._fields_} == {"k_albedo": 0, "k_normal": 4, "k_depth": 8, "reserved": 12}
    g = api.guide_defaults()
    assert (F(g.k_albedo), F(g.k_normal), F(g.k_depth), g.reserved) == (F(0.15), F(0.2), F(0.05), 0)
    api.load_library().rt_guide_defaults(None)               # a null pointer is ignored


def test_the_restatement_without_a_guide_is_the_unguided_restatement():
    w, h = 41, 23
    D, A, B = planes(w, h, "nonfinite")
    Fp = features(w, h)
    assert_same_bits(guided_restated(D, A, B, Fp, w, h, None, **PARAMS[0]), denoise_restated(D, A, B, w, h, **PARAMS[0]))
    for got, want in zip(pair_guided_restated(A, B, Fp, w, h, None, **PARAMS[0]), pair_restated(A, B, w, h, **PARAMS[0])):
        assert_same_bits(got, want)


@pytest.mark.parametrize("w,h,params,kind", CASES, ids=CASE_IDS)
def test_guided_planes_equals_the_restatement_bit_for_bit(w, h, params, kind):
    D, A, B = planes(w, h, kind)
    Fp = features(w, h, feature_kind(kind))
    got = api.denoise_guided_planes(D, A, B, Fp, w, h, params, GUIDE)
    assert_same_bits(got, guided_restated(D, A, B, Fp, w, h, GUIDE, **params))
    if params["search_radius"] > 1:
        assert not np.array_equal(got, api.denoise_planes(D, A, B, w, h, params), equal_nan=True)      # (the guide did something)


@pytest.mark.parametrize("w,h,params,kind", CASES, ids=CASE_IDS)
def test_pair_guided_planes_equals_the_restatement_bit_for_bit(w, h, params, kind):
    _, A, B = planes(w, h, kind)
    Fp = features(w, h, feature_kind(kind))
    fa, fb = api.denoise_pair_guided_planes(A, B, Fp, w, h, params, GUIDE)
    wa, wb = pair_guided_restated(A, B, Fp, w, h, GUIDE, **params)
    assert_same_bits(fa, wa)
    assert_same_bits(fb, wb)
    sa, sb = api.denoise_pair_guided_planes(B, A, Fp, w, h, params, GUIDE)      # exchanging the halves exchanges FA and FB
    assert_same_bits(sa, fb)
    assert_same_bits(sb, fa)


def test_a_nan_feature_constrains_nothing():
    """A NaN term of rule 13 is skipped by its comparison: a NaN in the feature plane reaches no output pixel."""
    w, h = 41, 23
    D, A, B = planes(w, h)
    got = api.denoise_guided_planes(D, A, B, features(w, h, "nan"), w, h, PARAMS[0], GUIDE)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("kind", ["noisy", "nonfinite"])
def test_the_three_identities(kind):
    w, h = 41, 23
    D, A, B = planes(w, h, kind)
    Fp = features(w, h)
    for P in (0, 1, 2):                                      # R = 0: the input
        r0 = {"search_radius": 0, "patch_radius": P}
        assert_same_bits(api.denoise_guided_planes(D, A, B, Fp, w, h, r0, GUIDE), D)
        for got, want in zip(api.denoise_pair_guided_planes(A, B, Fp, w, h, r0, GUIDE), (A, B)):
            assert_same_bits(got, want)
    for params in PARAMS:
        plain = api.denoise_planes(D, A, B, w, h, params)
        pair = api.denoise_pair_planes(A, B, w, h, params)
        for feat, guide in ((Fp, WIDE), (features(w, h, "constant"), GUIDE)):      # every k 1e18 and finite features; a constant plane: wf is exactly 1
            assert_same_bits(api.denoise_guided_planes(D, A, B, feat, w, h, params, guide), plain)
            for got, want in zip(api.denoise_pair_guided_planes(A, B, feat, w, h, params, guide), pair):
                assert_same_bits(got, want)


def test_a_null_guide_is_the_unguided_function():
    w, h = 41, 23
    D, A, B = planes(w, h, "nonfinite")
    for params in PARAMS:
        assert_same_bits(api.denoise_guided_planes(D, A, B, None, w, h, params, None), api.denoise_planes(D, A, B, w, h, params))
        for got, want in zip(api.denoise_pair_guided_planes(A, B, None, w, h, params, None), api.denoise_pair_planes(A, B, w, h, params)):
            assert_same_bits(got, want)


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    one, feat, out, out2 = np.zeros(3, F), np.ones(8, F), np.zeros(3, F), np.zeros(3, F)
    p = api._ptr
    nan, inf = float("nan"), float("inf")
    for name in ("k_albedo", "k_normal", "k_depth"):
        for bad in (0.0, -0.5, nan, inf):
            for call in (lambda g: api.denoise_guided_planes(one, one, one, feat, 1, 1, None, g), lambda g: api.denoise_pair_guided_planes(one, one, feat, 1, 1, None, g)):
                with pytest.raises(api.RtError) as err:
                    call({name: bad})
                assert err.value.code == RT_ERR_ARG and name in str(err.value)
    for call in (lambda g: api.denoise_guided_planes(one, one, one, feat, 1, 1, None, g), lambda g: api.denoise_pair_guided_planes(one, one, feat, 1, 1, None, g)):
        with pytest.raises(api.RtError) as err:
            call({"reserved": 1})
        assert err.value.code == RT_ERR_ARG and "reserved" in str(err.value)
        call(GUIDE)
    g = api.guide_defaults()
    assert lib.rt_denoise_guided_planes(p(out), p(one), p(one), p(one), None, 1, 1, None, C.byref(g)) == RT_ERR_ARG           # a guide and no feature plane
    assert lib.rt_denoise_pair_guided_planes(p(out), p(out2), p(one), p(one), None, 1, 1, None, C.byref(g)) == RT_ERR_ARG
    assert lib.rt_denoise_guided_planes(None, p(one), p(one), p(one), p(feat), 1, 1, None, C.byref(g)) == RT_ERR_ARG
    with pytest.raises(api.RtError):
        api.denoise_guided_planes(one, one, one, feat, 1, 1, {"k": 0.0}, GUIDE)      # the filter's own refusals stay
    with pytest.raises(ValueError):
        api.denoise_guided_planes(one, one, one, feat, 1, 1, None, {"k_colour": 1.0})
    assert not out.any()


# ---- what it is for ---------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the gain rt_denoise_guided_planes itself measured in this set-up, dB (include/rt_api.h quotes it); the test asserts HALF of it
MEASURED_GAIN = {"cornell": 0.54, "simple": 1.24}


def psnr8(img, ref):
    """PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5."""
    pack = lambda c: (np.clip(np.asarray(c, np.float64), 0.0, 1.0) ** (1 / 2.2) * 255 + .5).astype(np.int64)      # noqa: E731
    d = pack(img) - pack(ref)
    return 10 * np.log10(255.0 ** 2 / np.mean(d.astype(np.float64) ** 2))


@functools.lru_cache(maxsize=None)
def guided_gain(name, w=96, h=96, n=4, truth=1024):
    """(unguided, guided) PSNR of the filtered merge of two halves of n passes on seed streams 1 and 2 against `truth` oracle passes."""
    if name == "demo":
        sph, cam = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    else:
        z = np.load(os.path.join(GOLDEN, name + "_96x96_4spp.npz"))
        sph, c = z["spheres"].view(api.SPHERE_DT).copy(), z["camera"].astype(F)
        cam = host.compute_camera(tuple(c[0:3]), tuple(c[3:6]), w, h)
    A, B = (O.render(sph, cam, w, h, n, seeds_in=api.stream_seeds(s, 2 * w * h), threads=16)["colors"] for s in (1, 2))
    ref = O.render(sph, cam, w, h, truth, threads=16)["colors"]
    merged = ((A * F(n) + B * F(n)) * (F(1.0) / F(2 * n))).astype(F)
    Fp = api.features_planes(sph, cam, w, h)
    return psnr8(api.denoise_planes(merged, A, B, w, h), ref), psnr8(api.denoise_guided_planes(merged, A, B, Fp, w, h, None, api.guide_defaults()), ref)


@pytest.mark.parametrize("name", ["cornell", "simple"])
def test_the_guide_gains_over_the_unguided_filter_on_diffuse_scenes(name, capsys):
    plain, guided = guided_gain(name)
    with capsys.disabled():
        print("\n[guided] %s 96x96, 4 passes per half: unguided %.2f dB, guided %.2f dB (gain %.2f dB)" % (name, plain, guided, guided - plain))
    assert MEASURED_GAIN[name] >= 0.3                        # (below that on cornell, something differs from the prototype)
    assert guided - plain >= 0.5 * MEASURED_GAIN[name]


def test_the_guide_costs_the_glass_scene_at_most_a_tenth_of_a_db(capsys):
    plain, guided = guided_gain("demo")
    with capsys.disabled():
        print("\n[guided] Demo 96x96, 4 passes per half: unguided %.2f dB, guided %.2f dB (gain %.2f dB)" % (plain, guided, guided - plain))
    assert guided >= plain - 0.1
