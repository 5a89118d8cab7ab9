"""The error of the filtered frame (include/rt_api.h "the error of the filtered frame"), the part that needs no device: a numpy restatement
of rules 7-9 written independently of rt_host.cpp (whole-plane shifts, the helpers of tests/test_denoise_cpu.py), pinned by scalar loops straight
from the rules at a corner, beside it and inside; rt_denoise_pair_planes against it bit for bit; the properties the header states; the
refusals; and what the cross-filtered pair is for -- its PSNR against the true quality of the filtered merge, with frames of the oracle alone.
tests/test_gpu_denoise_pair.py compares the device with rt_denoise_pair_planes and imports the frames of this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host
from test_denoise_cpu import CASE_IDS, CASES, OTHER, PARAMS, F, _shift, _sum_window, assert_same_bits, planes, smoothed_variance

RT_ERR_ARG = -1
SYMBOLS = ("rt_denoise_pair_async", "rt_denoise_pair_planes", "rt_read_filtered", "rt_compare_filtered_async", "rt_compare_filtered",
           "rt_render_converged_filtered", "rt_render_adaptive_filtered")


# ---- the restatement ---------------------------------------------------------------------------------------------------
def cross_restated(X, G, Vh, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """Rule 8 for one direction on [h, w, 3] float32 planes: X's values, the weights from G and Vh; one float32 numpy operation per step."""
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
            Xq, Gq, Vq = _shift(X, oy, ox), _shift(G, oy, ox), _shift(Vh, oy, ox)
            t = G - Gq
            m = np.where(Vq < Vh, Vq, Vh)
            dc = (t * t - alpha * (Vh + m)) / (F(1e-10) + kk * (Vh + Vq))
            T = _sum_window((dc[..., 0] + dc[..., 1]) + dc[..., 2], P) * inv
            inside = ((ys + oy >= 0) & (ys + oy < h))[:, None] & ((xs + ox >= 0) & (xs + ox < w))[None, :]
            take = inside & ~np.isnan(T) & np.isfinite(Xq).all(axis=-1)
            g = np.where(T > 0, T, F(0.0))
            wgt = F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5)))
            num = np.where(take[..., None], num + wgt[..., None] * Xq, num)
            den = np.where(take, den + wgt, den)
    out = num / den[..., None]
    assert out.dtype == F
    return out


def pair_restated(A, B, w, h, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """Rules 7-9: (FA, FB), float32 [3 * w * h] each."""
    A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (A, B))
    if search_radius == 0:
        return A.reshape(-1).copy(), B.reshape(-1).copy()
    with np.errstate(all="ignore"):
        Vs = smoothed_variance(A, B)
        Vh = Vs + Vs
        assert Vh.dtype == F
        kw = dict(search_radius=search_radius, patch_radius=patch_radius, alpha=alpha, k=k)
        return cross_restated(A, B, Vh, **kw).reshape(-1), cross_restated(B, A, Vh, **kw).reshape(-1)


def pixel_by_hand(X, G, A, B, w, h, py, px, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """One pixel of FX by scalar loops straight from the rules: nothing shared, every e(cl(p + delta), o) formed where it is used."""
    X, G, A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (X, G, A, B))
    R, P = search_radius, patch_radius
    alpha, kk, inv = F(alpha), F(k) * F(k), F(1.0) / F(3 * (2 * P + 1) * (2 * P + 1))

    def cl(y, x):
        return min(max(y, 0), h - 1), min(max(x, 0), w - 1)

    @functools.lru_cache(maxsize=None)
    def vh(y, x, c):
        acc = None
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                d = (A[cl(y + j, x + i)][c] - B[cl(y + j, x + i)][c]) * F(0.5)
                acc = d * d if acc is None else acc + d * d
        vs = acc * (F(1.0) / F(9.0))
        return vs + vs

    def e(y, x, oy, ox):
        q = cl(y + oy, x + ox)                              # the clamped position's OWN clamped partner
        d = []
        for c in range(3):
            t = G[y, x, c] - G[q][c]
            vp, vq = vh(y, x, c), vh(q[0], q[1], c)
            m = vq if vq < vp else vp
            d.append((t * t - alpha * (vp + m)) / (F(1e-10) + kk * (vp + vq)))
        return (d[0] + d[1]) + d[2]

    num, den = [F(0.0)] * 3, F(0.0)
    with np.errstate(all="ignore"):
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                qy, qx = py + oy, px + ox
                if (oy, ox) == (0, 0):
                    wgt = F(1.0)
                elif not (0 <= qy < h and 0 <= qx < w):
                    continue
                else:
                    S = None
                    for dy in range(-P, P + 1):
                        for dx in range(-P, P + 1):
                            term = e(*cl(py + dy, px + dx), oy, ox)
                            S = term if S is None else S + term
                    T = S * inv
                    if np.isnan(T) or not np.isfinite(X[qy, qx]).all():
                        continue
                    g = T if T > 0 else F(0.0)
                    wgt = F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5)))
                num = [num[c] + wgt * X[qy, qx, c] for c in range(3)]
                den = den + wgt
        out = np.array([num[c] / den for c in range(3)])
    assert out.dtype == F
    return out


# ---- frames of the oracle, shared with the device tests ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def demo_halves(n, w=96, h=64):
    """The Demo scene's colour planes after n passes on seed streams 1 and 2 (oracle), read-only."""
    sph, cam = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    out = tuple(O.render(sph, cam, w, h, n, seeds_in=api.stream_seeds(s, 2 * w * h), threads=16)["colors"] for s in (1, 2))
    for x in out:
        x.setflags(write=False)
    return out


def pack(colors):
    """The oracle's toInt over a plane, one word per pixel in the plane's own order."""
    lib = O.oracle()
    ch = np.array([lib.orc_to_int(float(v)) for v in colors], np.uint32).reshape(-1, 3)
    return ch[:, 0] | (ch[:, 1] << 8) | (ch[:, 2] << 16)


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    for name in SYMBOLS:
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    for name in ("denoise_pair", "read_filtered", "compare_filtered", "compare_filtered_async", "render_converged_filtered",
                 "render_adaptive_filtered"):
        assert callable(getattr(api.RtContext, name))
    assert callable(api.denoise_pair_planes)


@pytest.mark.parametrize("w,h,params", CASES, ids=CASE_IDS)
def test_pair_planes_equals_the_restatement_bit_for_bit(w, h, params):
    _, A, B = planes(w, h)
    assert np.isfinite(A).all() and np.isfinite(B).all()
    got = api.denoise_pair_planes(A, B, w, h, params)
    want = pair_restated(A, B, w, h, **params)
    for g, wnt, X in zip(got, want, (A, B)):
        assert np.isfinite(wnt).all()
        assert np.array_equal(g.view(np.uint32), wnt.view(np.uint32))       # every value, both outputs
        if w * h > 1 and params["search_radius"] > 1:
            assert not np.array_equal(g, X)                  # (the filter did something)
    if w * h > 1:
        # ... and not what rt_denoise_planes gives for either half as the image: the guide is the OTHER half and the variance is doubled
        assert not np.array_equal(got[0], api.denoise_planes(A, A, B, w, h, params))


@pytest.mark.parametrize("kind", ["noisy", "nonfinite"])
def test_the_restatement_equals_scalar_loops_at_a_corner_beside_it_and_inside(kind):
    """The border pin of rule 4, in both directions: e at the clamped position and THAT position's clamped partner."""
    w, h = 41, 23
    D, A, B = planes(w, h, kind)
    A = D if kind == "nonfinite" else A                      # (the planted values in a half: the plane with a NaN, +inf and -inf)
    for params in (PARAMS[0], PARAMS[1], OTHER):
        FA, FB = (x.reshape(h, w, 3) for x in pair_restated(A, B, w, h, **params))
        for y, x in ((h - 1, w - 1), (0, 1), (11, 17)):
            assert_same_bits(pixel_by_hand(A, B, A, B, w, h, y, x, **params), FA[y, x])
            assert_same_bits(pixel_by_hand(B, A, A, B, w, h, y, x, **params), FB[y, x])


def test_radius_0_returns_the_halves_and_null_parameters_are_the_defaults():
    w, h = 41, 23
    D, A, B = planes(w, h, "nonfinite")
    for P in (0, 1, 2):
        FA, FB = api.denoise_pair_planes(D, B, w, h, {"search_radius": 0, "patch_radius": P})
        assert np.array_equal(FA.view(np.uint32), D.view(np.uint32)) and np.array_equal(FB.view(np.uint32), B.view(np.uint32))
    _, A, B = planes(w, h)
    for got, want in zip(api.denoise_pair_planes(A, B, w, h), pair_restated(A, B, w, h, 5, 1, 1.0, 0.45)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("params", PARAMS, ids=["R5-P1", "R8-P2", "R1-P0"])
def test_swapping_the_halves_swaps_the_outputs(params):
    w, h = 41, 23
    _, A, B = planes(w, h)
    FA, FB = api.denoise_pair_planes(A, B, w, h, params)
    GB, GA = api.denoise_pair_planes(B, A, w, h, params)
    assert np.array_equal(FA.view(np.uint32), GA.view(np.uint32)) and np.array_equal(FB.view(np.uint32), GB.view(np.uint32))


@pytest.mark.parametrize("params", PARAMS, ids=["R5-P1", "R8-P2", "R1-P0"])
def test_a_non_finite_value_stays_at_its_place_and_spreads_nowhere(params):
    """The half with a NaN, +inf and -inf planted (test_denoise_cpu.planes "nonfinite": its D) beside a finite half: FX is non-finite exactly
    where X is, and so is the other output finite everywhere -- there the planted values are in the guide, and only remove offsets."""
    w, h = 41, 23
    X, _, B = planes(w, h, "nonfinite")
    FX, FB = api.denoise_pair_planes(X, B, w, h, params)
    want = pair_restated(X, B, w, h, **params)
    assert_same_bits(FX, want[0])
    assert_same_bits(FB, want[1])
    assert np.array_equal(~np.isfinite(FX), ~np.isfinite(X)) and (~np.isfinite(X)).sum() == 3
    assert np.isfinite(FB).all()


def test_a_nan_in_the_guide_removes_only_the_offsets_whose_patches_touch_it():
    """P = 0, R = 1, a NaN in channel 1 of G at (11, 17).  It reaches Vh on the 3x3 around it, so e(x, o) is a NaN exactly where x or x + o lies in
    that 3x3: a pixel outside the 5x5 around it is untouched bit for bit; a pixel inside the 3x3 keeps its own value alone (every offset is
    removed, the centre weight stays)."""
    w, h, params = 41, 23, {"search_radius": 1, "patch_radius": 0}
    _, A, B = planes(w, h)
    G = B.copy()
    G.reshape(h, w, 3)[11, 17, 1] = np.nan
    FA, _ = (x.reshape(h, w, 3) for x in api.denoise_pair_planes(A, G, w, h, params))
    clean, _ = (x.reshape(h, w, 3) for x in api.denoise_pair_planes(A, B, w, h, params))
    assert np.isfinite(FA).all()
    far = np.ones((h, w), bool)
    far[8:15, 14:21] = False                                 # outside the 7x7: no offset of the pixel reads a touched e or Vh
    assert np.array_equal(FA[far].view(np.uint32), clean[far].view(np.uint32))
    near = A.reshape(h, w, 3)[10:13, 16:19]
    assert np.array_equal(FA[10:13, 16:19].view(np.uint32), near.view(np.uint32))
    assert not np.array_equal(clean[10:13, 16:19], near)


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    one, out_a, out_b = np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
    other = C.c_void_p(8)                                    # never dereferenced: a null context is refused first
    p = api._ptr
    err, n = api.FrameError(), C.c_int()

    def refused(rc):
        assert rc == RT_ERR_ARG and lib.rt_last_error() != b""

    for pair in ((None, other), (other, None)):
        for rc in (lib.rt_denoise_pair_async(*pair, None, None), lib.rt_compare_filtered_async(*pair, C.c_void_p(16), None, None),
                   lib.rt_compare_filtered(*pair, C.byref(err), None),
                   lib.rt_render_converged_filtered(*pair, 30.0, 1, 8, None, C.byref(err), C.byref(n)),
                   lib.rt_render_adaptive_filtered(*pair, 30.0, 1, 1, 8, None, C.byref(err), C.byref(n))):
            refused(rc)
            assert b"null" in lib.rt_last_error()
    refused(lib.rt_read_filtered(None, p(one)))
    for planes_ in ((None, p(out_b), p(one), p(one)), (p(out_a), None, p(one), p(one)), (p(out_a), p(out_b), None, p(one)),
                    (p(out_a), p(out_b), p(one), None)):
        refused(lib.rt_denoise_pair_planes(*planes_, 1, 1, None))
    for w, h in ((0, 1), (1, 0), (-3, 4)):
        refused(lib.rt_denoise_pair_planes(p(out_a), p(out_b), p(one), p(one), w, h, None))
    nan, inf = float("nan"), float("inf")
    for bad in ({"search_radius": -1}, {"search_radius": 9}, {"patch_radius": -1}, {"patch_radius": 3}, {"alpha": -0.25}, {"alpha": nan},
                {"alpha": inf}, {"k": 0.0}, {"k": -1.0}, {"k": nan}, {"k": inf}):
        with pytest.raises(api.RtError) as e:
            api.denoise_pair_planes(one, one, 1, 1, bad)
        assert e.value.code == RT_ERR_ARG and list(bad)[0] in str(e.value)
    assert not out_a.any() and not out_b.any()
    for good in ({"search_radius": 0}, {"search_radius": 8, "patch_radius": 2}, {"alpha": 0.0}, {"patch_radius": 0}):
        api.denoise_pair_planes(one, one, 1, 1, good)


def test_the_cross_filtered_pair_estimates_the_quality_of_the_filtered_merge(capsys):
    """The Demo scene at 96x64 with the oracle alone, 4 passes per half on seed streams 1 and 2, everything packed by the oracle's toInt,
    truth = 4096 passes of the default stream.  Measured when the arithmetic was prototyped: cross-filtered pair 28.00 dB, filtered merge against
    truth 27.69 dB, raw pair 14.78 dB.  The run is deterministic: the 1.5 dB are for last-bit differences of a restatement's pack, not for
    noise; the raw pair is 12.9 dB away."""
    w, h, n = 96, 64, 4
    A, B = demo_halves(n)
    sph, cam = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    truth = pack(O.render(sph, cam, w, h, 4096, threads=16)["colors"])
    merged = ((A * F(n) + B * F(n)) * (F(1.0) / F(2 * n))).astype(F)
    shown = O.psnr(pack(api.denoise_planes(merged, A, B, w, h)), truth)
    FA, FB = api.denoise_pair_planes(A, B, w, h)
    cross, raw = O.psnr(pack(FA), pack(FB)), O.psnr(pack(A), pack(B))
    with capsys.disabled():
        print("\n[filtered error] Demo 96x64, %d passes per half: cross-filtered pair %.2f dB, filtered merge against 4096 passes %.2f dB, raw pair %.2f dB"
              % (n, cross, shown, raw))
    assert abs(cross - shown) <= 1.5
    assert abs(raw - shown) > 10.0
