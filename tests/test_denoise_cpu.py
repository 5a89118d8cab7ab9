"""Denoising (include/rt_api.h "denoising", csrc/rt_denoise.hip), the part that needs no device: a numpy restatement of rules 1-6 written
independently of rt_host.cpp (whole-plane shifts where the host function loops over pixels), pinned by scalar loops straight from the rules at a
corner and an interior pixel; rt_denoise_planes against it bit for bit; the struct, the defaults, the argument checks; and what the filter is
for -- the PSNR it gains over the merged frame, with frames of the oracle alone.  tests/test_gpu_denoise.py compares the device with
rt_denoise_planes and imports the planes of this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host

F = np.float32
SIZES = [(1, 1), (8, 8), (41, 23), (70, 19)]
PARAMS = [{"search_radius": 5, "patch_radius": 1}, {"search_radius": 8, "patch_radius": 2}, {"search_radius": 1, "patch_radius": 0}]
OTHER = {"search_radius": 5, "patch_radius": 1, "alpha": 0.5, "k": 0.7}          # at 41x23 only
RT_ERR_ARG = -1


def full(params):
    return {"search_radius": 5, "patch_radius": 1, "alpha": 1.0, "k": 0.45, **params}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _shift(X, dy, dx):
    """X[cl(y + dy, x + dx)] for every (y, x): the plane moved by an offset, clamped at the image's border."""
    h, w = X.shape[:2]
    return X[np.clip(np.arange(h) + dy, 0, h - 1)[:, None], np.clip(np.arange(w) + dx, 0, w - 1)[None, :]]


def _sum_window(X, r):
    """Sum over the (2r + 1)^2 clamped neighbours, dy outer, dx inner, starting from the first term."""
    acc = None
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            term = _shift(X, dy, dx)
            acc = term if acc is None else acc + term
    return acc


def smoothed_variance(A, B):
    d = (A - B) * F(0.5)
    return _sum_window(d * d, 1) * (F(1.0) / F(9.0))


def denoise_restated(D, A, B, w, h, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """Rules 1-6 of include/rt_api.h on float32 planes [3 * w * h]; every operation one float32 numpy operation, in the stated order."""
    D, A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (D, A, B))
    R, P = search_radius, patch_radius
    alpha, kk, inv = F(alpha), F(k) * F(k), F(1.0) / F(3 * (2 * P + 1) * (2 * P + 1))
    ys, xs = np.arange(h), np.arange(w)
    with np.errstate(all="ignore"):
        Vs = smoothed_variance(A, B)
        num, den = np.zeros((h, w, 3), F), np.zeros((h, w), F)
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                if oy == 0 and ox == 0:
                    num, den = num + F(1.0) * D, den + F(1.0)
                    continue
                Dq, Vq = _shift(D, oy, ox), _shift(Vs, oy, ox)
                t = D - Dq
                m = np.where(Vq < Vs, Vq, Vs)
                dc = (t * t - alpha * (Vs + m)) / (F(1e-10) + kk * (Vs + Vq))
                e = (dc[..., 0] + dc[..., 1]) + dc[..., 2]
                T = _sum_window(e, P) * inv
                inside = ((ys + oy >= 0) & (ys + oy < h))[:, None] & ((xs + ox >= 0) & (xs + ox < w))[None, :]
                take = inside & ~np.isnan(T) & np.isfinite(Dq).all(axis=-1)
                g = np.where(T > 0, T, F(0.0))
                wgt = F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5)))
                num = np.where(take[..., None], num + wgt[..., None] * Dq, num)
                den = np.where(take, den + wgt, den)
        out = num / den[..., None]
    assert out.dtype == F and Vs.dtype == F
    return out.reshape(-1)


def pixel_by_hand(D, A, B, w, h, py, px, search_radius=5, patch_radius=1, alpha=1.0, k=0.45):
    """One output pixel by scalar loops straight from the rules: nothing shared, every e(cl(p + delta), o) formed where it is used."""
    D, A, B = (np.asarray(x, F).reshape(h, w, 3) for x in (D, A, B))
    R, P = search_radius, patch_radius
    alpha, kk, inv = F(alpha), F(k) * F(k), F(1.0) / F(3 * (2 * P + 1) * (2 * P + 1))

    def cl(y, x):
        return min(max(y, 0), h - 1), min(max(x, 0), w - 1)

    @functools.lru_cache(maxsize=None)                       # (a value per position and channel: formed once, by the rule)
    def vs(y, x, c):
        acc = None
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                d = (A[cl(y + j, x + i)][c] - B[cl(y + j, x + i)][c]) * F(0.5)
                acc = d * d if acc is None else acc + d * d
        return acc * (F(1.0) / F(9.0))

    def e(y, x, oy, ox):
        q = cl(y + oy, x + ox)
        d = []
        for c in range(3):
            t = D[y, x, c] - D[q][c]
            vp, vq = vs(y, x, c), vs(q[0], q[1], c)
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
                    if np.isnan(T) or not np.isfinite(D[qy, qx]).all():
                        continue
                    g = T if T > 0 else F(0.0)
                    wgt = F(1.0) / (F(1.0) + g * (F(1.0) + g * F(0.5)))
                num = [num[c] + wgt * D[qy, qx, c] for c in range(3)]
                den = den + wgt
        out = np.array([num[c] / den for c in range(3)])
    assert out.dtype == F
    return out


# ---- the planes --------------------------------------------------------------------------------------------------------
PLANTED = [(0, 0, 1, np.nan), (1, 2, 0, np.inf), (0, 3, 2, -np.inf)]      # (fraction of h, of w) in thirds, channel, value: see planes()


@functools.lru_cache(maxsize=None)
def planes(w, h, kind="noisy"):
    """(D, A, B), float32 [3 * w * h], read-only, values in 0 .. 4 (some above 1: they clamp when packed).
    noisy: blocks of 4x4 pixels of one colour, two halves with independent noise on it, D their mean -- the merge of equal halves;
    equal: A == B, D of two values only (variance zero: weight 1 between identical patches, next to none otherwise);
    nonfinite: `noisy` with a NaN, +inf and -inf planted in D (the NaN in the corner (0, 0)) and a NaN in A."""
    rng = np.random.default_rng(1000 * w + h)
    base = np.repeat(np.repeat(rng.uniform(0.0, 4.0, ((h + 3) // 4, (w + 3) // 4, 3)), 4, axis=0), 4, axis=1)[:h, :w].astype(F)
    if kind == "equal":
        D = np.where(base > 2.0, F(3.0), F(1.0)).astype(F)
        A = B = rng.uniform(0.0, 4.0, (h, w, 3)).astype(F)
    else:
        A = np.clip(base + rng.normal(0.0, 0.3, base.shape).astype(F), 0.0, 4.0).astype(F)
        B = np.clip(base + rng.normal(0.0, 0.3, base.shape).astype(F), 0.0, 4.0).astype(F)
        D = ((A * F(4.0) + B * F(4.0)) * (F(1.0) / F(8.0))).astype(F)
    if kind == "nonfinite":
        D, A = D.copy(), A.copy()
        for y, x, c, v in planted(w, h):
            D[y, x, c] = v
        A[h // 2, w // 2, 1] = np.nan
    out = tuple(np.ascontiguousarray(x, F).reshape(-1) for x in (D, A, B))
    for x in out:
        x.setflags(write=False)
    return out


def planted(w, h):
    return [(fy * (h - 1) // 3, fx * (w - 1) // 3, c, v) for fy, fx, c, v in PLANTED]


def assert_same_bits(got, want):
    """Bit for bit where the wanted value is finite; non-finite values by position only."""
    got, want = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    for name in ("rt_denoise_defaults", "rt_denoise_async", "rt_denoise_planes"):
        assert name in api.SYMBOLS and callable(getattr(lib, name))
    assert callable(api.RtContext.denoise) and callable(api.denoise_planes) and callable(api.denoise_defaults)


def test_the_struct_is_16_bytes_and_the_defaults_are_5_1_1_045():
    assert C.sizeof(api.DenoiseParams) == 16
    assert {n: getattr(api.DenoiseParams, n).offset for n, _ in api.DenoiseParams._fields_} == \
        {"search_radius": 0, "patch_radius": 4, "alpha": 8, "k": 12}
    p = api.denoise_defaults()
    assert (p.search_radius, p.patch_radius) == (5, 1) and F(p.alpha) == F(1.0) and F(p.k) == F(0.45)
    api.load_library().rt_denoise_defaults(None)             # a null pointer is ignored


def _id(params):
    return "R%d-P%d" % (params["search_radius"], params["patch_radius"]) + ("-alpha%g-k%g" % (params["alpha"], params["k"]) if "k" in params else "")


CASES = [(w, h, p) for w, h in SIZES for p in PARAMS] + [(41, 23, OTHER)]
CASE_IDS = ["%dx%d-%s" % (w, h, _id(p)) for w, h, p in CASES]


@pytest.mark.parametrize("w,h,params", CASES, ids=CASE_IDS)
def test_denoise_planes_equals_the_restatement_bit_for_bit(w, h, params):
    D, A, B = planes(w, h)
    got = api.denoise_planes(D, A, B, w, h, params)
    want = denoise_restated(D, A, B, w, h, **params)
    assert np.isfinite(want).all()
    assert_same_bits(got, want)
    if w * h > 1 and params["search_radius"] > 1:
        assert not np.array_equal(got, D)                    # (the filter did something)
    assert_same_bits(api.denoise_planes(D, A, B, w, h, full(params)), want)       # the four fields spelt out


def test_null_parameters_are_the_defaults_and_radius_0_is_the_image():
    D, A, B = planes(41, 23)
    assert_same_bits(api.denoise_planes(D, A, B, 41, 23), denoise_restated(D, A, B, 41, 23, 5, 1, 1.0, 0.45))
    for P in (0, 1, 2):
        assert_same_bits(api.denoise_planes(D, A, B, 41, 23, {"search_radius": 0, "patch_radius": P}), D)
        assert_same_bits(denoise_restated(D, A, B, 41, 23, 0, P), D)


@pytest.mark.parametrize("params", PARAMS, ids=["R5-P1", "R8-P2", "R1-P0"])
def test_equal_halves_have_no_variance_and_only_identical_patches_mix(params):
    w, h = 41, 23
    D, A, B = planes(w, h, "equal")
    assert np.array_equal(A, B) and not smoothed_variance(A.reshape(h, w, 3), B.reshape(h, w, 3)).any()
    got = api.denoise_planes(D, A, B, w, h, params)
    assert_same_bits(got, denoise_restated(D, A, B, w, h, **params))
    if params["patch_radius"] == 0:
        # a pixel's patch is the pixel: distance 0 and weight 1 to an identical pixel, (1 or 4 or ...) / 1e-10 and a weight below 1e-19 to any other;
        # the sum of n equal small integers divided by n is that integer
        assert_same_bits(got, D)


@pytest.mark.parametrize("params", PARAMS, ids=["R5-P1", "R8-P2", "R1-P0"])
def test_a_non_finite_pixel_stays_non_finite_and_spreads_to_no_neighbour(params):
    w, h = 41, 23
    D, A, B = planes(w, h, "nonfinite")
    assert (0, 0, 1) in [(y, x, c) for y, x, c, _ in planted(w, h)] and np.isnan(A).sum() == 1
    got = api.denoise_planes(D, A, B, w, h, params)
    assert_same_bits(got, denoise_restated(D, A, B, w, h, **params))
    bad = np.zeros((h, w, 3), bool)
    for y, x, c, _ in planted(w, h):
        bad[y, x, c] = True
    assert np.array_equal(~np.isfinite(got).reshape(h, w, 3), bad)              # exactly the planted D values; the NaN of A reaches nothing


@pytest.mark.parametrize("kind", ["noisy", "nonfinite"])
def test_the_restatement_equals_scalar_loops_at_a_corner_and_inside(kind):
    """The border pin: rule 4 takes e at the clamped position and THAT position's clamped partner.  A restatement (or a kernel) that clamps
    p + delta + o instead differs at the corner."""
    w, h = 41, 23
    D, A, B = planes(w, h, kind)
    for params in (PARAMS[0], PARAMS[1], OTHER):
        want = denoise_restated(D, A, B, w, h, **params).reshape(h, w, 3)
        for y, x in ((h - 1, w - 1), (0, 1), (11, 17)):      # a corner, beside the planted corner, inside
            by_hand = pixel_by_hand(D, A, B, w, h, y, x, **params)
            assert_same_bits(by_hand, want[y, x])


def test_the_single_clamp_would_differ_at_the_corner():
    """... and the pin can tell: e taken at cl(p + delta + o) gives another corner pixel."""
    w, h = 41, 23
    D, A, B = planes(w, h)
    D3, Vs = D.reshape(h, w, 3), smoothed_variance(A.reshape(h, w, 3), B.reshape(h, w, 3))
    y, x, oy, ox = h - 1, w - 1, -2, -3

    def e(py, px, qy, qx):
        t = D3[py, px] - D3[qy, qx]
        vp, vq = Vs[py, px], Vs[qy, qx]
        dc = (t * t - F(1.0) * (vp + np.where(vq < vp, vq, vp))) / (F(1e-10) + F(0.45) * F(0.45) * (vp + vq))
        return (dc[0] + dc[1]) + dc[2]

    cl = lambda v, n: min(max(v, 0), n - 1)                  # noqa: E731
    double = [e(cl(y + dy, h), cl(x + dx, w), cl(cl(y + dy, h) + oy, h), cl(cl(x + dx, w) + ox, w)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    single = [e(cl(y + dy, h), cl(x + dx, w), cl(y + dy + oy, h), cl(x + dx + ox, w)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    assert not np.array_equal(np.array(double), np.array(single))


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    one = np.zeros(3, F)
    out = np.zeros(3, F)
    other = C.c_void_p(8)                                    # never dereferenced: a null context is refused first

    def refused(rc):
        assert rc == RT_ERR_ARG and lib.rt_last_error() != b""

    for ctxs in ((None, other, other), (other, None, other), (other, other, None)):
        refused(lib.rt_denoise_async(*ctxs, None, None))
        assert b"null" in lib.rt_last_error()
    p = api._ptr
    for planes_ in ((None, p(one), p(one), p(one)), (p(out), None, p(one), p(one)), (p(out), p(one), None, p(one)), (p(out), p(one), p(one), None)):
        refused(lib.rt_denoise_planes(*planes_, 1, 1, None))
    for w, h in ((0, 1), (1, 0), (-3, 4)):
        refused(lib.rt_denoise_planes(p(out), p(one), p(one), p(one), w, h, None))
    nan, inf = float("nan"), float("inf")
    for bad in ({"search_radius": -1}, {"search_radius": 9}, {"patch_radius": -1}, {"patch_radius": 3}, {"alpha": -0.25}, {"alpha": nan},
                {"alpha": inf}, {"k": 0.0}, {"k": -1.0}, {"k": nan}, {"k": inf}):
        with pytest.raises(api.RtError) as err:
            api.denoise_planes(one, one, one, 1, 1, bad)
        assert err.value.code == RT_ERR_ARG and list(bad)[0] in str(err.value)
    assert not out.any()
    for good in ({"search_radius": 0}, {"search_radius": 8, "patch_radius": 2}, {"alpha": 0.0}, {"patch_radius": 0}):
        api.denoise_planes(one, one, one, 1, 1, good)
    with pytest.raises(ValueError):
        api.denoise_planes(one, one, one, 1, 1, {"radius": 3})


def test_the_filter_gains_3_db_over_the_merged_frame_at_4_passes_per_half(capsys):
    """The Demo scene at 96x64 with the oracle alone: halves of 4 passes on seed streams 1 and 2, their merge by rt_merge_async's rule, the
    filter at its defaults, all three packed by the oracle's toInt and held against 4096 passes of the default stream.  The header's table
    (numpy's pack) has 14.8 / 20.4 / 27.7 dB; the bound is a little under half that gain and far above what a filter that does nothing gives."""
    w, h, n = 96, 64, 4
    sph, cam = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    A, B = (O.render(sph, cam, w, h, n, seeds_in=api.stream_seeds(s, 2 * w * h), threads=16)["colors"] for s in (1, 2))
    ref = O.render(sph, cam, w, h, 4096, threads=16)["colors"]
    merged = ((A * F(n) + B * F(n)) * (F(1.0) / F(2 * n))).astype(F)
    filtered = api.denoise_planes(merged, A, B, w, h)
    lib = O.oracle()

    def pack(colors):
        ch = np.array([lib.orc_to_int(float(v)) for v in colors], np.uint32).reshape(-1, 3)
        return ch[:, 0] | (ch[:, 1] << 8) | (ch[:, 2] << 16)

    want = pack(ref)
    pair, before, after = O.psnr(pack(A), pack(B)), O.psnr(pack(merged), want), O.psnr(pack(filtered), want)
    with capsys.disabled():
        print("\n[denoise] Demo 96x64, %d passes per half: pair %.2f dB, merged %.2f dB, filtered %.2f dB (gain %.2f dB)"
              % (n, pair, before, after, after - before))
    assert after - before >= 3.0
