"""The shadow frames of tests/test_gpu_fast_shadow.py, proved without a GPU (tests/_shadow_frames.py): the ORACLE's one-pass frame of
every scene of that module must pass the same check under K.exact(); the cap of 2 % and the vacuity guards -- conditions on the reference
alone -- must hold under K.exact() and under K.measured(); tampered frames must fail, each with its own message; and the two closed
bounds that replace the running envelope for a shadow ray's own sphere and own light must contain what correctly rounded binary32
returns (R.pairs32) on random rays of exactly those two kinds, and be used only where they are not wider than what they replace.
Run with -s for the figures."""
import numpy as np
import pytest

import _fast_reference as R
import _oracle as O
import _shadow_frames as SF

F, D = np.float32, np.float64


@pytest.fixture(scope="module", params=list(SF.SCENES))
def oracle_frame(request):
    name = request.param
    sph, cam, _, _ = SF.scene(name)
    return name, O.render(sph, cam, SF.W, SF.H, 1, threads=16)["colors"], SF.reference(name, False)


def test_oracle_frame_agrees_with_binary64_light_by_light(oracle_frame):
    name, colors, ref = oracle_frame
    out = SF.check_frame("oracle / " + name, colors, ref)
    assert out["ratio"] <= 1.0


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "measured"])
def test_cap_and_vacuity_guards_hold_on_the_reference_alone(oracle_frame, fast):
    name = oracle_frame[0]
    if fast and R.K.measured() is None:
        pytest.skip("not measured yet: profiles/r20_fast_blocks.jsonl has no record")
    SF.check_reference("%s under K.%s()" % (name, "measured" if fast else "exact"), SF.reference(name, fast))


def test_one_percent_of_the_lit_answers_set_to_zero_fails(oracle_frame):
    name, colors, ref = oracle_frame
    with pytest.raises(AssertionError, match="dark where binary64 finds no blocker"):
        SF.check_frame("tampered / " + name, SF.tamper_lit_to_zero(colors, ref), ref, verbose=False)


def test_one_percent_of_the_dark_answers_lit_fails(oracle_frame):
    name, colors, ref = oracle_frame
    with pytest.raises(AssertionError, match="lit where binary64 is dark"):
        SF.check_frame("tampered / " + name, SF.tamper_dark_to_lit(colors, ref), ref, verbose=False)


@pytest.mark.parametrize("light", [0, 1])
def test_one_light_s_channel_one_percent_brighter_fails(oracle_frame, light):
    name, colors, ref = oracle_frame
    with pytest.raises(AssertionError, match="light %d: a lit channel outside the envelope of 8 k" % light):
        SF.check_frame("tampered / " + name, SF.tamper_scale(colors, light), ref, verbose=False)


def test_negative_zeros_pass(oracle_frame):
    name, colors, ref = oracle_frame
    bad = SF.tamper_negative_zero(colors)
    assert np.signbit(bad[bad == 0]).all() and (bad == 0).any()
    SF.check_frame("negative zeros / " + name, bad, ref, verbose=False)


def test_a_negative_or_non_finite_receiver_pixel_is_a_failure_not_an_exclusion(oracle_frame):
    name, colors, ref = oracle_frame
    px = int(np.nonzero(ref["pop"] & ~ref["decided"].all(0))[0][0]) if (ref["pop"] & ~ref["decided"].all(0)).any() else int(np.nonzero(ref["pop"])[0][0])
    for value in (-1e-30, np.nan, np.inf):
        c = SF.plane(colors).copy()
        c[px, 0] = value
        with pytest.raises(AssertionError, match="non-finite or negative"):
            SF.check_frame("tampered / " + name, SF._back(c), ref, verbose=False)


# ---- the two closed bounds on rays of their own kind ------------------------------------------------------------------------------------
N = 20000


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -4])
def test_own_sphere_bound_contains_binary32_s_far_root(scale):
    """rays that leave a sphere outward from a binary32 point of its surface (distance 0 .. a few ulps: binary32's own rounding of the
    point), radii 0.02 .. 60, at cosines down to 1e-3: the far root binary32 returns must not exceed own_sphere_upper, and where the
    running envelope decides the root against EPS the bound used -- the smaller of the two -- is the running one or smaller"""
    rng = np.random.default_rng(11)
    k = R.K.exact()
    rad = (10.0 ** rng.uniform(np.log10(0.3), np.log10(1000.0), N) * scale).astype(F)
    c = (rng.uniform(-100, 100, (N, 3)) * scale).astype(F)
    nrm = _units(rng, N)
    hp = (c.astype(D) + rad.astype(D)[:, None] * nrm).astype(F)
    cos = 10.0 ** rng.uniform(-3, 0, N)
    tang = np.cross(nrm, _units(rng, N))
    tang /= np.linalg.norm(tang, axis=1)[:, None]
    d = R.unit32((nrm * cos[:, None] + tang * np.sqrt(1 - cos * cos)[:, None]).astype(F))
    rays = np.concatenate([hp, d], 1)
    worst, used_closed = 0.0, 0
    for a in range(0, N, 2000):
        sl = slice(a, a + 2000)
        tab = np.concatenate([c[sl], (rad[sl] * rad[sl]).astype(F)[:, None]], 1)
        got, p = R.pairs32(rays[sl], tab), R.pairs64(rays[sl], tab, k)
        i = np.arange(len(tab))
        r2 = tab[:, 3].astype(D)
        delta = np.abs(np.linalg.norm(hp[sl].astype(D) - c[sl].astype(D), axis=1) - np.sqrt(r2))
        b = p["b"]
        m = np.linalg.norm(d[sl].astype(D), axis=1)
        upper = SF.own_sphere_upper(r2, delta, -(b.v[i, i] + b.e[i, i]), m, k)
        assert np.isfinite(upper).mean() > 0.99
        with np.errstate(all="ignore"):
            det32, b32 = got["det"][i, i], got["b"][i, i]
            t2 = (b32 + np.sqrt(det32)).astype(D)
        real = np.isfinite(upper) & (det32 >= 0)
        assert (t2[real] <= upper[real]).all(), ("the far root exceeds the closed bound", float((t2[real] - upper[real]).max()))
        worst = max(worst, float((t2[real] / upper[real]).max()))
        run_hi = p["t2"].v[i, i] + p["t2"].e[i, i]
        run_decides = p["decided"][i, i]
        used = np.minimum(upper, run_hi)
        assert (used[run_decides] <= run_hi[run_decides]).all()
        used_closed += int((upper < run_hi).sum())
    print("own sphere (scale %g): largest far root / closed bound %.3f; the closed bound is the smaller one on %d of %d rays" % (scale, worst, used_closed, N))


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -4])
def test_own_light_bound_contains_binary32_s_near_root(scale):
    """rays from a binary32 point towards a binary32 point of a light's surface, sd and len formed in binary32 as sample_light_drawn does:
    the near root binary32 returns for the light's own record must not fall below len by more than own_light_margin, at |wo| down to 1e-3"""
    rng = np.random.default_rng(12)
    k = R.K.exact()
    eps_s, _ = SF.norm_errors(k)
    rad = (rng.uniform(1.0, 12.0, N) * scale).astype(F)
    c = (rng.uniform(-80, 80, (N, 3)) * scale).astype(F)
    us = _units(rng, N)
    on = (c.astype(D) + rad.astype(D)[:, None] * us).astype(F)
    wo = -(10.0 ** rng.uniform(-3, 0, N))
    tang = np.cross(us, _units(rng, N))
    tang /= np.linalg.norm(tang, axis=1)[:, None]
    way = us * wo[:, None] + tang * np.sqrt(1 - wo * wo)[:, None]            # direction of travel: enters the light at `on`
    hp = (on.astype(D) - way * (rng.uniform(2.0, 150.0, N) * scale)[:, None]).astype(F)
    with np.errstate(all="ignore"):
        diff = (on - hp).astype(F)
        length = np.sqrt(R.dot32(diff, diff)).astype(F)
        sd = (diff * (F(1) / length)[:, None]).astype(F)
    rays = np.concatenate([hp, sd], 1)
    worst, decided = 0.0, 0
    for a in range(0, N, 2000):
        sl = slice(a, a + 2000)
        tab = np.concatenate([c[sl], (rad[sl] * rad[sl]).astype(F)[:, None]], 1)
        got = R.pairs32(rays[sl], tab)
        i = np.arange(len(tab))
        r2 = tab[:, 3].astype(D)
        # here the device's inputs are known exactly: Q, its distance from the surface, the slope and |sd|^2 in binary64
        q = hp[sl].astype(D) + length[sl].astype(D)[:, None] * sd[sl].astype(D)
        qc = q - c[sl].astype(D)
        delta = np.abs(np.linalg.norm(qc, axis=1) - np.sqrt(r2))
        g = np.abs((qc * sd[sl].astype(D)).sum(1))
        s2 = np.abs((sd[sl].astype(D) ** 2).sum(1) - 1.0)
        assert (s2 <= 2.1 * eps_s).all(), "|sd|^2 is further from 1 than the derivation allows"
        margin = SF.own_light_margin(r2, delta, g, length[sl].astype(D), s2, k)
        ok = np.isfinite(margin) & got["hit"][i, i]
        fall = length[sl].astype(D) - got["t"][i, i].astype(D)
        assert (fall[ok] <= margin[ok]).all(), ("the near root falls below len by more than the closed bound", float((fall[ok] - margin[ok]).max()))
        worst = max(worst, float((fall[ok] / margin[ok]).max()))
        decided += int((margin < R.EPS).sum())
    print("own light (scale %g): largest (len - t1) / closed bound %.3f; %d of %d rays decided against EPS" % (scale, worst, decided, N))


def test_e_div_is_one_rounding_in_exact_mode():
    rng = np.random.default_rng(13)
    a, b = R.log_uniform(rng, -20, 20, 4096), R.log_uniform(rng, -20, 20, 4096)
    q = SF.e_div(R.Err(a.astype(D)), R.Err(b.astype(D)), R.K.exact())
    assert (np.abs((a / b).astype(D) - q.v) <= q.e).all() and (q.e <= 1.01 * R.U * np.abs(q.v) + 2.0 ** -100).all()


def test_the_64_sphere_frame_reaches_the_rotated_loop_and_the_65_sphere_frame_cannot():
    """rt_trace_fast_w1 runs the rotated loop (the later light's shadow ray on the bounce ray's sweep, sweep_both) on the wavefronts whose
    8x8 tile has at most direct_max = 3 candidate spheres, and only on scenes of at most 64 records (the candidate masks' width).  The
    tiles' masks are the library's own host function: of random64's population enough pixels must lie in such tiles to meet the frame's
    floor of 500 decided answers by themselves; 65 records get no masks, so that frame's wavefronts all run the old loop (both lights
    through sweep_any)."""
    from test_tile_candidates import masks_of
    sph, cam, _, _ = SF.scene("random64")
    masks = masks_of(sph, cam, SF.W, SF.H)
    few = np.array([[bin(int(m)).count("1") <= 3 for m in row] for row in masks])
    ref = SF.reference("random64", False)
    gid = np.arange(SF.W * SF.H)
    in_few = few[(gid // SF.W) // 8, (gid % SF.W) // 8]
    decided = int((ref["decided"] & (ref["pop"] & in_few)[None, :]).sum())
    print("random64: %d of %d decided answers on tiles that run the rotated loop" % (decided, int((ref["decided"] & ref["pop"][None, :]).sum())))
    assert decided >= 500, decided
    assert len(SF.scene("random65")[0]) == 65
