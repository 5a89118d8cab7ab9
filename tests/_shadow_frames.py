"""Shadow frames: the any-hit decision and the light term of a whole render kernel for the shadow rays of its first diffuse hit, pixel
by pixel and light by light, against binary64 (tests/test_shadow_frames_cpu.py on the oracle, tests/test_gpu_fast_shadow.py on every
shipped rt_trace_fast_* instance).  numpy only; built from tests/_fast_reference.py (R) and the camera rays of tests/_first_hit.py.

THE TRICK.  The maker's geometry, scaled by 2^-4 (below), with its materials replaced:
  * ONE receiver: a sphere with c = (1, 1, 1), e = 0, DIFF;
  * two lights, e = (8, 0, 0) for the one that comes first in the table and (0, 0, 8) for the later one -- no_emission() reads x and z, so
    green carries nothing and must stay an exact zero;
  * every other record an occluder: DIFF, c = (0, 0, 0), e = 0.
A camera ray that hits an occluder multiplies the throughput by zero; one that hits the receiver samples both lights (two draws each,
whatever happens next: the stream replays on the host, R.mwc_word) and bounces.  The bounce ray leaves a convex sphere and cannot come back
to it; whatever else it meets is an occluder (throughput zero from there on: every later term is an exact 0 * finite), an emitter
(after_specular is false: nothing is added) or nothing.  So one pass leaves in a receiver pixel exactly  thr * ld = sum_j e_j k_j visible_j
with thr = 1 * 1: the red channel is 8 k_0 where the first light wanted a shadow ray and the any-hit sweep found no blocker, the blue
channel the same for the second light, and an exact zero otherwise.  8 is a power of two and the other light's term is 0 * k = 0, so a lit
channel is rt_div(numer, len * len) itself times 8, fused or not.

THE REFERENCE, per pixel: the camera ray with its envelope (R.shade64(0, ...)), R.pairs64 / R.scene64 for the first hit (with
_first_hit.behind_the_winner); the POPULATION is the pixels whose decided first hit is the receiver.  There hp = o + d t, nrm, dp, nl are
formed as R.Err, then per light in table order R.sample_light64 on those columns, R.pairs64(o_env=hp, d_env=sd), R.scene64 against
max_t = len - EPS WITH its envelope, and k = numer / len^2 with its envelope (e_div).

THE EXCLUSION RULE is R's: an answer (pixel, light) is compared only where every decision on its way is further from its threshold than
its envelope: the first hit, the side of the surface (dp against 0), wo <= 0, wi > 0, and every pair up to the first clear blocker.  A
condition on the reference alone.  At most 2 % of a frame's answers may be left out (R.cap), under K.exact() and under K.measured().

WHY THE SCENES ARE SCALED.  RT_EPS = 0.01 is an ABSOLUTE margin, and the running envelopes of a second-generation ray (its origin and its
direction are computed quantities) exceed it at the makers' scale for almost every ray.  Multiplying every position and radius, and the
camera, by 2^-4 is exact, shrinks every envelope 16-fold and leaves EPS where it is; the kernels are scale-free except for EPS, so the
decisions are the same code paths.  The camera stands close to the receiver (this module's choice, as _first_hit._nearer's).

TWO CLOSED BOUNDS replace the running envelope for two pairs of every shadow ray, where the running analysis treats as independent what
is one quantity.  Notation: u = 2^-24; the device evaluates b = op.d, det = b b - op.op + r2 (r2 the table's binary32 square, R = sqrt(r2)),
sq = sqrt(det), t1 = b - sq, t2 = b + sq, the roots of  phi(t) = t^2 - 2 b t + c0,  c0 = |op|^2 - r2  -- whatever |d| is.  Rounding alone
(inputs taken as the device has them) costs, by the rules of R's docstring with |op| <= M and |d| <= m:  eb = 4 u M m;
edet = u m^2 (24 M^2 + r2)  (the closed det bound with b^2 <= M^2 m^2);  |sqrt(det') - sqrt(det)| <= min(edet / sqrt(det_lo), sqrt(edet)) for
det >= det_lo;  the hardware root adds K_sqrt 2^-23 sqrt(M^2 m^2 + r2 + edet), the last sum u times its result.

  OWN SPHERE (own_sphere_upper).  The shadow ray leaves the receiver from hp, which lies within delta of the sphere's surface
  (delta = | |hp - c| - R | in binary64 plus the length of hp's envelope), outward: b < 0, |b| >= b_lo.  Then |c0| = | |op| - R | (|op| + R)
  <= delta (2 R + delta), and t1 t2 = c0 with |t1| = |b| + sq >= |b| gives
        |t2| <= delta (2 R + delta) / (|b| + sqrt(max(b_lo^2 - |c0|, 0)))  <=  (2 R delta + delta^2) / |b|.
  With M = R + delta the rounding terms above are added; a negative det (true or computed) is a miss, which is the same answer.  So the
  pair is decided -- no hit, t2 < EPS -- wherever that sum is below EPS, and the rule's "t2 against EPS" is this number against EPS.
  The running envelope of the same root is about 3.4 e_hp (1 + cos) / cos whatever the radius, because it does not know that hp came from
  this very sphere; the bound used is the smaller of the two (never wider than what it replaces).

  OWN LIGHT (own_light_margin).  sd and len are formed from diff = on - hp, on the sampled point: sd = diff inv, len = sqrt(diff.diff).
  The device's point Q = hp + len sd therefore lies within L eps_n of `on` (eps_n = 1.01 (eps_s + 3 u + K_sqrt 2^-23), eps_s = the
  relative error of inv plus 3 u: the dot product's 3 u halved, the product's u, rounded up; L >= len), `on` within the length of its
  envelope of c + r us with |us| = 1, and r within |r - R| of R: Q lies within delta of the light's surface, and | |sd|^2 - 1 | <= s2 = 2.1 eps_s.
  phi(len) = (|Q - c|^2 - r2) + (1 - |sd|^2) len^2, so |phi(len)| <= P = delta (2 R + delta) + s2 L^2;  phi'(len) / 2 = len - b
  = (Q - c).sd + (1 - |sd|^2) len, and (Q - c).sd = r wo up to (|Q - on|) |sd| + r |sd - sd64|: with g_lo a lower bound of r |wo| less
  those, |phi'(len)| / 2 >= h_lo = g_lo - s2 L, and its sign is wo's (negative: the ray enters the light there).  phi is convex with
  leading coefficient 1, so for t < len:  phi(t) >= phi(len) + phi'(len) (t - len) > 0  as soon as  len - t > P / (2 h_lo) = Delta.
  Both roots are therefore >= len - Delta: the light's own near root cannot fall below len - EPS -- the light cannot block its own
  shadow ray -- wherever  Delta + rounding (M = L + R + delta, det_lo = h_lo^2 - P) + u L (the rounding of len - EPS)  is below EPS.
  About delta / |wo| plus the rounding terms.  The running analysis takes t1 and len for independent quantities and at grazing samples
  its envelope grows like 1 / |wo| times the envelope of hp.

VACUITY GUARDS (conditions on the reference, chosen with the scenes): per frame at least 500 decided answers; of each light's decided
answers at least 10 % lit and at least 10 % dark because a sphere blocks (not merely because the light is behind the surface or the
sample on its far side); the blockers at least min(4, n - 3) distinct records.

DECODING.  A population pixel's channels are compared as they are (read_colors' plane, pass 0: fold_sample returns the sample).  A
non-finite or negative channel there, or a green channel that is not zero, is a failure, never an exclusion; -0 is a zero.  Pixels whose
decided first hit is an occluder, or nothing, must be three exact zeros (a by-product: it costs nothing)."""
import functools
import os

import numpy as np

import _fast_reference as R
import _first_hit as FH
from raytracing_simple_amd import api, host, scenes

F, D = np.float32, np.float64
W, H = 96, 64
CHUNK = 256
SCALE = 2.0 ** -4
LIGHT_E = 8.0
RECORDS = os.path.join(R.ROOT, "profiles", "r28_shadow_frames.jsonl")


# ---- the two closed bounds (module docstring) -----------------------------------------------------------------------------------------
def _rounding(M, m, r2, det_lo, k):
    """rounding alone of one root b -+ sqrt(det) for |op| <= M, |d| <= m, det >= det_lo (module docstring) -> (its bound, edet)"""
    with np.errstate(all="ignore"):
        eb = 4.0 * R.U * M * m
        edet = R.U * m * m * (24.0 * M * M + r2)
        e_sq = np.where(det_lo > 0, np.minimum(edet / np.sqrt(np.where(det_lo > 0, det_lo, 1.0)), np.sqrt(edet)), np.sqrt(edet))
        sq_hi = np.sqrt(M * M * m * m + r2 + edet)
        return eb + e_sq + k.sqrt * 2.0 ** -23 * sq_hi + R.U * (M * m + sq_hi) + 4 * R.TINY, edet


def own_sphere_upper(r2, delta, b_lo, m, k):
    """Upper bound of the far root t2 the device returns for the sphere (table square r2) a ray leaves outward: delta bounds the distance
    of its origin from the surface, b_lo > 0 bounds |b| from below (b < 0), m >= |d|.  inf where b_lo <= 0."""
    with np.errstate(all="ignore"):
        rad = np.sqrt(r2)
        c0 = delta * (2.0 * rad + delta)
        det_lo = b_lo * b_lo - c0
        bound = c0 / (b_lo + np.sqrt(np.maximum(det_lo, 0.0)))
        rounding, _ = _rounding(rad + delta, m, r2, det_lo, k)
        return np.where(b_lo > 0, bound + rounding, np.inf)


def own_light_margin(r2, delta, g_lo, length, s2, k):
    """How far below len the device's near root of the sampled light's own record can fall, rounding and the rounding of len - EPS
    included: delta bounds the distance of Q = hp + len sd from the light's surface, g_lo bounds |(Q - c).sd| from below, length >= len,
    s2 >= | |sd|^2 - 1 |.  inf where the slope is not clear of zero."""
    with np.errstate(all="ignore"):
        rad = np.sqrt(r2)
        P = delta * (2.0 * rad + delta) + s2 * length * length
        h_lo = g_lo - s2 * length
        gap = P / (2.0 * np.where(h_lo > 0, h_lo, 1.0))
        rounding, _ = _rounding(length * np.sqrt(1.0 + s2) + rad + delta, np.sqrt(1.0 + s2), r2, h_lo * h_lo - P, k)
        return np.where(h_lo > 0, gap + rounding + R.U * length, np.inf)


def norm_errors(k):
    """(eps_s, eps_n) of the module docstring for the mode k describes"""
    inv = k.rsq if k.fast else (k.sqrt + k.rcp)
    eps_s = inv * 2.0 ** -23 + 3.0 * R.U
    return eps_s, 1.01 * (eps_s + 3.0 * R.U + k.sqrt * 2.0 ** -23)


def e_div(a, b, k):
    """rt_div: a * v_rcp_f32(b) in fast mode, the correctly rounded quotient otherwise (one rounding)"""
    if k.fast:
        return a * b.rcp(k.rcp)
    return a * b.rcp(0.0)


def _length(cols):
    return np.sqrt(sum(c * c for c in cols))


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
def _many(n):
    return lambda: FH._many_spheres(n)


# name -> (maker, receiver, the two lights (record indices), radius given to the lights (None: the maker's), camera offset from the
# receiver's centre in units of its radius; the camera looks at that centre).  How they were chosen, and what was tried: profiles/HISTORY.md, r28.
SCENES = {
    "demo_plus16": (lambda: scenes.demo_plus(16), 11, (2, 15), None, (-2.33, 1.77, 0.66)),
    "random64": (lambda: scenes.random_spheres(64), 11, (34, 15), (6.0, 6.0), (-2.51, 1.46, -0.76)),
    "random65": (lambda: scenes.random_spheres(65), 11, (34, 15), (6.0, 6.0), (-2.51, 1.46, -0.76)),
    "random256": (lambda: scenes.random_spheres(256), 53, (160, 183), (6.0, 6.0), (2.57, 1.55, -0.02)),
    "many2000": (_many(2000), 1533, (280, 1162), (2.0, 2.0), (-2.14, 0.19, 3.95)),
    "many5000": (_many(5000), 4553, (1122, 737), None, (2.98, 0.3, 0.23)),
}


def shadow_scene(spheres, receiver, lights, light_rad=None):
    """the maker's geometry times SCALE with the materials of the module docstring"""
    sph = api.as_spheres(spheres).copy()
    assert len(set(lights)) == 2 and receiver not in lights
    sph["p"] = (sph["p"] * F(SCALE)).astype(F)
    sph["rad"] = (sph["rad"] * F(SCALE)).astype(F)
    sph["e"], sph["c"], sph["refl"] = 0, 0, api.DIFF
    sph["c"][receiver] = 1
    first, second = sorted(lights)
    sph["e"][first] = (LIGHT_E, 0, 0)
    sph["e"][second] = (0, 0, LIGHT_E)
    if light_rad is not None:
        for j, r in zip(lights, light_rad):
            if r is not None:
                sph["rad"][j] = F(r * SCALE)
    return sph


def make(spec):
    """-> (records, camera, receiver, (first light, second light))"""
    maker, receiver, lights, light_rad, offset = spec
    sph0 = api.as_spheres(maker()[0])
    sph = shadow_scene(sph0, receiver, lights, light_rad)
    c, r = sph["p"][receiver].astype(D), float(sph["rad"][receiver])
    orig = tuple(float(F(v)) for v in c + r * np.asarray(offset, D))
    cam = host.compute_camera(orig, tuple(float(v) for v in c), W, H)
    return sph, cam, receiver, tuple(sorted(lights))


@functools.lru_cache(maxsize=None)
def scene(name):
    return make(SCENES[name])


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _sub(cols, sel):
    return [R.Err(c.v[sel], c.e[sel]) for c in cols]


def reference_of(sph, cam, receiver, lights, k):
    """binary64's answers for one pass of the default stream (gid order: y * W + x).  -> dict:
    first-hit stage: id, any_hit, id_decided, pop (population);
    per light [2, N]: decided, lit, blocker (record index of binary64's first blocker, -1 none), wanted, val, env (8 k and its envelope),
    own_sphere / own_light [2, N]: 0 not needed, 1 decided by the running envelope, 2 by the closed bound only, 3 undecided."""
    tab = R.table_of(sph)
    n, n_px = len(sph), W * H
    seeds = api.stream_seeds(0, 2 * n_px)
    rec = np.zeros((n_px, 16), F)
    words = rec.view(np.uint32)
    words[:, 0], words[:, 1] = seeds[0::2], seeds[1::2]
    gid = np.arange(n_px)
    items, _, _ = R.shade64(0, rec, {"cam": np.asarray(cam, F), "w": W, "h": H, "px": gid % W, "py": gid // W}, k)
    o, d = items[1][2], items[2][2]
    s0, s1, _ = R.mwc_word(words[:, 0].copy(), words[:, 1].copy())
    s0, s1, _ = R.mwc_word(s0, s1)                                        # the camera's two draws
    draws = []
    for _ in lights:
        s0, s1, f1 = R.mwc_word(s0, s1)
        s0, s1, f2 = R.mwc_word(s0, s1)
        draws.append((3.0 - f1.astype(D), (f2.astype(D) * 0.5 - 1.0).astype(F)))       # zc, u2: exact (2^-22 / 2^-23 grids)
    eps_s, eps_n = norm_errors(k)
    s2 = 2.1 * eps_s
    out = {"id": np.zeros(n_px, np.int64), "any_hit": np.zeros(n_px, bool), "id_decided": np.zeros(n_px, bool), "pop": np.zeros(n_px, bool),
           "decided": np.zeros((2, n_px), bool), "lit": np.zeros((2, n_px), bool), "wanted": np.zeros((2, n_px), bool),
           "blocker": np.full((2, n_px), -1, np.int64), "val": np.zeros((2, n_px), D), "env": np.full((2, n_px), np.inf, D),
           "own_sphere": np.zeros((2, n_px), np.int8), "own_light": np.zeros((2, n_px), np.int8), "n": n, "receiver": receiver, "lights": lights}
    rc, r2r = [R.Err(np.full(1, float(tab[receiver, j]))) for j in range(3)], float(tab[receiver, 3])
    with np.errstate(all="ignore"):
        for a in range(0, n_px, CHUNK):
            sl = slice(a, min(a + CHUNK, n_px))
            oc, dc = _sub(o, sl), _sub(d, sl)
            p = FH.behind_the_winner(R.pairs64(None, tab, k, oc, dc), k)
            s = R.scene64(p, np.full(len(oc[0].v), R.T_NONE, F))
            rows, win = np.arange(len(oc[0].v)), s["id"]
            out["id"][sl], out["any_hit"][sl], out["id_decided"][sl] = win, s["any_hit"], s["id_decided"]
            pop = s["id_decided"] & s["any_hit"] & (win == receiver) & p["t_decided"][rows, win]
            out["pop"][sl] = pop
            if not pop.any():
                continue
            at = a + np.nonzero(pop)[0]
            oc, dc = _sub(oc, pop), _sub(dc, pop)
            t = R.Err(p["t"][rows, win][pop], p["t_env"][rows, win][pop])
            hp = [oc[j] + dc[j] * t for j in range(3)]
            nrm = R.e_unit([hp[j] - rc[j] for j in range(3)], k)
            dp = R.e_dot(nrm, dc)
            side = np.abs(dp.v) > dp.e
            sgn = -np.sign(dp.v)
            nl = [c.exact_scale(1.0) * R.Err(sgn) for c in nrm]
            hp_env = _length([c.e for c in hp])
            delta_r = np.abs(_length([hp[j].v - rc[j].v for j in range(3)]) - np.sqrt(r2r)) + hp_env
            for li, light in enumerate(lights):
                zc, u2 = draws[li]
                q = R.sample_light64(R.Err(zc[at]), u2[at], [R.Err(np.full(1, float(tab[light, j]))) for j in range(3)],
                                     np.full(1, sph["rad"][light], F), np.full(1, F(4) * F(3.14159265358979323846) * sph["rad"][light] * sph["rad"][light], F),
                                     hp, nl, k)
                wo, wi, sd, length = q["wo"], q["wi"], q["sd"], q["len"]
                wo_clear, wi_clear = np.abs(wo.v) > wo.e, np.abs(wi.v) > wi.e
                wanted = q["want"]
                # not wanted: either compare that says so is clear of its tie; wanted: both are
                dec = side & np.where(wanted, wo_clear & wi_clear, (wo_clear & (wo.v > 0)) | (wi_clear & (wi.v <= 0)))
                p2 = R.pairs64(None, tab, k, hp, sd)
                m = 1.0 + eps_s
                # -- the receiver's own pair
                b = p2["b"]
                run_hi = p2["t2"].v[:, receiver] + p2["t2"].e[:, receiver]
                closed_hi = own_sphere_upper(r2r, delta_r, -(b.v[:, receiver] + b.e[:, receiver]), m, k)
                run_ok = p2["decided"][:, receiver] & (~p2["hit"][:, receiver] | p2["t_decided"][:, receiver])
                closed_ok = np.minimum(closed_hi, np.where(np.isfinite(run_hi), run_hi, np.inf)) < R.EPS
                p2["hit"][:, receiver] &= ~closed_ok
                p2["decided"][:, receiver] |= closed_ok
                p2["t_decided"][:, receiver] &= ~closed_ok
                own_s = np.where(run_ok, 1, np.where(closed_ok, 2, 3))
                # -- the sampled light's own pair
                r2l, rl = float(tab[light, 3]), float(sph["rad"][light])
                L = length.v + length.e
                on_env = _length([c.e for c in q["on"]])
                d_q = on_env + L * eps_n
                delta_l = d_q + abs(rl - np.sqrt(r2l))
                g_lo = rl * np.abs(wo.v) - d_q * m - rl * _length([c.e for c in sd])
                margin = own_light_margin(r2l, delta_l, g_lo, L, s2, k)
                run_ok_l = p2["decided"][:, light] & (~p2["hit"][:, light] | (p2["t_decided"][:, light] & (
                    np.abs(p2["t"][:, light] - (length.v - R.EPS)) > p2["t_env"][:, light] + length.e + R.U * L)))
                closed_ok_l = (wo.v < 0) & (margin < R.EPS) & (length.v - length.e - margin > 2 * R.EPS)
                own_l = np.where(run_ok_l, 1, np.where(closed_ok_l, 2, 3))
                take = closed_ok_l & ~run_ok_l                    # (never wider than what it replaces: the running envelope stands where it decides)
                p2["hit"][:, light] &= ~take                      # cannot block: for the sweep against max_t the record is not there
                p2["decided"][:, light] |= take
                p2["t_decided"][:, light] &= ~take
                max_t = length - R.EPS
                s2nd = R.scene64(p2, max_t)
                blocked = s2nd["first"] < n
                dec &= ~wanted | s2nd["first_decided"]
                kk = e_div(q["numer"], length * length, k)
                lit = wanted & ~blocked
                out["decided"][li, at], out["lit"][li, at], out["wanted"][li, at] = dec, lit, wanted
                out["blocker"][li, at] = np.where(wanted & blocked, s2nd["first"], -1)
                out["val"][li, at], out["env"][li, at] = LIGHT_E * kk.v, LIGHT_E * kk.e
                out["own_sphere"][li, at] = np.where(wanted, own_s, 0)
                out["own_light"][li, at] = np.where(wanted, own_l, 0)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, fast):
    k = R.K.measured() if fast else R.K.exact()
    assert k is not None
    return reference_of(*scene(name), k)


def figures(ref):
    """the reference's own counts: what the cap and the vacuity guards are about"""
    pop = ref["pop"]
    total = 2 * int(pop.sum())
    dec = ref["decided"] & pop[None, :]
    lit = dec & ref["lit"]
    blk = dec & (ref["blocker"] >= 0)
    return {"pixels": int(pop.size), "population": int(pop.sum()), "answers": total, "decided": int(dec.sum()), "excluded": total - int(dec.sum()),
            "lit": [int(v) for v in lit.sum(1)], "dark_by_blocker": [int(v) for v in blk.sum(1)], "decided_per_light": [int(v) for v in dec.sum(1)],
            "blockers": sorted(int(v) for v in np.unique(ref["blocker"][blk])),
            "own_sphere_closed_only": int(((ref["own_sphere"] == 2) & pop[None, :]).sum()), "own_light_closed_only": int(((ref["own_light"] == 2) & pop[None, :]).sum())}


def check_reference(name, ref, verbose=True):
    """The cap and the vacuity guards: conditions on the reference alone.  -> figures(ref)"""
    f = figures(ref)
    if verbose:
        print("%-40s population %5d  answers %5d  excluded %4d (%.2f %%)  lit %s  dark by blocker %s of %s  blockers %s  closed bound alone: sphere %d light %d" % (
            name, f["population"], f["answers"], f["excluded"], 100.0 * f["excluded"] / max(f["answers"], 1), f["lit"], f["dark_by_blocker"],
            f["decided_per_light"], f["blockers"][:8], f["own_sphere_closed_only"], f["own_light_closed_only"]))
    R.cap(name + " shadow answers", f["excluded"], f["answers"])
    assert f["decided"] >= 500, (name, "vacuous: fewer than 500 decided answers", f)
    for j in range(2):
        assert 10 * f["lit"][j] >= f["decided_per_light"][j], (name, "vacuous: light %d is lit in fewer than 10 %% of its decided answers" % j, f)
        assert 10 * f["dark_by_blocker"][j] >= f["decided_per_light"][j], (name, "vacuous: light %d is blocked by a sphere in fewer than 10 %% of its decided answers" % j, f)
    assert len(f["blockers"]) >= min(4, ref["n"] - 3), (name, "vacuous: too few distinct blockers", f)
    return f


def plane(colors):
    """read_colors' layout (row h - 1 - y) -> [N, 3] in gid order"""
    return np.ascontiguousarray(colors, F).reshape(H, W, 3)[::-1].reshape(-1, 3)


CHANNEL = (0, 2)


def check_frame(name, colors, ref, verbose=True):
    """The assertions of a shadow frame against ref = reference(...).  -> {counts, the largest observed / bound of 8 k}"""
    c = plane(colors)
    pop = ref["pop"]
    f = check_reference(name, ref, verbose=False)
    with np.errstate(all="ignore"):
        bad = pop & ~(np.isfinite(c).all(1) & (c >= 0).all(1))
        assert not bad.any(), (name, "a non-finite or negative channel on a receiver pixel", np.nonzero(bad)[0][:4].tolist(), c[bad][:4].tolist())
        bad = pop & (c[:, 1] != 0)
        assert not bad.any(), (name, "green is not zero on a receiver pixel", np.nonzero(bad)[0][:4].tolist(), c[bad][:4].tolist())
        black = ref["id_decided"] & (~ref["any_hit"] | ((ref["id"] != ref["receiver"]) & ~np.isin(ref["id"], ref["lights"])))
        bad = black & (c != 0).any(1)
        assert not bad.any(), (name, "an occluder or the sky is not black", np.nonzero(bad)[0][:4].tolist(), c[bad][:4].tolist())
        worst = 0.0
        for j in range(2):
            got = c[:, CHANNEL[j]].astype(D)
            dec = ref["decided"][j] & pop
            dark_lit = dec & ref["lit"][j] & (got == 0)
            assert not dark_lit.any(), (name, "light %d: dark where binary64 finds no blocker (pixel, binary64's 8 k)" % j, np.nonzero(dark_lit)[0][:4].tolist(),
                                        ref["val"][j][dark_lit][:4].tolist())
            lit_dark = dec & ~ref["lit"][j] & (got != 0)
            assert not lit_dark.any(), (name, "light %d: lit where binary64 is dark (pixel, blocker or -1, got)" % j, np.nonzero(lit_dark)[0][:4].tolist(),
                                        ref["blocker"][j][lit_dark][:4].tolist(), got[lit_dark][:4].tolist())
            sel = dec & ref["lit"][j]
            ratio = np.where(sel, np.abs(got - ref["val"][j]) / ref["env"][j], 0.0)
            assert not np.isnan(ratio).any() and ratio.max() <= 1.0, (name, "light %d: a lit channel outside the envelope of 8 k (ratio, pixel)" % j, float(ratio.max()),
                                                                      int(np.nanargmax(ratio)))
            worst = max(worst, float(ratio.max()))
    out = dict(f, scene=name, ratio=worst)
    if verbose:
        print("%-44s population %5d  answers %5d  excluded %4d (%.2f %%)  lit %s  dark by blocker %s  blockers %d   8 k observed / bound %.3f" % (
            name, f["population"], f["answers"], f["excluded"], 100.0 * f["excluded"] / max(f["answers"], 1), f["lit"], f["dark_by_blocker"], len(f["blockers"]), worst))
    return out


# ---- tampered frames (tests/test_shadow_frames_cpu.py) ------------------------------------------------------------------------------------------
def _pick(sel, share, seed):
    idx = np.nonzero(sel)[0]
    return np.random.default_rng(seed).choice(idx, max(1, int(round(share * len(idx)))), replace=False)


def _back(c):
    return c.reshape(H, W, 3)[::-1].reshape(-1).copy()


def tamper_lit_to_zero(colors, ref, share=0.01, seed=1):
    c = plane(colors).copy()
    for j in range(2):
        c[_pick(ref["decided"][j] & ref["pop"] & ref["lit"][j], share, seed + j), CHANNEL[j]] = 0
    return _back(c)


def tamper_dark_to_lit(colors, ref, share=0.01, seed=1):
    c = plane(colors).copy()
    for j in range(2):
        at = _pick(ref["decided"][j] & ref["pop"] & ~ref["lit"][j] & ref["wanted"][j], share, seed + j)
        c[at, CHANNEL[j]] = ref["val"][j][at].astype(F)
    return _back(c)


def tamper_scale(colors, j, factor=1.01):
    c = plane(colors).copy()
    c[:, CHANNEL[j]] = (c[:, CHANNEL[j]] * F(factor)).astype(F)
    return _back(c)


def tamper_negative_zero(colors):
    c = plane(colors).copy()
    c[c == 0] = F(-0.0)
    return _back(c)


# ---- rendering --------------------------------------------------------------------------------------------------------------------------
def render(name, diag=False, knobs=(), fast=True):
    """One pass over scene `name` -> (colour plane, rt_last_kernel, seeds, stats)"""
    sph, cam, _, _ = scene(name)
    with api.RtContext(W, H, diag=diag or bool(knobs)) as ctx:
        for setter, args in knobs:
            ctx._check(getattr(ctx._lib, setter)(ctx._h, *args))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.set_mode(api.RT_MODE_FAST if fast else api.RT_MODE_PARITY)
        ctx.render_pass(1)
        return ctx.read_colors(), ctx.last_kernel, ctx.read_seeds(), ctx.stats()
