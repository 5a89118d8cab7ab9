"""What fast mode's arithmetic is held to: binary64 references, binary32 restatements, error envelopes and the input
families of tests/test_fast_reference_cpu.py, test_gpu_fast_blocks.py and test_gpu_fast_rays.py.  numpy only.

The probe (tests/fast_probe.hip) runs the library's own inline functions (csrc/rt_trace.inc.h, included unchanged)
one lane per input, built twice: the FAST arm with rt_kernel_fast.hip's flags and a CONTROL arm with parity's.  The
control arm must equal the restatements here bit for bit; only then do the fast arm's numbers mean anything.

THE LIMIT.  -ffp-contract=fast fuses whatever multiply and add end up next to each other, so the same source function
can compile to different roundings in the probe and in each of the shipped rt_trace_fast_* kernels.  The probe
therefore holds the SOURCE FUNCTIONS UNDER THE FAST FLAGS to envelopes that are valid for ANY fusing; it does not hold
the shipped machine code.  The shipped kernels' own fusing is seen by tests/test_gpu_fast_bias.py and the PSNR gates of
tests/test_gpu_parity.py, and -- for the closest-hit decision of camera rays, ray by ray -- by the first-hit frames of
tests/test_gpu_fast_first_hit.py (tests/_first_hit.py): every shipped rt_trace_fast_* instance renders one pass of a scene whose
spheres are all emitters that carry their own index, and hit or miss, the winner and |n.d| of every pixel are held to pairs64 /
scene64 on the camera ray formed in binary64 with its envelope (pairs64's o_env / d_env).

REFERENCES.  Every binary64 reference is fed the very binary32 inputs the device gets (directions are normalised in
binary32 on the host and those floats go to both), and is evaluated in binary64, whose own rounding (2^-53 per
operation) is 2^-29 of the binary32 unit roundoff the envelopes are made of.

ENVELOPES: a running error analysis.  `Err` carries, for every intermediate, the binary64 value v and a bound e on
|device value - v|.  With u = 2^-24 and the standard model fl(x op y) = (x op y)(1 + d), |d| <= u:
    x + y:   e = ex + ey + u (|v| + ex + ey)            x * y:   p = |x| ey + |y| ex + ex ey,  e = p + u (|v| + p)
A fused multiply-add rounds once where the separate operations round twice, so these bounds hold however the
compiler contracts -- which is what makes them valid for the probe and for every shipped instance alike.  The hardware
approximations are K ulps from the exact function of their (already inexact) operand, and an ulp of y is at most
2^-23 |y|:
    sqrt:    p = min(ex / sqrt(x), sqrt(ex))  (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt|a - b|),   e = p + K 2^-23 (|v| + p)
    rsq:     p = ex / (2 (x - ex)^(3/2)),   rcp: p = ex / (|x| (|x| - ex))   (mean value theorem on the interval), same K term
K = 0.5 is a correctly rounded operation (the CPU tests and the control arm); for v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 the
guides at hand state no accuracy, so K is MEASURED on the device against binary64 (profiles/r20_fast_blocks.jsonl) and the
tests use twice the observed maximum.  Every bound gets 2^-149 added per operation (a subnormal result rounds absolutely).

det.  hit_pre forms op = c - o, b = (op.x d.x + op.y d.y) + op.z d.z, det = (b b - op.op) + r^2.  Running the rules
above: op_k carries u |op_k|, each product 2u |op_k d_k|, the two sums u each: eb <= 4u S1 with S1 = sum |op_k d_k|;
b b carries 2 |b| eb + u b^2, op.op carries 5u |op|^2, the last two sums u |b^2 - |op|^2| and u |det|.  With
S1 <= |op| |d| and 2 |b| |op| <= b^2 + |op|^2 this is at most 12 * 2^-24 (b^2 + |op|^2) + 2^-24 r^2 for |d| = 1 -- the
derivation of csrc/rt_candidates.h plus the r^2 term; |d| != 1 enters through S1, which the running form keeps.  The
tests use the running form (tighter, and right for any |d|); the CPU test asserts it never exceeds the closed one.

t.  sq = sqrt(det) carries edet / sqrt(det) + K_sqrt 2^-23 sq, the roots b -+ sq carry eb + esq + u |t|: the envelope
grows like edet / (2 sqrt(det)) towards det = 0, so it is used only where det > edet.

THE EXCLUSION RULE.  A decision (hit or miss; which root; which sphere wins; blocked or not) is compared only where the
binary64 quantity it depends on is further from its threshold than that quantity's envelope: |det| > edet,
|t2 - EPS| > et2, |t1 - EPS| > et1, the winner's lead over every other candidate larger than both envelopes together.
That is a condition on the reference, never on what the code under test returned.  See `cap()` for the 2 % rule.

NOT REACHED by the probe, and why: everything that is open-coded in the kernel bodies rather than a function -- the
refraction direction and the Fresnel terms (rt_trace.inc.h, the REFR branch), the throughput / radiance updates, the
Russian-roulette compare itself, fold_sample's table read (it needs the workgroup's LDS table), coop_any (it needs a
whole wavefront's pending rays and its LDS slots).  The hierarchy walk (rt_walk.inc.h, kernel state throughout) is not reached by
THIS probe either, but its source under the fast flags is held ray by ray, closest-hit and shadow rays, by tests/walk_probe.hip
(rt_walk.inc.h's own rays kernel, tests/test_gpu_fast_walk.py, tests/_walk_probe.py); the rotated candidate loop of
RT_OPT_DIRECT_CAMERA (it calls hit_pre / hit_roots, which ARE probed, on a kernel-held list) and the walk as the shipped instances
compile it are held for camera rays by the first-hit frames.  The shadow rays of the shipped kernels -- sweep_any, coop_any's shared
decisions, sweep_both, the walk's any-hit in its three table placements, and rt_div(numer, len * len) -- are held pixel by pixel and
light by light by the shadow frames (tests/_shadow_frames.py, tests/test_gpu_fast_shadow.py: one white receiver, a red and a blue light,
black occluders; sample_light64 below and scene64's max_t with an envelope are theirs), for the shadow rays of the FIRST diffuse hit.
STILL OPEN: the REFR branch, and paths beyond the first diffuse hit (the bounce ray's own hit and everything after it).
camera_direction, sample_light and next_random* take the generator's state by reference and are called with a state
per lane; the host replays the generator exactly (integers).  The reflected direction is one open-coded expression,
d - nrm * (2 dp); the probe restates that expression from the library's sub / scale."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -149
EPS = float(F(0.01))                    # RT_EPS
T_NONE = F(1e20)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = os.path.join(ROOT, "profiles", "r20_fast_blocks.jsonl")

OPS = {"sincos": 0, "gamma": 1, "to_int": 2, "rcp": 3, "div": 4, "sqrt": 5, "sqrt_unit": 6, "sqrt_det": 7, "sqrt_and_rcp": 8, "unit": 9}


# ---- the probe ----------------------------------------------------------------------------------------------------
def build_probe(out_dir, fast, source="fast_probe"):
    """tests/<source>.hip (fast_probe, walk_probe) -> a shared library in out_dir; the fast arm with rt_kernel_fast.hip's flags, the
    control arm with parity's."""
    from raytracing_simple_amd import _build
    extra = dict(_build.UNITS)["rt_kernel_fast.hip" if fast else "rt_kernel_parity.hip"]
    assert extra == (["-ffp-contract=fast"] if fast else ["-ffp-contract=off"]), extra
    so = os.path.join(str(out_dir), "lib%s_%s.so" % (source, "fast" if fast else "control"))
    cmd = [_build.hipcc()] + _build.COMMON + extra + ["-DRT_FAST=%d" % (1 if fast else 0), "-I" + _build.CSRC, "-shared",
                                                      os.path.join(ROOT, "tests", source + ".hip"), "-o", so]
    subprocess.run(cmd, check=True, capture_output=True)
    return so


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Probe:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.fast = bool(self.lib.probe_is_fast())
        for name in ("probe_eval", "probe_pairs", "probe_scene", "probe_shade"):
            getattr(self.lib, name).restype = C.c_int

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: HIP error %d" % (what, rc))

    def eval(self, op, a, b=None):
        """-> (r0, r1): r1 only for 'sincos' (cos) and 'sqrt_and_rcp' (the reciprocal); 'unit' takes and returns [n, 3]"""
        a = np.ascontiguousarray(a, F)
        n = len(a)
        b = np.ascontiguousarray(b, F) if b is not None else np.zeros(1, F)
        r0, r1 = np.zeros_like(a), np.zeros(n, F)
        self._ok(self.lib.probe_eval(OPS[op], _p(a), _p(b), _p(r0), _p(r1), C.c_size_t(n)), "probe_eval")
        return r0, r1

    def pairs(self, rays, table):
        """-> dict of [R, S] arrays: b, det, t (hit_roots), hit (bool), t_post (hit_post)"""
        rays, table = np.ascontiguousarray(rays[:, :6], F), np.ascontiguousarray(table, F)
        out = np.zeros((len(rays), len(table), 5), F)
        self._ok(self.lib.probe_pairs(_p(rays), C.c_size_t(len(rays)), _p(table), C.c_size_t(len(table)), _p(out)), "probe_pairs")
        return {"b": out[..., 0], "det": out[..., 1], "t": out[..., 2], "hit": out[..., 3] != 0, "t_post": out[..., 4]}

    def scene(self, rays, table):
        """rays [R, 7] = o, d, max_t -> dict: t (float32), id, first"""
        rays, table = np.ascontiguousarray(rays, F), np.ascontiguousarray(table, F)
        out = np.zeros((len(rays), 3), np.uint32)
        self._ok(self.lib.probe_scene(_p(rays), C.c_size_t(len(rays)), _p(table), C.c_uint(len(table)), _p(out)), "probe_scene")
        return {"t": out[:, 0].copy().view(F), "id": out[:, 1].astype(np.int64), "first": out[:, 2].astype(np.int64)}

    def shade(self, what, rec, cam=None):
        rec = np.ascontiguousarray(rec, F)
        assert rec.shape[1] == 16
        cam = np.ascontiguousarray(cam, F) if cam is not None else np.zeros(14, F)
        out = np.zeros((len(rec), 12), F)
        self._ok(self.lib.probe_shade(what, _p(rec), _p(cam), _p(out), C.c_size_t(len(rec))), "probe_shade")
        return out


# ---- measured constants ---------------------------------------------------------------------------------------------
def records():
    """{op: record} of profiles/r20_fast_blocks.jsonl ({} where it does not exist yet)"""
    if not os.path.exists(RECORDS):
        return {}
    return {r["op"]: r for r in (json.loads(line) for line in open(RECORDS) if line.strip())}


class K:
    """Accuracy of the elementary operations, in ulps (sin_abs: absolute).  K.exact(): correctly rounded binary32 -- parity mode, the
    oracle, the restatements.  K.measured(): twice what profiles/r20_fast_blocks.jsonl observed on the device; None before that visit."""

    def __init__(self, fast, sqrt, rcp, rsq, sin_abs):
        self.fast, self.sqrt, self.rcp, self.rsq, self.sin_abs = fast, sqrt, rcp, rsq, sin_abs

    @classmethod
    def exact(cls):
        # sin / cos of parity mode: the argument is fl(fl(2 pi) u): RT_PI is off by 2.8e-8 relative, the product by 2^-24, together
        # 8.8e-8 * 2 pi = 5.5e-7 absolute at most, plus the rounding of the result (2^-24): below 11 * 2^-24
        return cls(False, 0.5, 0.5, None, 11 * U)

    @classmethod
    def measured(cls):
        r = records()
        need = ("v_sqrt_f32", "v_rcp_f32", "v_rsq_f32", "v_sin_f32", "v_cos_f32")
        if any(k not in r for k in need):
            return None
        return cls(True, 2 * r["v_sqrt_f32"]["observed_max"], 2 * r["v_rcp_f32"]["observed_max"], 2 * r["v_rsq_f32"]["observed_max"],
                   2 * max(r["v_sin_f32"]["observed_max"], r["v_cos_f32"]["observed_max"]))


def ulp_error(got, exact):
    """|got - exact| in ulps of the binary32 neighbourhood of `exact` (binary64 array)"""
    with np.errstate(all="ignore"):
        return np.abs(got.astype(D) - exact) / np.spacing(np.abs(exact).astype(F)).astype(D)


# ---- running error ------------------------------------------------------------------------------------------------
class Err:
    """binary64 value v of an intermediate and a bound e on |device value - v| (module docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, D)
        self.e = np.broadcast_to(np.asarray(e, D), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _round(self, v, p, half_ulps=1.0):
        return Err(v, p + half_ulps * U * (np.abs(v) + p) + TINY)

    def __add__(self, o):
        o = Err.of(o)
        return self._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Err.of(o)
        return self._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = Err.of(o)
        return self._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __neg__(self):
        return Err(-self.v, self.e)

    def exact_scale(self, k):
        """times a power of two or a sign: no rounding"""
        return Err(self.v * k, self.e * abs(k))

    def sqrt(self, ulps):
        with np.errstate(all="ignore"):
            v = np.sqrt(np.maximum(self.v, 0.0))
            p = np.where(self.v > 0, np.minimum(self.e / np.where(v > 0, v, 1.0), np.sqrt(self.e)), np.sqrt(self.e))
        return self._round(v, p, 2 * ulps)

    def rsq(self, ulps):
        with np.errstate(all="ignore"):
            lo = self.v - self.e
            v = 1.0 / np.sqrt(self.v)
            p = np.where(lo > 0, self.e / (2.0 * np.where(lo > 0, lo, 1.0) ** 1.5), np.inf)
        return self._round(v, p, 2 * ulps)

    def rcp(self, ulps):
        with np.errstate(all="ignore"):
            lo = np.abs(self.v) - self.e
            v = 1.0 / self.v
            p = np.where(lo > 0, self.e / (np.abs(self.v) * np.where(lo > 0, lo, 1.0)), np.inf)
        return self._round(v, p, 2 * ulps)


def e_sqrt_and_rcp(dd, k):
    """-> (root, reciprocal root) as sqrt_and_rcp forms them in the mode k describes"""
    if k.fast:
        return dd.sqrt(k.sqrt), dd.rsq(k.rsq)
    root = dd.sqrt(k.sqrt)
    return root, root.rcp(k.rcp)


def e_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def e_cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def e_unit(a, k):
    inv = e_sqrt_and_rcp(e_dot(a, a), k)[1]
    return [c * inv for c in a]


def e_vec(a):
    """[n, 3] binary32 -> three exact Err columns"""
    return [Err(a[:, j].astype(D)) for j in range(3)]


def e_sincos(u, k):
    ang = 2.0 * np.pi * u.astype(D)
    return Err(np.sin(ang), k.sin_abs), Err(np.cos(ang), k.sin_abs)


# ---- binary32 restatements (parity association order, no contraction: numpy rounds every operation) --------------------
def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def unit32(a):
    """unit() of parity mode: f = 1.f / sqrt(a.a), a * f"""
    with np.errstate(all="ignore"):
        return (a * (F(1) / np.sqrt(dot32(a, a)))[..., None]).astype(F)


def pairs32(rays, table):
    """hit_pre / hit_roots / hit_post of every (ray, sphere) pair in binary32 -- tests/test_tile_candidates.py::discriminants for all
    spheres at once, extended by b and the roots (the CPU test holds det to that function bit for bit)"""
    o, d = rays[:, None, 0:3].astype(F), rays[:, None, 3:6].astype(F)
    with np.errstate(all="ignore"):
        op = (table[None, :, 0:3] - o).astype(F)
        b = dot32(op, d)
        det = (b * b - dot32(op, op)) + table[None, :, 3]
        sq = np.sqrt(det)
        t1, t2 = b - sq, b + sq
        eps = F(0.01)
        hit = (det >= 0) & (t2 > eps)
        t = np.where(t1 > eps, t1, t2)
        t_post = np.where(det < 0, F(0), np.where(t1 > eps, t1, np.where(t2 > eps, t2, F(0))))
    return {"b": b, "det": det, "t": t, "hit": hit, "t_post": t_post.astype(F)}


def scene_from_pairs(t, hit, max_t):
    """sweep_closest / sweep_any over per-pair results [R, S] (of any arithmetic): -> t, id, first"""
    n = t.shape[1]
    best, idx = np.full(len(t), T_NONE, t.dtype), np.zeros(len(t), np.int64)
    first = np.full(len(t), n, np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            take = hit[:, i] & (t[:, i] < best)
            best, idx = np.where(take, t[:, i], best), np.where(take, i, idx)
            block = hit[:, i] & (t[:, i] < max_t) & (first == n)
            first = np.where(block, i, first)
    return {"t": best, "id": idx, "first": first}


def table_of(spheres):
    """{centre, radius^2} as rt_scene.hip builds it: the square in binary32"""
    with np.errstate(all="ignore"):
        return np.concatenate([spheres["p"].astype(F), (spheres["rad"] * spheres["rad"]).astype(F)[:, None]], 1)


def bits_equal(a, b):
    """bit for bit, any two NaNs counting as equal"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the generator (rt_trace.inc.h next_random_word), exact ---------------------------------------------------------------
def mwc_word(s0, s1):
    s0 = (np.uint32(36969) * (s0 & np.uint32(65535)) + (s0 >> np.uint32(16))).astype(np.uint32)
    s1 = (np.uint32(18000) * (s1 & np.uint32(65535)) + (s1 >> np.uint32(16))).astype(np.uint32)
    word = ((s0 << np.uint32(16)) + s1).astype(np.uint32)
    f = ((word & np.uint32(0x007fffff)) | np.uint32(0x40000000)).view(F)          # in [2, 4) on a 2^-22 grid
    return s0, s1, f


# ---- (ray, sphere) pairs in binary64 with envelopes ------------------------------------------------------------------
def pairs64(rays, table, k, o_env=None, d_env=None):
    """-> dict of [R, S]: det, b, t1, t2 (Err); finite (records and rays the analysis covers); hit (the binary64 decision);
    decided (the exclusion rule lets the hit / miss decision be compared); t, t_env, t_decided (distance, envelope, and whether which
    root is returned can be compared as well).
    o_env, d_env: three Err columns [R] each -- the origin and the direction as binary64 values WITH envelopes (rays the device forms
    itself, e.g. camera rays: shade64(0, ...)); they take the place of the columns of `rays`, which are then not read.  Absent: the rays
    are exact binary32 inputs, as before."""
    with np.errstate(all="ignore"):
        o = [Err(rays[:, None, j].astype(D)) for j in range(3)] if o_env is None else [Err(c.v[:, None], c.e[:, None]) for c in o_env]
        d = [Err(rays[:, None, 3 + j].astype(D)) for j in range(3)] if d_env is None else [Err(c.v[:, None], c.e[:, None]) for c in d_env]
        op = [Err(table[None, :, j].astype(D)) - o[j] for j in range(3)]
        b = e_dot(op, d)
        det = (b * b - e_dot(op, op)) + Err(table[None, :, 3].astype(D))
        sq = det.sqrt(k.sqrt)
        t1, t2 = b - sq, b + sq
        finite = np.isfinite(det.v) & np.isfinite(det.e) & np.isfinite(b.v)
        det_clear = np.abs(det.v) > det.e
        miss = det.v < 0
        t2_clear = np.abs(t2.v - EPS) > t2.e
        t1_clear = np.abs(t1.v - EPS) > t1.e
        hit = finite & ~miss & (t2.v > EPS)
        decided = finite & det_clear & (miss | t2_clear)
        near = t1.v > EPS
        t = np.where(near, t1.v, t2.v)
        t_env = np.where(near, t1.e, t2.e)
    return {"det": det, "b": b, "t1": t1, "t2": t2, "finite": finite, "hit": hit, "decided": decided, "t": t, "t_env": t_env,
            "t_decided": decided & hit & t1_clear}


def closed_det_bound(p, table):
    """12 * 2^-24 (b^2 + |op|^2) + 2^-24 r^2 of the module docstring (|d| = 1), from pairs64's values"""
    b2 = p["b"].v ** 2
    op2 = b2 - (p["det"].v - table[None, :, 3].astype(D))            # det = b^2 - |op|^2 + r^2
    return U * (12.0 * (b2 + np.abs(op2)) + np.abs(table[None, :, 3].astype(D)))


def scene64(p, max_t):
    """The sweeps' answers in binary64 and which rays the exclusion rule lets be compared.  p = pairs64(...).
    -> id, any_hit, id_decided: the closest hit, whether there is one, and whether every pair of the ray is decided and the winner leads
       every other hit by more than the two envelopes together;
       first, first_decided: the first blocker closer than max_t (n: none); decided when the blocker and every record in front of it are.
    max_t: a binary32 array (exact), or an Err [R] whose envelope then counts towards every tie with it."""
    n = p["t"].shape[1]
    max_env = 0.0
    if isinstance(max_t, Err):                  # a bound the device formed itself (len - EPS of a shadow ray): its envelope widens every tie with it
        max_t, max_env = max_t.v, max_t.e[:, None]
    max_t = max_t.astype(D)[:, None]
    with np.errstate(all="ignore"):
        ok = ~p["finite"] | (p["decided"] & (~p["hit"] | p["t_decided"]))      # (a non-finite record never hits: asserted apart)
        hit = p["hit"] & (p["t"] < 1e20)
        t = np.where(hit, p["t"], np.inf)
        lo, hi = np.where(hit, p["t"] - p["t_env"], np.inf), np.where(hit, p["t"] + p["t_env"], np.inf)
        idx = np.argmin(t, 1)
        any_hit = hit.any(1)
        rows = np.arange(len(t))
        lo_others = lo.copy()
        lo_others[rows, idx] = np.inf
        id_decided = ok.all(1) & (~any_hit | (hi[rows, idx] < lo_others.min(1)))
        blocks = hit & (p["t"] < max_t)
        block_clear = ok & (~hit | (np.abs(p["t"] - max_t) > p["t_env"] + max_env))
        first = np.where(blocks.any(1), np.argmax(blocks, 1), n)
        first_unclear = np.where((~block_clear).any(1), np.argmax(~block_clear, 1), n)
        first_decided = first_unclear > np.minimum(first, n - 1)
    return {"id": np.where(any_hit, idx, 0), "any_hit": any_hit, "id_decided": id_decided, "first": first, "first_decided": first_decided}


def cap(name, skipped, total, limit=0.02):
    """The exclusion rule's cap: at most 2 % of a family's comparisons may be left out"""
    frac = float(skipped) / float(max(total, 1))
    assert frac <= limit, "%s: %d of %d comparisons (%.2f %%) lie within the envelope of a tie; the cap is %.0f %%" % (
        name, skipped, total, 100 * frac, 100 * limit)
    return frac


def check_pairs(name, got, p, verbose=True):
    """The assertions of the (ray, sphere) pairs on `got` (a Probe.pairs / pairs32 result) against p = pairs64(...).
    -> {observed / bound ratios, counts}."""
    fin = p["finite"]
    with np.errstate(all="ignore"):
        r_det = np.where(fin, np.abs(got["det"].astype(D) - p["det"].v) / p["det"].e, 0.0)
        r_b = np.where(fin, np.abs(got["b"].astype(D) - p["b"].v) / p["b"].e, 0.0)
        both = p["t_decided"] & got["hit"]
        r_t = np.where(both, np.abs(got["t"].astype(D) - p["t"]) / p["t_env"], 0.0)
    out = {"det": float(r_det.max()), "b": float(r_b.max()), "t": float(r_t.max()), "pairs": int(fin.sum()),
           "skipped": int((fin & ~p["decided"]).sum() + (fin & p["decided"] & p["hit"] & ~p["t_decided"]).sum()),
           "hits": int((p["decided"] & p["hit"]).sum()), "misses": int((p["decided"] & ~p["hit"]).sum())}
    if verbose:
        print("%-28s pairs %8d  skipped %6d (%.3f %%)  hits %7d  misses %8d   observed / bound: b %.3f  det %.3f  t %.3f" % (
            name, out["pairs"], out["skipped"], 100.0 * out["skipped"] / max(out["pairs"], 1), out["hits"], out["misses"], out["b"], out["det"], out["t"]))
    assert out["b"] <= 1.0, (name, "b outside its envelope", out["b"])
    assert out["det"] <= 1.0, (name, "det outside its envelope", out["det"])
    wrong = p["decided"] & (got["hit"] != p["hit"])
    assert not wrong.any(), (name, "hit / miss differs from binary64 away from a tie", np.argwhere(wrong)[:4].tolist())
    assert out["t"] <= 1.0, (name, "t outside its envelope", out["t"])
    # the reference's form of the test (hit_post) and the sweeps' (hit_roots) are one decision
    same = bits_equal(got["t_post"], np.where(got["hit"], got["t"], F(0)))
    assert same.all(), (name, "hit_post and hit_roots disagree", np.argwhere(~same)[:4].tolist())
    # NaN and infinite records never hit at a finite distance (and so never win a sweep: both compare t < a finite bound)
    bad = ~fin & got["hit"] & np.isfinite(got["t"])
    assert not bad.any(), (name, "a non-finite record hit", np.argwhere(bad)[:4].tolist())
    return out


def check_scene(name, got, p, max_t, verbose=True, tie=False):
    """probe_scene's (or scene_from_pairs') answers against binary64 where the exclusion rule decides them.  -> counts.
    tie=True (the shadow family, whose max_t IS a blocker's distance give or take a few ulps): the first blocker must still be one of the
    answers binary64 gives with max_t moved 2^-10 of itself either way (a thousand times the envelopes), or a record whose own distance
    lies in that band -- whichever way the ties fall."""
    s = scene64(p, max_t)
    if tie:
        m = np.abs(max_t.astype(D)) * 2.0 ** -10
        lo, hi = scene64(p, (max_t.astype(D) - m)), scene64(p, (max_t.astype(D) + m))
        both = lo["first_decided"] & hi["first_decided"]
        assert both.mean() > 0.9, (name, float(both.mean()))
        one_of = (got["first"] == lo["first"]) | (got["first"] == hi["first"])
        n_rec = p["t"].shape[1]                                       # (or any other record whose distance lies in that band)
        in_band = p["hit"] & (np.abs(p["t"] - max_t.astype(D)[:, None]) <= m[:, None])
        one_of |= (got["first"] < n_rec) & in_band[np.arange(len(m)), np.minimum(got["first"], n_rec - 1)]
        assert one_of[both].all(), (name, "any hit at a tie: neither of the two possible first blockers", np.nonzero(both & ~one_of)[0][:4].tolist())
    idd, fd = s["id_decided"], s["first_decided"]
    got_hit = got["t"] < T_NONE
    assert np.array_equal(got_hit[idd], s["any_hit"][idd]), (name, "closest: hit / miss differs away from a tie")
    sel = idd & s["any_hit"]
    assert np.array_equal(got["id"][sel], s["id"][sel]), (name, "closest: another sphere wins away from a tie", np.nonzero(sel & (got["id"] != s["id"]))[0][:4].tolist())
    assert np.array_equal(got["first"][fd], s["first"][fd]), (name, "any hit: another first blocker away from a tie", np.nonzero(fd & (got["first"] != s["first"]))[0][:4].tolist())
    # non-finite records are never the answer
    nonfinite = ~p["finite"]
    rows = np.arange(len(got["id"]))
    assert not (got_hit & nonfinite[rows, got["id"]]).any(), (name, "a non-finite record won the sweep")
    blocked = got["first"] < p["t"].shape[1]
    assert not (blocked & nonfinite[rows, np.minimum(got["first"], p["t"].shape[1] - 1)]).any(), (name, "a non-finite record blocked")
    out = {"rays": len(idd), "id_skipped": int((~idd).sum()), "first_skipped": int((~fd).sum()), "blocked": int((fd & (s["first"] < p["t"].shape[1])).sum()),
           "hits": int(sel.sum())}
    if verbose:
        print("%-28s rays %5d  closest skipped %4d  any-hit skipped %4d  decided hits %5d  decided blockers %5d" % (
            name, out["rays"], out["id_skipped"], out["first_skipped"], out["hits"], out["blocked"]))
    return out


def check_ray_totals(fam, tot):
    """Of a family's rays over all scenes: the two families built AT ties keep a floor of decided rays instead of the 2 % cap.  grazing:
    steps of +-1 and +-8 units of 2^-23 lie inside det's envelope whatever the geometry (the step moves det by 4 k u r s against an
    envelope of 12 u (2 s^2 + r^2) with s the distance to the tangent point: a ratio of at most k / 8.5), +-64 outside: a third of the
    rays at least is decided.  shadow: max_t sits on the blocker's distance, so any-hit is decided only where an earlier record
    blocks; check_scene(tie=True) holds the rest to the two possible answers, so none of those rays goes unchecked."""
    if fam == "grazing":
        assert tot["rays"] - tot["id_skipped"] >= tot["rays"] // 3, tot
    assert tot["hits"] > 0 and tot["misses"] > 0, tot


# ---- ray families -----------------------------------------------------------------------------------------------------
N_RAYS = 4096
FAMILIES = ("camera", "leaving", "grazing", "inside", "far", "shadow")


def _normalise32(v):
    v = v.astype(F)
    return unit32(v)


def _random_units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def camera_rays32(cam, w, h, px, py, j1, j2):
    """rt_shade.inc.h camera_direction / camera_origin and unit() in binary32 (as tests/test_tile_candidates.py::tile_rays forms them)
    -> rd, o, d"""
    inv_w, inv_h = F(1) / F(w), F(1) / F(h)
    kcx = (px.astype(F) + j1.astype(F)) * inv_w - F(0.5)
    kcy = (py.astype(F) + j2.astype(F)) * inv_h - F(0.5)
    co, cd, cx, cy = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    rd = np.stack([(cx[k] * kcx + cy[k] * kcy) + cd[k] for k in range(3)], 1).astype(F)
    o = (rd * F(0.1) + co[None, :]).astype(F)
    return rd, o, unit32(rd)


def _usable(spheres, max_radius):
    """finite spheres of a radius in [0.5, max_radius] whose centre is within 2e4 of the origin (the fixtures hold spheres 5e5 away:
    distance is the `far` family's subject, not every family's)"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(spheres["p"]).all(1) & np.isfinite(spheres["rad"]) & (spheres["rad"] >= 0.5) & (spheres["rad"] <= max_radius)
        ok &= np.abs(spheres["p"]).max(1) <= 2e4
    return np.nonzero(ok)[0]


def _surface_points(rng, spheres, idx, orig):
    """binary32 points on spheres idx, on the side that faces `orig` (the scene's camera) -> (points, binary64 unit normals)"""
    c, r = spheres["p"][idx].astype(D), spheres["rad"][idx].astype(D)
    to_cam = np.asarray(orig, D)[None, :] - c
    to_cam /= np.linalg.norm(to_cam, axis=1)[:, None]
    n = to_cam + 0.9 * _random_units(rng, len(idx)) * np.minimum(1.0, 60.0 / r)[:, None]       # (a huge sphere: the patch in front of the camera)
    n /= np.linalg.norm(n, axis=1)[:, None]
    hp = (c + r[:, None] * n).astype(F)
    return hp, n


def family(name, spheres, orig, target, seed):
    """N_RAYS rays [N, 7] = origin, direction, max_t (binary32) of one family for one scene.  Seeded; the scene's camera gives the side
    the rays come from."""
    rng = np.random.default_rng(seed)
    n = N_RAYS
    from raytracing_simple_amd import host
    cam = host.compute_camera(tuple(float(v) for v in orig), tuple(float(v) for v in target), 64, 40)
    big = _usable(spheres, 2e4)
    small = _usable(spheres, 1500.0)            # surfaces rays leave: not the 1e4 walls, where EPS itself is inside the envelope (see below)
    if len(small) == 0:
        small = big
    max_t = np.full(n, T_NONE, F)
    if name == "camera":
        k = np.arange(n) % (64 * 40)
        j = (rng.integers(0, 1 << 23, (2, n)) / F(1 << 23) - 0.5).astype(F)
        _, o, d = camera_rays32(cam, 64, 40, k % 64, k // 64, j[0], j[1])
    elif name == "leaving":
        # origin = a binary32 point of a surface; the mirrored direction of a ray that arrived from the camera's side, and a cosine-weighted
        # one.  The sphere just left answers t = 0 +- rounding against EPS = 0.01: on a sphere of radius 1e4 the envelope of that root
        # (about 2^-24 * 20 r^2 / (2 r cos)) reaches EPS itself, so the 1e4 walls are left to the other families' far roots.
        idx = small[rng.integers(0, len(small), n)]
        hp, nrm = _surface_points(rng, spheres, idx, orig)
        d_in = hp.astype(D) - np.asarray(orig, D)[None, :] + 5.0 * _random_units(rng, n)
        d_in /= np.linalg.norm(d_in, axis=1)[:, None]
        dn = (d_in * nrm).sum(1)
        nrm = np.where((dn > 0)[:, None], -nrm, nrm)
        refl = d_in - 2.0 * (d_in * nrm).sum(1)[:, None] * nrm
        a = np.where((np.abs(nrm[:, 0]) > 0.1)[:, None], np.array([0.0, 1.0, 0.0])[None, :], np.array([1.0, 0.0, 0.0])[None, :])
        uu = np.cross(a, nrm)
        uu /= np.linalg.norm(uu, axis=1)[:, None]
        vv = np.cross(nrm, uu)
        phi, r2 = 2 * np.pi * rng.random(n), rng.random(n)
        cosd = uu * (np.cos(phi) * np.sqrt(r2))[:, None] + vv * (np.sin(phi) * np.sqrt(r2))[:, None] + nrm * np.sqrt(1 - r2)[:, None]
        o, d = hp, _normalise32(np.where((np.arange(n) % 2 == 0)[:, None], refl, cosd))
        max_t = rng.uniform(1.0, 300.0, n).astype(F)
    elif name == "grazing":
        # from a point outside sphere i, the tangent direction (binary64), then moved in the plane of the centre by k units of 2^-23 (an
        # ulp of a direction of length one) outward (+) or inward (-): k = +-1, +-8, +-64.  The direction is not renormalised: |d| != 1.
        idx = big[rng.integers(0, len(big), n)]
        c, r = spheres["p"][idx].astype(D), spheres["rad"][idx].astype(D)
        away = _random_units(rng, n)
        dist = r * rng.uniform(1.2, 2.5, n)
        o = (c + away * dist[:, None]).astype(F)
        oc = c - o.astype(D)
        L = np.linalg.norm(oc, axis=1)
        axis = oc / L[:, None]
        side = np.cross(axis, _random_units(rng, n))
        side /= np.linalg.norm(side, axis=1)[:, None]
        sb = r / L
        d0 = axis * np.sqrt(1 - sb * sb)[:, None] + side * sb[:, None]
        outward = side * np.sqrt(1 - sb * sb)[:, None] - axis * sb[:, None]
        steps = np.array([-64, -8, -1, 1, 8, 64], D)[np.arange(n) % 6]
        d = (d0.astype(F).astype(D) + outward * (steps * 2.0 ** -23)[:, None]).astype(F)
    elif name == "inside":
        idx = big[rng.integers(0, len(big), n)]
        c, r = spheres["p"][idx].astype(D), spheres["rad"][idx].astype(D)
        o = (c + _random_units(rng, n) * (r * np.minimum(0.9 * rng.random(n), 100.0 / r))[:, None]).astype(F)
        d = _normalise32(_random_units(rng, n))
    elif name == "far":
        # 1e4 away.  There binary32 no longer resolves a sphere of radius 10 (the envelope of det is about 80, the sphere's largest det 100):
        # the rays are aimed through and past the spheres of radius 200 and more; a scene without one gets rays that pass its spheres at 30 to
        # 100 units (clear misses).
        huge = big[spheres["rad"][big] >= 200.0]
        idx = huge[rng.integers(0, len(huge), n)] if len(huge) else big[rng.integers(0, len(big), n)]
        c, r = spheres["p"][idx].astype(D), spheres["rad"][idx].astype(D)
        off = r * rng.uniform(0.0, 1.5, n) if len(huge) else r + rng.uniform(30.0, 100.0, n)
        aim = c + _random_units(rng, n) * off[:, None]
        o = (aim + _random_units(rng, n) * 1e4).astype(F)
        d = _normalise32(aim - o.astype(D))
    elif name == "shadow":
        # from a surface point towards a point of another sphere; max_t = that blocker's binary64 distance rounded to binary32 and moved
        # by +-1, +-2, +-4 ulps: the compare t < max_t of sweep_any at its tie
        ia = small[rng.integers(0, len(small), n)]
        hp, _ = _surface_points(rng, spheres, ia, orig)
        ib = big[rng.integers(0, len(big), n)]
        c, r = spheres["p"][ib].astype(D), spheres["rad"][ib].astype(D)
        aim = c + _random_units(rng, n) * (r * np.minimum(0.7, 40.0 / r))[:, None]
        o, d = hp, _normalise32(aim - hp.astype(D))
        p = pairs64(np.concatenate([o, d], 1), table_of(spheres), K.exact())
        t_b = p["t"][np.arange(n), ib]
        hits = p["hit"][np.arange(n), ib]
        base = np.where(hits, t_b, 50.0).astype(F)
        steps = np.array([-4, -2, -1, 1, 2, 4])[np.arange(n) % 6]
        max_t = (base.view(np.int32) + steps.astype(np.int32)).view(F)
    else:
        raise KeyError(name)
    return np.concatenate([o.astype(F), d.astype(F), max_t[:, None]], 1)


def scenes_of_the_rays():
    """[(name, spheres, orig, target)]: the Demo scene, the mirror box, 256 random spheres, the eight adversarial fixtures"""
    from raytracing_simple_amd import host, scenes
    out = [("demo", host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET),
           ("mirror_box64",) + tuple(scenes.mirror_box(64)), ("random256",) + tuple(scenes.random_spheres(256))]
    z = np.load(os.path.join(ROOT, "tests", "golden", "fuzz_candidates.npy"))
    for k, rec in enumerate(z):
        out.append(("fuzz%d" % k, rec["spheres"][:int(rec["n"])].copy(), tuple(float(v) for v in rec["orig"]), tuple(float(v) for v in rec["target"])))
    return out


# ---- scalar blocks in binary64 ------------------------------------------------------------------------------------------
GAMMA = 1.0 / 2.2


def to_int64(v):
    """floor(clip(v, 0, 1)^(1/2.2) * 255 + 0.5) in binary64 -> (code value, distance of the argument of floor from an integer).
    NaN clips to 0 as fminf(fmaxf(v, 0), 1) does."""
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(v), 0.0, np.clip(v.astype(D), 0.0, 1.0))
        y = c ** GAMMA * 255.0 + 0.5
    return np.floor(y).astype(np.int64), np.abs(y - np.round(y))


def to_int_inputs():
    """every float within +-64 ulps of each of the 255 rounding boundaries (bisection in binary64), every 1024th bit pattern of [0, 1],
    and the edges"""
    near = []
    for m in range(1, 256):
        lo, hi = 0.0, 1.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if mid ** GAMMA * 255.0 + 0.5 < m:
                lo = mid
            else:
                hi = mid
        centre = int(np.array([hi], F).view(np.uint32)[0])
        near.append(np.arange(centre - 64, centre + 65, dtype=np.int64))
    near = np.concatenate(near)
    near = near[(near >= 0) & (near <= 0x3f800000)].astype(np.uint32).view(F)
    grid = np.arange(0, 0x3f800000 + 1, 1024, dtype=np.uint32).view(F)
    one_up = np.array([0x3f800001], np.uint32).view(F)
    edges = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 2.0 ** -126, 1.0, one_up[0], 7.5, -2.0 ** -149, -1.0, -7.5,
                      np.inf, -np.inf, np.nan], F)
    return near, grid, edges


def log_uniform(rng, lo_exp, hi_exp, n):
    """n binary32 values, exponent uniform in [lo_exp, hi_exp), mantissa uniform"""
    return (2.0 ** rng.uniform(lo_exp, hi_exp, n)).astype(F)


# ---- shading steps: binary32 restatement and binary64 with envelopes ------------------------------------------------------
def shade_inputs(what, rng, n=N_RAYS):
    """-> (rec [n, 16] binary32 words, cam [14] or None, extra): the input records of probe_shade's step `what`"""
    rec = np.zeros((n, 16), F)
    words = rec.view(np.uint32)
    cam14, extra = None, {}
    if what in (0, 4):
        seeds = rng.integers(2, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    if what == 0:
        from raytracing_simple_amd import host
        w, h = 64, 40
        cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
        k = np.arange(n) % (w * h)
        words[:, 0], words[:, 1] = seeds[:, 0], seeds[:, 1]
        words[:, 2] = (k % w).astype(np.uint32) | ((k // w).astype(np.uint32) << np.uint32(16))
        cam14 = np.concatenate([cam[0:3], cam[6:9], cam[9:12], cam[12:15], [F(1) / F(w), F(1) / F(h)]]).astype(F)
        extra = {"cam": cam, "w": w, "h": h, "px": k % w, "py": k // w}
    elif what == 1:
        rec[:, 0:3] = _normalise32(_random_units(rng, n))
        rec[:n // 8, 0] = np.where(np.arange(n // 8) % 2 == 0, F(0.1), np.nextafter(F(0.1), F(1)))          # the basis' axis choice at its threshold
        rec[:n // 8, 0:3] = unit32(rec[:n // 8, 0:3])
        rec[:, 3] = (rng.integers(0, 1 << 23, n) / F(1 << 23)).astype(F)
        rec[:, 4] = (rng.integers(0, 1 << 23, n) / F(1 << 23)).astype(F)
        rec[:4, 4] = [0.0, 2.0 ** -23, 1 - 2.0 ** -23, 0.5]
    elif what == 2:
        rec[:, 0:3] = _normalise32(_random_units(rng, n))
        rec[:, 3:6] = _normalise32(_random_units(rng, n))
        g = n // 4                                                      # a quarter grazing: d nearly perpendicular to the normal
        perp = np.cross(rec[:g, 0:3].astype(D), _random_units(rng, g))
        rec[:g, 3:6] = _normalise32(perp + rec[:g, 0:3].astype(D) * rng.normal(0, 1e-6, g)[:, None])
    elif what == 3:
        into = np.arange(n) % 2 == 0
        rec[:, 0] = np.where(into, F(1) / F(1.52), F(1.52) / F(1))
        rec[:, 1] = -rng.random(n).astype(F)
        crit = -np.sqrt(1 - 1 / 1.52 ** 2)                              # total internal reflection begins here
        rec[:n // 4, 1] = (crit + rng.normal(0, 1e-5, n // 4)).astype(F)
        rec[:, 2] = rng.random(n).astype(F)
        rec[:, 3] = (rng.integers(0, 1 << 23, n) / F(1 << 23)).astype(F)      # the roulette's draw (compared on the host)
    else:
        rec[:, 0:3] = rng.uniform(-50, 50, (n, 3)).astype(F) + F(60) * np.array([0, 1, 0], F)
        rec[:, 3] = rng.uniform(1, 12, n).astype(F)
        rec[:, 4] = (F(4) * F(np.pi) * rec[:, 3] * rec[:, 3]).astype(F)
        words[:, 5], words[:, 6] = seeds[:, 0], seeds[:, 1]
        rec[:, 7:10] = rng.uniform(-80, 80, (n, 3)).astype(F)
        rec[:, 10:13] = _normalise32(_random_units(rng, n))
    return rec, cam14, extra


def _om(name, x):
    import _oracle as O
    fn = getattr(O.oracle(), name)
    return np.array([fn(float(v)) for v in x], F)


def sincos32(u):
    """parity mode's sine and cosine of a draw: the oracle's sinf / cosf of fl(fl(2 pi) u)"""
    ang = ((F(2) * F(3.14159265358979323846)) * u.astype(F)).astype(F)
    return _om("om_sinf", ang), _om("om_cosf", ang)


def shade32(what, rec, extra):
    """probe_shade's step in binary32, parity association order -> [n, 12]"""
    n = len(rec)
    words = rec.view(np.uint32)
    out = np.zeros((n, 12), F)
    with np.errstate(all="ignore"):
        if what == 0:
            s0, s1, f1 = mwc_word(words[:, 0].copy(), words[:, 1].copy())
            s0, s1, f2 = mwc_word(s0, s1)
            j1, j2 = f1 * F(0.5) - F(1.5), f2 * F(0.5) - F(1.5)
            rd, o, d = camera_rays32(extra["cam"], extra["w"], extra["h"], extra["px"], extra["py"], j1, j2)
            out[:, 0:3], out[:, 3:6], out[:, 6:9] = rd, o, d
        elif what == 1:
            w, u, r2 = rec[:, 0:3], rec[:, 3], rec[:, 4]
            r2s = np.sqrt(r2)
            a = np.where((np.abs(w[:, 0]) > F(0.1))[:, None], np.array([0, 1, 0], F)[None, :], np.array([1, 0, 0], F)[None, :])
            uu = unit32(cross32(a, w))
            vv = cross32(w, uu)
            sn, cs = sincos32(u)
            nd = (uu * (cs * r2s)[:, None] + vv * (sn * r2s)[:, None]) + w * np.sqrt(F(1) - r2)[:, None]
            out[:, 0:3], out[:, 3:6], out[:, 6:9] = uu, vv, nd
        elif what == 2:
            nrm, d = rec[:, 0:3], rec[:, 3:6]
            dp = dot32(nrm, d)
            out[:, 0] = dp
            out[:, 1:4] = nrm * (F(-1) * np.sign(dp))[:, None]
            out[:, 4:7] = d - nrm * (F(2) * dp)[:, None]
        elif what == 3:
            nnt, ddn, re = rec[:, 0], rec[:, 1], rec[:, 2]
            out[:, 0] = F(1) - nnt * nnt * (F(1) - ddn * ddn)
            out[:, 1] = F(0.25) + F(0.5) * re
        else:
            s0, s1, f1 = mwc_word(words[:, 5].copy(), words[:, 6].copy())
            s0, s1, f2 = mwc_word(s0, s1)
            zc, u2 = F(3) - f1, f2 * F(0.5) - F(1)
            ring = np.sqrt(np.maximum(F(0), F(1) - zc * zc))
            sn, cs = sincos32(u2)
            us = np.stack([ring * cs, ring * sn, zc], 1)
            sd = (us * rec[:, 3:4] + rec[:, 0:3]) - rec[:, 7:10]
            length = np.sqrt(dot32(sd, sd))
            sd = sd * (F(1) / length)[:, None]
            wo = dot32(sd, us)
            wi = dot32(sd, rec[:, 10:13])
            out[:, 0] = ((wo <= 0) & (wi > 0)).astype(F)
            out[:, 1:4], out[:, 4], out[:, 5] = sd, length, rec[:, 4] * wi * (-wo)
    return out


def sample_light64(zc, u2, centre, rad, area, hp, nl, k):
    """sample_light_drawn (rt_trace.inc.h) in binary64 with envelopes.  zc: Err (exact: a 2^-22 grid), u2: binary32 (exact), centre: three
    columns, rad / area (lightA.w, lightB.w): binary32 arrays, hp / nl: three Err columns each -- exact records (shade64(4, ...)) or the
    hit point and facing normal a kernel formed itself, WITH their envelopes (tests/_shadow_frames.py).
    -> us, on (the sampled point), sd, len, wo, wi, numer (Err) and want (binary64's decision wo <= 0 and wi > 0)"""
    inner = 1.0 - zc * zc
    ring = Err(np.maximum(inner.v, 0.0), inner.e).sqrt(k.sqrt)
    sn, cs = e_sincos(u2, k)
    us = [ring * cs, ring * sn, zc]
    centre = [Err.of(c) for c in centre]
    on = [us[c] * Err(np.asarray(rad).astype(D)) + centre[c] for c in range(3)]
    sd = [on[c] - hp[c] for c in range(3)]
    length, inv = e_sqrt_and_rcp(e_dot(sd, sd), k)
    sd = [c * inv for c in sd]
    wo, wi = e_dot(sd, us), e_dot(sd, nl)
    numer = (Err(np.asarray(area).astype(D)) * wi) * (-wo)
    return {"us": us, "on": on, "sd": sd, "len": length, "wo": wo, "wi": wi, "numer": numer, "want": (wo.v <= 0) & (wi.v > 0)}


def shade64(what, rec, extra, k):
    """-> (list of (label, column(s) of the output, Err), decisions): each output of the step with its envelope.  The bound of every line
    is the running error of the operations written on it (module docstring); `decisions` are (label, Err, threshold) of the quantities
    a decision hangs on."""
    words = rec.view(np.uint32)
    items, ties = [], []
    with np.errstate(all="ignore"):
        if what == 0:
            s0, s1, f1 = mwc_word(words[:, 0].copy(), words[:, 1].copy())
            s0, s1, f2 = mwc_word(s0, s1)
            j1, j2 = f1.astype(D) * 0.5 - 1.5, f2.astype(D) * 0.5 - 1.5               # exact: a 2^-23 grid in [-0.5, 0.5)
            cam = extra["cam"].astype(D)
            inv_w, inv_h = float(F(1) / F(extra["w"])), float(F(1) / F(extra["h"]))
            kcx = (Err(extra["px"].astype(D)) + Err(j1)) * inv_w - 0.5               # (pixel + jitter) * inv_size - 0.5: three roundings
            kcy = (Err(extra["py"].astype(D)) + Err(j2)) * inv_h - 0.5
            rd = [(kcx * cam[9 + c] + kcy * cam[12 + c]) + cam[6 + c] for c in range(3)]   # two products, two sums per component
            o = [rd[c] * float(F(0.1)) + cam[c] for c in range(3)]
            d = e_unit(rd, k)
            items = [("camera rd", slice(0, 3), rd), ("camera origin", slice(3, 6), o), ("camera direction", slice(6, 9), d)]
        elif what == 1:
            w = e_vec(rec[:, 0:3])
            u, r2 = rec[:, 3], rec[:, 4]
            r2s = Err(r2.astype(D)).sqrt(k.sqrt)
            axis_y = np.abs(rec[:, 0]) > F(0.1)                                      # decided on an INPUT: exact in every mode
            a = [Err(np.where(axis_y, 0.0, 1.0)), Err(np.where(axis_y, 1.0, 0.0)), Err(np.zeros(len(rec)))]
            uu = e_unit(e_cross(a, w), k)                                            # products with 0 and 1 are exact: covered by |v| = 0 terms
            vv = e_cross(w, uu)
            sn, cs = e_sincos(u, k)
            last = (1.0 - Err(r2.astype(D))).sqrt(k.sqrt)
            c1, c2 = cs * r2s, sn * r2s
            nd = [(uu[c] * c1 + vv[c] * c2) + w[c] * last for c in range(3)]
            items = [("basis uu", slice(0, 3), uu), ("basis vv", slice(3, 6), vv), ("cosine direction", slice(6, 9), nd)]
        elif what == 2:
            nrm, d = e_vec(rec[:, 0:3]), e_vec(rec[:, 3:6])
            dp = e_dot(nrm, d)
            sgn = -np.sign(dp.v)
            nl = [c.exact_scale(1.0) * Err(sgn) for c in nrm]                         # times +-1: the product's rounding term is zero-width, kept for simplicity
            rfl = [d[c] - nrm[c] * dp.exact_scale(2.0) for c in range(3)]
            items = [("n.d", 0, dp), ("facing normal", slice(1, 4), nl), ("reflected direction", slice(4, 7), rfl)]
            ties = [("side of the surface", dp, 0.0)]
        elif what == 3:
            nnt, ddn, re = Err(rec[:, 0].astype(D)), Err(rec[:, 1].astype(D)), Err(rec[:, 2].astype(D))
            cos2t = 1.0 - (nnt * nnt) * (1.0 - ddn * ddn)
            pr = 0.25 + re.exact_scale(0.5)
            items = [("cos2t", 0, cos2t), ("roulette p", 1, pr)]
            ties = [("total internal reflection", cos2t, 0.0), ("roulette", pr, rec[:, 3].astype(D))]
        else:
            s0, s1, f1 = mwc_word(words[:, 5].copy(), words[:, 6].copy())
            s0, s1, f2 = mwc_word(s0, s1)
            zc, u2 = Err(3.0 - f1.astype(D)), (f2.astype(D) * 0.5 - 1.0).astype(F)    # exact (2^-22 / 2^-23 grids)
            q = sample_light64(zc, u2, e_vec(rec[:, 0:3]), rec[:, 3], rec[:, 4], e_vec(rec[:, 7:10]), e_vec(rec[:, 10:13]), k)
            sd, length, numer, wo, wi, want = q["sd"], q["len"], q["numer"], q["wo"], q["wi"], q["want"]
            items = [("light direction", slice(1, 4), sd), ("light distance", 4, length), ("light numerator", 5, numer)]
            ties = [("far side of the light", wo, 0.0), ("light behind the surface", wi, 0.0)]
            extra = dict(extra, want=want)
    return items, ties, extra


def check_shade(what, got, rec, extra, k, verbose=True):
    """Every output of the step within its envelope, every decision equal to binary64's away from its tie.  -> largest observed / bound"""
    items, ties, extra = shade64(what, rec, extra, k)
    n = len(rec)
    decided = np.ones(n, bool)
    for label, q, thr in ties:
        decided &= np.abs(q.v - thr) > q.e
    compare = decided.copy()
    if what == 4:
        want_got = got[:, 0] != 0
        assert np.array_equal(want_got[decided], extra["want"][decided]), "sample_light: shadow ray wanted / not wanted differs away from a tie"
        compare &= extra["want"]                     # the outputs are defined for the lanes that want a shadow ray
        assert extra["want"][decided].any() and (~extra["want"][decided]).any()
    if what == 2:
        assert np.array_equal(np.sign(got[decided, 0]), np.sign(items[0][2].v[decided])), "side of the surface differs away from a tie"
    if what == 3:
        cos2t, pr = ties[0][1], ties[1][1]
        clear = np.abs(cos2t.v) > cos2t.e
        assert np.array_equal(got[clear, 0] < 0, cos2t.v[clear] < 0), "total internal reflection decided differently away from a tie"
        u = rec[:, 3]
        clear_p = np.abs(pr.v - u.astype(D)) > pr.e
        assert np.array_equal(u[clear_p] < got[clear_p, 1], u[clear_p].astype(D) < pr.v[clear_p]), "roulette decided differently away from a tie"
        assert (cos2t.v[clear] < 0).any() and (cos2t.v[clear] >= 0).any()
        compare = np.ones(n, bool)                   # the two values themselves are continuous: compared everywhere
    cap("shade step %d" % what, int((~decided).sum()), n)
    worst = 0.0
    for label, cols, q in items:
        qs = q if isinstance(q, list) else [q]
        g = got[:, cols].reshape(n, -1).astype(D)
        ratio = 0.0
        for c, e in enumerate(qs):
            sel = compare & np.isfinite(e.e)
            if what == 2 and label == "facing normal":
                sel &= decided
            assert sel.sum() > n // 8, (label, int(sel.sum()))
            r = np.abs(g[sel, c] - e.v[sel]) / e.e[sel]
            ratio = max(ratio, float(r.max()))
        if verbose:
            print("shade step %d  %-22s observed / bound %.3f" % (what, label, ratio))
        assert ratio <= 1.0, (what, label, ratio)
        worst = max(worst, ratio)
    return worst


# ---- fast mode as an unbiased renderer (tests/test_gpu_fast_bias.py, and its preconditions on the CPU) ----------------------------
PARITY_STREAMS = (1, 2, 3, 4)
FAST_STREAM = 5


def bias_scenes():
    """[(name, maker of (spheres, orig, target), w, h)]"""
    from raytracing_simple_amd import scenes

    def glass_and_mirror():
        from test_gpu_parity import _glass_and_mirror_scene
        return _glass_and_mirror_scene()
    return [("mirror_box64", lambda: scenes.mirror_box(64), 64, 48), ("random256", lambda: scenes.random_spheres(256), 64, 48),
            ("glass_and_mirror", glass_and_mirror, 41, 23)]


def brighter_light(spheres, scale):
    """the precondition's first bias: every emission scaled"""
    out = spheres.copy()
    out["e"] = (out["e"] * F(scale)).astype(F)
    return out


def glass_turned_diffuse(spheres):
    """the precondition's second bias: the glass spheres diffuse"""
    from raytracing_simple_amd import api
    out = spheres.copy()
    assert (out["refl"] == api.REFR).any()
    out["refl"][out["refl"] == api.REFR] = api.DIFF
    return out


def bias_gate(among_parity, against_parity):
    """min(F) >= min(D) - (max(D) - min(D)): the candidate frame is no further from an independent parity frame than independent
    parity frames are from each other, by the spread those showed in the same run.  -> (passes, threshold)"""
    threshold = min(among_parity) - (max(among_parity) - min(among_parity))
    return min(against_parity) >= threshold, threshold


# ---- the scalar blocks on the device: input sets and what is observed of them (measured constants) --------------------------------------
def block_inputs(seed=20):
    """{set: array}: 2^20 log-uniform values per exponent range the renderer can produce (the argument ranges in the comments of
    csrc/rt_trace.inc.h), seeded"""
    rng = np.random.default_rng(seed)
    n = 1 << 20
    return {
        "rcp": log_uniform(rng, -60, 60, n) * rng.choice(np.array([-1, 1], F), n),     # 1 / (s + 1), reciprocals of lengths and of squared lengths
        "div_a": log_uniform(rng, -40, 40, n), "div_b": log_uniform(rng, -40, 40, n),     # numer / len^2
        "sqrt": log_uniform(rng, -96, 127, n),                                            # cos2t and whatever else is not a subnormal's neighbour
        "sqrt_unit": np.concatenate([np.zeros(16, F), log_uniform(rng, -96, 0, n - 16)]),  # 0 or >= 2^-96 by construction
        "sqrt_det": log_uniform(rng, -96, 100, n),                                        # a discriminant that passed det >= 0
        "sq_len": log_uniform(rng, -96, 100, n),                                          # sqrt_and_rcp: a squared length
    }


def observe_blocks(probe):
    """The three measured quantities of the fast arm against binary64 -> [{op, observed_max, unit, input, inputs}] (the build id is the caller's).
    Run by tools/measure_fast_blocks.py for profiles/r20_fast_blocks.jsonl, and by the tests, which print observed / bound."""
    assert probe.fast
    x = block_inputs()
    out = []

    def rec(op, err, inputs, unit, what):
        i = int(np.nanargmax(err))
        out.append({"op": op, "observed_max": float(err[i]), "unit": unit, "input": [float(v) for v in np.atleast_1d(inputs[i])], "inputs": what})
    with np.errstate(all="ignore"):
        got = probe.eval("rcp", x["rcp"])[0]
        rec("v_rcp_f32", ulp_error(got, 1.0 / x["rcp"].astype(D)), x["rcp"], "ulp", "rt_rcp, 2^20 log-uniform in +-[2^-60, 2^60)")
        root, inv = probe.eval("sqrt_and_rcp", x["sq_len"])
        rec("v_rsq_f32", ulp_error(inv, 1.0 / np.sqrt(x["sq_len"].astype(D))), x["sq_len"], "ulp", "sqrt_and_rcp's reciprocal, 2^20 log-uniform in [2^-96, 2^100)")
        errs, ins = [ulp_error(root, np.sqrt(x["sq_len"].astype(D)))], [x["sq_len"]]
        for op in ("sqrt", "sqrt_unit", "sqrt_det"):
            errs.append(ulp_error(probe.eval(op, x[op])[0], np.sqrt(x[op].astype(D))))
            ins.append(x[op])
        rec("v_sqrt_f32", np.concatenate(errs), np.concatenate(ins), "ulp", "rt_sqrt, rt_sqrt_unit, rt_sqrt_det and sqrt_and_rcp's root, 2^20 log-uniform each over its range")
        u = (np.arange(1 << 23) / F(1 << 23)).astype(F)
        sn, cs = probe.eval("sincos", u)
        ang = 2.0 * np.pi * u.astype(D)
        rec("v_sin_f32", np.abs(sn.astype(D) - np.sin(ang)), u, "absolute", "fm_sincos_turns, all 2^23 arguments k / 2^23")
        rec("v_cos_f32", np.abs(cs.astype(D) - np.cos(ang)), u, "absolute", "fm_sincos_turns, all 2^23 arguments k / 2^23")
        rec("sincos_pythagoras", np.abs(sn.astype(D) ** 2 + cs.astype(D) ** 2 - 1.0), u, "absolute", "|sin^2 + cos^2 - 1| over the same arguments")
        near, grid, _ = to_int_inputs()
        v = np.concatenate([near, grid])
        code = probe.eval("to_int", v)[0].view(np.int32).astype(np.int64)
        want, dist = to_int64(v)
        differs = code != want
        rec("to_int_delta", np.where(differs, dist, 0.0), v, "distance of clip(v)^(1/2.2) * 255 + 0.5 from an integer",
            "fast to_int against binary64: every float within 64 ulps of the 255 boundaries, every 1024th bit pattern of [0, 1]; %d of %d differ" % (int(differs.sum()), len(v)))
    return out
