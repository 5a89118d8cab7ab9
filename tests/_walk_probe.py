"""The hierarchy walk under fast flags, ray by ray (tests/walk_probe.hip, tests/test_gpu_fast_walk.py; the ray sets and the checks
proved on the CPU in tests/test_fast_walk_cpu.py).

csrc/rt_walk.inc.h carries a kernel that sends arbitrary rays through the walk AND through the plain sweep, one lane per ray
(rt_debug_walk_rays); the library builds it with parity's flags only, and the derivation of the walk's pad is written for parity's
roundings.  walk_probe.hip builds the same text under the fast flags (and, as the control arm, under parity's: that arm must equal the
library's own kernel bit for bit, or the probe is wired wrong and the fast arm means nothing).

Every ray (origin, direction, max_t) is sent TWICE: as a closest-hit ray (which ignores max_t: it starts at 1e20) and as a shadow ray.
The fast arm's answers -- the walk's and the sweep's, each on its own -- go through _fast_reference.check_scene against
pairs64(..., K.measured()) where binary64 can judge the ray: all components finite and the direction within 1e-3 of unit length.
The other rays (the walk gives them an infinite pad and must visit everything) are held to walk == sweep in hit / miss and index; a ray
with a NaN or infinite component must hit nothing in either."""
import ctypes as C
import functools
import os
import sys

import numpy as np

import _fast_reference as R
from _adversarial_rays import adversarial_rays
from raytracing_simple_amd import scenes

sys.path.insert(0, os.path.join(R.ROOT, "tools"))
import bvh_check  # noqa: E402
from bvh_scenes import _adversarial  # noqa: E402

F, D = np.float32, np.float64
NONE = 0xffffffff
N_ADVERSARIAL = 12000
CHUNK = 1024                # rays per pairs64 call: 1024 x 1024 pairs keep the reference below a gigabyte of host memory


class WalkProbe:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.fast = bool(self.lib.walk_probe_is_fast())
        self.lib.walk_probe_rays.restype = C.c_int

    def rays(self, table, tree, rays8):
        """-> out4 [n, 4] uint32 as rt_debug_walk_rays: the walk's answer, then the sweep's"""
        table, blob, rays8 = np.ascontiguousarray(table, F), np.ascontiguousarray(tree["blob"], F), np.ascontiguousarray(rays8, F)
        out = np.zeros((len(rays8), 4), np.uint32)
        rc = self.lib.walk_probe_rays(R._p(table), C.c_uint(len(table)), R._p(blob), C.c_size_t(blob.size // 4), C.c_uint(tree["n_always"]),
                                      C.c_uint(tree["n_leaves"]), C.c_uint(tree["stack_depth"]), R._p(rays8), C.c_uint(len(rays8)), R._p(out))
        if rc != 0:
            raise RuntimeError("walk_probe_rays failed: %d" % rc)
        return out


def tree_of(ctx):
    """the hierarchy of the context's scene as the diagnostics library hands it out: counts (tools/bvh_check.read_bvh) and the whole blob"""
    b = bvh_check.read_bvh(ctx)
    assert b is not None
    n4 = 2 + b["n_slots"] + (b["n_slots"] + 3) // 4 + 4 * (b["n_leaves"] - 1) + 2 * b["n_slots"]
    blob = np.zeros(4 * n4, F)
    counts = (C.c_uint32 * 4)()
    ctx._check(ctx._lib.rt_debug_read_bvh(ctx._h, blob.ctypes.data_as(C.c_void_p), n4, counts))
    assert list(counts) == [b["n_always"], b["n_leaves"], b["stack_depth"], b["root"]]
    return {"blob": blob, "n_always": b["n_always"], "n_leaves": b["n_leaves"], "stack_depth": b["stack_depth"], "n_slots": b["n_slots"]}


def library_answers(ctx, rays8):
    rays8 = np.ascontiguousarray(rays8, F)
    out = np.zeros((len(rays8), 4), np.uint32)
    ctx._check(ctx._lib.rt_debug_walk_rays(ctx._h, rays8.ctypes.data_as(C.c_void_p), len(rays8), out.ctypes.data_as(C.c_void_p)))
    return out


def both_kinds(rays7):
    """[N, 7] = o, d, max_t -> the kernel's records [2N, 8] = o, max_t, d, bits(shadow): ray i as a closest-hit ray at 2i, as a shadow ray at 2i + 1"""
    out = np.zeros((2 * len(rays7), 8), F)
    out[0::2, 0:3] = out[1::2, 0:3] = rays7[:, 0:3]
    out[0::2, 3] = out[1::2, 3] = rays7[:, 6]
    out[0::2, 4:7] = out[1::2, 4:7] = rays7[:, 3:6]
    out[1::2, 7:8].view(np.uint32)[:] = 1
    return out


def answers(out4, first_word):
    """out4 of both_kinds' records -> what check_scene takes: t, id (closest), first (shadow); first_word 0: the walk's, 2: the sweep's"""
    closest, shadow = out4[0::2], out4[1::2]
    hit = closest[:, first_word] != NONE
    t = np.where(hit, closest[:, first_word], np.array([R.T_NONE], F).view(np.uint32)[0]).astype(np.uint32).view(F)
    return {"t": t, "id": np.where(hit, closest[:, first_word + 1], 0).astype(np.int64), "first": shadow[:, first_word].astype(np.int64),
            "hit": hit, "t_bits": closest[:, first_word]}


def judged(rays7):
    """rays binary64 can judge: every component finite, the direction within 1e-3 of unit length"""
    with np.errstate(all="ignore"):
        return np.isfinite(rays7).all(1) & (np.abs(np.linalg.norm(rays7[:, 3:6].astype(D), axis=1) - 1.0) <= 1e-3)


def not_a_number_or_infinite(rays7):
    return ~np.isfinite(rays7[:, 0:6]).all(1)


@functools.lru_cache(maxsize=None)
def walk_scenes():
    """{name: (spheres, orig, target)}"""
    return {"random256": scenes.random_spheres(256), "random1024": scenes.random_spheres(1024), "mirror_box120": scenes.mirror_box(120),
            "adversarial3": _adversarial(3)}


def set_names(name):
    """the six families on the two scattered scenes, the adversarial rays on the three scenes test_walk_equals_sweep_for_adversarial_rays uses"""
    return (list(R.FAMILIES) if name in ("random256", "random1024") else []) + (["adversarial"] if name != "random256" else [])


@functools.lru_cache(maxsize=None)
def ray_sets(name):
    """{set: rays [N, 7]} of scene `name` (seeded)"""
    sph, orig, target = walk_scenes()[name]
    out = {}
    for fam in set_names(name):
        if fam == "adversarial":
            with np.errstate(all="ignore"):
                a = adversarial_rays(sph, np.random.default_rng(len(sph)), N_ADVERSARIAL)
            out[fam] = np.concatenate([a[:, 0:3], a[:, 4:7], a[:, 3:4]], 1)
        else:
            out[fam] = R.family(fam, sph, orig, target, 2600 + 10 * len(sph) + R.FAMILIES.index(fam))
    return out


def check_judged(name, gots, rays7, table, k, tie, verbose=True):
    """check_scene on the rays of `rays7` that binary64 judges (CHUNK at a time, one reference for every answer in `gots` = {label:
    answers(...)}), and the closest distance within its envelope where the ray is decided.  -> {label: summed counts and the largest
    observed / bound of t}"""
    sel = np.nonzero(judged(rays7))[0]
    tots = {label: {"rays": 0, "id_skipped": 0, "first_skipped": 0, "hits": 0, "blocked": 0, "t_ratio": 0.0} for label in gots}
    for a in range(0, len(sel), CHUNK):
        rows = sel[a:a + CHUNK]
        p = R.pairs64(rays7[rows], table, k)
        s = R.scene64(p, np.full(len(rows), R.T_NONE, F))
        at = np.nonzero(s["id_decided"] & s["any_hit"])[0]
        assert p["t_decided"][at, s["id"][at]].all()
        for label, got in gots.items():
            g = {key: got[key][rows] for key in ("t", "id", "first")}
            res = R.check_scene(name + " " + label, g, p, rays7[rows, 6], verbose=False, tie=tie)
            tot = tots[label]
            if len(at):
                with np.errstate(all="ignore"):
                    ratio = np.abs(g["t"][at].astype(D) - p["t"][at, s["id"][at]]) / p["t_env"][at, s["id"][at]]
                assert not np.isnan(ratio).any() and ratio.max() <= 1.0, (name, label, "closest distance outside its envelope", float(ratio.max()),
                                                                          int(rows[at[int(np.argmax(ratio))]]))
                tot["t_ratio"] = max(tot["t_ratio"], float(ratio.max()))
            for key in ("rays", "id_skipped", "first_skipped", "hits", "blocked"):
                tot[key] += res[key]
    if verbose:
        for label, tot in tots.items():
            print("%-40s %-14s judged %5d of %5d  closest skipped %4d  any-hit skipped %4d  decided hits %5d  decided blockers %5d   t observed / bound %.3f" % (
                name, label, tot["rays"], len(rays7), tot["id_skipped"], tot["first_skipped"], tot["hits"], tot["blocked"], tot["t_ratio"]))
    return tots


def check_caps(name, set_name, tot):
    """the 2 % cap of the exclusion rule, except for the sets built AT ties (tests/test_gpu_fast_rays.py): grazing and shadow, and the
    adversarial rays -- of their twelve kinds one is tangent to a sphere to within 1e-7 of its radius, one slides along a box plane (a
    tangent plane of the sphere) and one starts 1e4 .. 1e25 away, where binary32 resolves no sphere: three kinds in twelve are ties or
    beyond the envelopes by construction, and the adversarial SCENE adds exact ties of its own (duplicated records, concentric spheres, a
    zero radius: every ray that meets one is undecided); the set keeps a floor of decided rays instead: one half"""
    if set_name in ("grazing", "shadow"):
        return
    if set_name == "adversarial":
        assert tot["rays"] - tot["id_skipped"] >= tot["rays"] // 2 and tot["rays"] - tot["first_skipped"] >= tot["rays"] // 2, (name, tot)
        return
    R.cap(name + " closest hits", tot["id_skipped"], tot["rays"])
    R.cap(name + " first blockers", tot["first_skipped"], tot["rays"])
