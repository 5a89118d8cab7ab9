"""The scenes tests/test_gpu_features_walk.py forms feature planes of through the hierarchy, and what each is there for.  No device in here:
tests/test_features_walk_cpu.py shows on the hierarchy's host work (tools/sanitize/features_main.cpp FILE: rt_bvh_host.cpp's repeats and its cut
between tree and always-list) and on rt_features_planes that every scene contains what it claims; a case that exercises nothing fails there."""
import os
import re

import numpy as np

from raytracing_simple_amd import api, host

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BVH_MIN = 56                # csrc/rt_instance.h Knobs::bvh_min: the fewest tree spheres that get a hierarchy
SIZES = [(1, 1), (41, 23), (70, 19)]        # partial 32x8 workgroups in both directions: lanes outside the image sit through every ballot and barrier
ORIG, TARGET = (0.0, 0.0, 50.0), (0.0, 0.0, 0.0)


def walk_min():
    """kFeaturesWalkMin, read from the header."""
    text = open(os.path.join(ROOT, "raytracing_simple_amd", "csrc", "rt_instance.h")).read()
    return int(re.search(r"constexpr uint32_t kFeaturesWalkMin = (\d+);", text).group(1))


def small_and_large(n_small, n_large, seed=11):
    """n_small spheres a camera at ORIG sees in front of it, then n_large far larger ones behind them that leave sky between and above."""
    rng = np.random.default_rng(seed)
    sph = np.zeros(n_small + n_large, api.SPHERE_DT)
    sph["rad"][:n_small] = rng.uniform(0.7, 1.9, n_small).astype(F)
    sph["p"][:n_small] = np.stack([rng.uniform(-24, 24, n_small), rng.uniform(-14, 14, n_small), rng.uniform(-12, 12, n_small)], 1).astype(F)
    sph["c"] = rng.uniform(0.1, 0.9, (len(sph), 3)).astype(F)
    big = [(40.0, (-60.0, 10.0, -120.0)), (50.0, (70.0, -25.0, -140.0)), (30.0, (5.0, 55.0, -100.0))]
    for k in range(n_large):
        sph["rad"][n_small + k], sph["p"][n_small + k] = big[k]
    sph["e"][n_small - 1] = (2.0, 1.0, 0.5)         # (a light among the small ones: the albedo word adds emission)
    return sph


def doubled(sph, which, seed=5):
    """`sph` with the records `which` repeated behind it in another colour: exact ties in distance, and records that stay out of the tree."""
    rng = np.random.default_rng(seed)
    again = sph[list(which)].copy()
    again["c"] = rng.uniform(0.1, 0.9, (len(again), 3)).astype(F)
    return np.concatenate([sph, again])


def camera(w, h, orig=ORIG, target=TARGET):
    return np.array(host.compute_camera(orig, target, w, h), F).reshape(-1).copy()


def seen(sph, w=41, h=23):
    """Scene indices the plane at w x h shows, most pixels first (what a doubled record must be one of)."""
    ids = api.features_planes(sph, camera(w, h), w, h)[..., 7].view(np.uint32).reshape(-1)
    vals, counts = np.unique(ids[ids != 0xFFFFFFFF], return_counts=True)
    return [int(v) for v in vals[np.argsort(-counts)]]


SCENES = ["two_sizes", "doubled", "smallest", "inside", "away", "nonfinite", "camera_nonfinite"]


def scene(name, w, h):
    """(records, camera) of a named case at w x h."""
    base = small_and_large(64, 3)
    if name == "two_sizes":                     # always-list and tree
        return base, camera(w, h)
    if name == "doubled":                       # eight visible small records and one large one again: ties, repeats out of the tree and out of the always-list
        return doubled(base, [k for k in seen(base) if k < 64][:7] + [64]), camera(w, h)
    if name == "smallest":                      # 56 small spheres and nothing else: the smallest scene that gets a hierarchy
        return small_and_large(BVH_MIN, 0), camera(w, h)
    if name == "inside":                        # the camera inside a sphere of the tree: every ray leaves through it by the second root
        k = int(np.argmax(base["rad"][:64]))
        return base, camera(w, h, tuple(float(v) for v in base["p"][k]), (0.0, 0.0, -30.0))
    if name == "away":                          # all sky
        return base, camera(w, h, ORIG, (0.0, 0.0, 100.0))
    if name == "nonfinite":                     # a NaN centre (never hit; outside the tree) and a radius of 0 (inside it)
        sph = base.copy()
        sph["p"][10, 0] = np.nan
        sph["rad"][20] = 0.0
        return sph, camera(w, h)
    if name == "camera_nonfinite":              # an infinite image axis: no ray is finite, the pad is infinite, every lane visits everything
        cam = camera(w, h)
        cam[9] = np.inf
        return base, cam
    raise KeyError(name)


def many(n):
    """tools/bvh_scenes.py _many_spheres(n) and its camera: 1 600 spheres are shaped by surface area on the device, 8 200 halved on the host and copied."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bvh_scenes import _many_spheres
    sph, orig, target = _many_spheres(n)
    return sph, orig, target


def lds_of(n_leaves, n_slots, depth):
    """csrc/rt_instance.h features_lds: (everything staged, the pairs staged, nothing but header and stacks)."""
    stacks = (2 * depth * 256 + 15) // 16 * 16
    return 16 * (2 + 4 * (n_leaves - 1) + n_slots) + stacks, 16 * (2 + 4 * (n_leaves - 1)) + stacks, 32 + stacks
