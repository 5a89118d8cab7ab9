"""Scenes the hierarchy's builders are held to (tests/test_gpu_bvh.py, tools/bvh_check.py digests): adversarial records, repeated
records, slabs of thousands of small spheres, two size classes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raytracing_simple_amd import api, host  # noqa: E402


def _adversarial(seed):
    """Duplicated spheres (the reference's loader doubles them: exact ties), zero and negative radii, concentric and
    heavily overlapping spheres, a camera inside a glass sphere, non-finite records, a far-away cluster."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([40, 70, 130]))
    sph = np.zeros(n, api.SPHERE_DT)
    sph["rad"] = rng.uniform(0.5, 6.0, n).astype(np.float32)
    sph["p"] = rng.uniform(-30, 30, (n, 3)).astype(np.float32)
    sph["c"] = rng.uniform(0.1, 0.95, (n, 3)).astype(np.float32)
    sph["refl"] = rng.integers(0, 3, n)
    sph["rad"][0], sph["p"][0], sph["refl"][0] = 1000.0, (0, -1030, 0), 0          # ground
    sph["rad"][1], sph["p"][1], sph["e"][1] = 8.0, (0, 45, 0), (10, 10, 10)         # light
    half = n // 2
    dup = rng.integers(2, half, 8)
    sph[half:half + 8] = sph[dup]                                                   # exact duplicates, higher index
    sph["rad"][half + 8] = 0.0
    sph["rad"][half + 9] = -3.0                                                      # rad*rad is what the test uses
    sph["p"][half + 10] = sph["p"][half + 11]                                        # concentric
    sph["rad"][half + 12] = np.float32("nan")
    sph["p"][half + 13, 1] = np.float32("inf")
    sph["p"][half + 14] = (4000.0, 10.0, -3000.0)                                    # far-away member of the tree
    orig = (float(sph["p"][3, 0]), float(sph["p"][3, 1]), float(sph["p"][3, 2]) + 0.5) if seed % 2 else (10.0, 30.0, 70.0)
    if seed % 2:
        sph["refl"][3], sph["rad"][3] = 2, 5.0                                       # the camera sits inside glass
    return sph, orig, (0.0, 5.0, 0.0)


def _with_repeats(seed):
    """A scene in which later records repeat earlier ones bit for bit in centre and radius^2 but NOT in material (a repeated diffuse sphere that
    is glass, black, a light), a repeated light, a repeated ground (always-list), a record with the negated radius (same radius^2) and the
    reference loader's own pattern: a block of zero-radius records at the origin in FRONT of everything (Utility.cpp:120,154)."""
    rng = np.random.default_rng(100 + seed)
    n_real, n_ph = 90, 40
    real = np.zeros(n_real, api.SPHERE_DT)
    real["rad"] = rng.uniform(0.8, 5.0, n_real).astype(np.float32)
    real["p"] = rng.uniform(-30, 30, (n_real, 3)).astype(np.float32)
    real["p"][:, 1] = np.abs(real["p"][:, 1])
    real["c"] = rng.uniform(0.1, 0.95, (n_real, 3)).astype(np.float32)
    real["refl"] = rng.integers(0, 3, n_real)
    real["rad"][0], real["p"][0], real["refl"][0] = 1000.0, (0, -1000, 0), 0         # ground
    real["rad"][1], real["p"][1], real["e"][1], real["refl"][1] = 8.0, (0, 45, 0), (10, 10, 10), 0          # light
    for k, src in enumerate(rng.integers(2, 40, 12)):                                # repeats with OTHER materials, at higher indices
        dst = 60 + k
        real[dst] = real[src]
        real["refl"][dst] = (int(real["refl"][src]) + 1 + k % 2) % 3
        real["c"][dst] = (0.05, 0.9, 0.05)
        if k % 4 == 0:
            real["e"][dst] = (3, 3, 3)                                               # a repeat that is a light (it is sampled as one; never hit)
        if k % 3 == 0:
            real["rad"][dst] = -real["rad"][dst]                                     # same radius^2
    real[75] = real[1]                                                               # the light, repeated
    real[76] = real[0]                                                               # the ground, repeated (always-list)
    real["c"][76] = (0.9, 0.1, 0.1)
    phantoms = np.zeros(n_ph, api.SPHERE_DT)
    return np.concatenate([phantoms, real]), (20.0, 40.0, 90.0), (0.0, 8.0, 0.0)


def _many_spheres(n, seed=7):
    """n small spheres in a slab above a ground sphere, one light: beyond what LDS holds for n > ~9000."""
    rng = np.random.default_rng(seed)
    sph = np.zeros(n, api.SPHERE_DT)
    sph["rad"] = rng.uniform(0.3, 1.2, n).astype(np.float32)
    sph["p"] = np.stack([rng.uniform(-90, 90, n), rng.uniform(0.5, 9, n), rng.uniform(-90, 90, n)], 1).astype(np.float32)
    sph["c"] = rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32)
    sph["refl"] = rng.choice([api.DIFF, api.DIFF, api.SPEC, api.REFR], n)
    sph["rad"][0], sph["p"][0], sph["refl"][0], sph["c"][0] = 1000.0, (0, -1000, 0), api.DIFF, (.75, .75, .75)
    sph["rad"][1], sph["p"][1], sph["e"][1], sph["refl"][1] = 9.0, (0, 70, 0), (14, 14, 14), api.DIFF
    return sph, host.DEMO_ORIG, host.DEMO_TARGET


def _two_size_classes(n_small, n_large, seed=3):
    """Dust among objects fifty times its size, a ground sphere and a light (tools/always_list_probe.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import always_list_probe
    return always_list_probe.two_classes(n_small, n_large, seed)
