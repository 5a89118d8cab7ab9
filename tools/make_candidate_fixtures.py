#!/usr/bin/env python3
"""`python tools/make_candidate_fixtures.py`: writes tests/golden/fuzz_candidates.npy -- the adversarial scenes the tile
certificate (csrc/rt_candidates.h) is held to by tests/test_tile_candidates.py and tests/test_gpu_direct_camera.py: cameras
inside spheres, zero, tiny and huge radii, far-away spheres, NaN and infinite records.  One record per scene: { n, orig, target,
spheres[64] } (the first n sphere records count).  Seeded: the file is reproducible."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api  # noqa: E402


def scene(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([3, 6, 9, 12, 20, 33, 64]))
    sph = np.zeros(n, api.SPHERE_DT)
    kind = rng.integers(0, 10, n)
    sph["rad"] = np.where(kind == 0, 0.0, np.where(kind == 1, 1e-4, np.where(kind == 2, 5e3, rng.uniform(0.5, 25.0, n)))).astype(np.float32)
    sph["p"] = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    sph["p"][kind == 3] *= np.float32(1e4)
    sph["c"] = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    sph["refl"] = rng.choice([api.DIFF, api.DIFF, api.SPEC, api.REFR], n)
    sph["e"][int(rng.integers(0, n))] = rng.uniform(2.0, 20.0, 3).astype(np.float32)
    orig = rng.uniform(-80, 80, 3).astype(np.float32)
    if seed % 4 == 1:                                   # the camera inside sphere 0
        sph["rad"][0] = np.float32(15.0)
        orig = (sph["p"][0] + np.float32(0.25) * sph["rad"][0]).astype(np.float32)
    if seed % 4 == 2:                                   # NaN and infinite records
        sph["p"][1] = (np.nan, 1.0, 2.0)
        sph["rad"][2] = np.nan
        if n > 4:
            sph["p"][4] = (np.inf, 0.0, 0.0)
    if seed % 4 == 3:                                   # the camera ON a sphere's surface, and a negative radius
        sph["rad"][0] = np.float32(10.0)
        orig = (sph["p"][0] + np.array([10.0, 0.0, 0.0], np.float32)).astype(np.float32)
        sph["rad"][1] = np.float32(-3.0)
    target = rng.uniform(-10, 10, 3).astype(np.float32)
    return sph, orig, target


if __name__ == "__main__":
    out = np.zeros(8, np.dtype([("n", "<i4"), ("orig", "<f4", 3), ("target", "<f4", 3), ("spheres", api.SPHERE_DT, 64)]))
    for k in range(8):
        sph, orig, target = scene(k)
        out[k]["n"] = len(sph)
        out[k]["orig"] = orig
        out[k]["target"] = target
        out[k]["spheres"][:len(sph)] = sph
    np.save(os.path.join(ROOT, "tests", "golden", "fuzz_candidates.npy"), out)
    print("wrote 8 scenes")
