#!/usr/bin/env python3
"""What the rule that picks a launch's instance (csrc/rt_instance.h pick_shape) reads of real scenes, and the kernel the library picked for them:
one pass at 64x48 of each scene below on a default context of the diagnostics library, then the hierarchy's counts (rt_debug_read_bvh) and
rt_last_kernel.  One JSON row per scene: the SceneFacts members, the passes of the launch, the form the launch had and the kernel's symbol.
The form is read off the kernel, because only the context knows it: an instance that walks the hierarchy was launched as Walk (a scene with a
hierarchy starts on it: rt_choice.h), anything else of such a scene as Sweep; a scene below twelve spheres is in the cooperative-or-plain
measurement, whose first arm is the cooperative instance (SweepCoop), and any other scene is launched as Sweep.
tools/sanitize/instance_main.cpp carries the rows as literals and holds pick_shape to them.

    python tools/record_instance_facts.py > profiles/r29_instance_facts.jsonl"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_scenes  # noqa: E402
from raytracing_simple_amd import api, host, scenes  # noqa: E402

W, H, PASSES = 64, 48, 1
SCENES = [("random_spheres(1024)", lambda: scenes.random_spheres(1024)),
          ("_many_spheres(2000)", lambda: bvh_scenes._many_spheres(2000)),
          ("_many_spheres(5000)", lambda: bvh_scenes._many_spheres(5000)),
          ("_many_spheres(9500)", lambda: bvh_scenes._many_spheres(9500)),
          ("mirror_box(120)", lambda: scenes.mirror_box(120)),
          ("mirror_box(64)", lambda: scenes.mirror_box(64)),
          ("demo_plus(16)", lambda: scenes.demo_plus(16)),
          ("Demo", lambda: (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET))]


def main():
    for name, make in SCENES:
        sph, orig, target = make()
        sph = api.as_spheres(sph)
        with api.RtContext(W, H, diag=True) as ctx:
            ctx.set_scene(sph)
            ctx.set_camera(host.compute_camera(orig, target, W, H))
            ctx.render_pass(PASSES)
            kernel = ctx.last_kernel
            cnt = np.zeros(4, np.uint32)
            ctx._check(ctx._lib.rt_debug_read_bvh(ctx._h, None, 0, cnt.ctypes.data_as(C.c_void_p)))
        n_always, n_leaves, depth = int(cnt[0]), int(cnt[1]), int(cnt[2])
        has = n_leaves > 0
        n_lights = int(np.count_nonzero((sph["e"][:, 0] != 0) | (sph["e"][:, 2] != 0)))      # (the reference's zero test looks at x and z only)
        if "_pairs" in kernel:
            form = "Walk"
        elif len(sph) < 12:
            form = "SweepCoop" if "_coop" in kernel else "SweepPlain"
        else:
            form = "Sweep"
        print(json.dumps({"scene": name, "n_spheres": int(len(sph)), "n_lights": n_lights, "has_hierarchy": has, "n_always": n_always,
                          "n_leaves": n_leaves, "n_slots": n_always + 8 * n_leaves if has else 0, "stack_depth": depth, "n_top": 0, "packed_at": 0,
                          "passes": PASSES, "form": form, "kernel": kernel}), flush=True)


if __name__ == "__main__":
    main()
