#!/usr/bin/env python3
"""What measuring cooperative any-hit against plain INSIDE a small scene's first long frame would cost (rt_choice.h Choice::next_small defers it to the
second frame): the Demo scene and the reference's simple.scn, first frame of 64 passes on a fresh context --
  as the library does it   the first frame whole (pricing launch + the rest), the second frame split for the four probe launches, the third decided
  probes in frame 1        emulated with the library's own pieces: the passes of the four probe launches as separate short calls first (they ARE the
                           probes for short launches), then the rest of the frame in one call
Device time between the events around everything the frame launched is not observable across calls, so both are timed as wall clock around blocking
calls on a warm GPU; per frame: launches, kernel the frame ended on, ms."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402
from tools import reference_scenes  # noqa: E402

SPP = 64


def frames(ctx, split_first):
    out = []
    for k in range(4):
        ctx.reset()
        t0 = time.perf_counter()
        if k == 0 and split_first:
            for n in (1, 4, 1, 4):
                ctx.render_pass(n, copy=False)
            ctx.render_pass(SPP - 10, copy=False)
        else:
            ctx.render_pass(SPP, copy=False)
        out.append({"frame": k + 1, "wall_ms": round((time.perf_counter() - t0) * 1e3, 4), "launches": int(ctx.stats()["launches"]), "kernel": ctx.last_kernel})
    return out


def main():
    for name, (sph, orig, target), w, h in (("demo 1080p", (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET), 1920, 1080),
                                           ("simple.scn 800x600", reference_scenes.load_scene("simple"), 800, 600)):
        cam = host.compute_camera(orig, target, w, h)
        with api.RtContext(w, h) as warm:                      # GPU warm, code objects loaded
            warm.set_scene(sph); warm.set_camera(cam); warm.render_pass(SPP, copy=False)
        for split_first in (False, True):
            best = None
            for _ in range(5):                                  # fresh context each time; the fastest of five (host jitter)
                with api.RtContext(w, h) as ctx:
                    ctx.set_scene(sph); ctx.set_camera(cam)
                    f = frames(ctx, split_first)
                if best is None or f[0]["wall_ms"] < best[0]["wall_ms"]:
                    best = f
            print(json.dumps({"scene": name, "spp": SPP, "probes": "inside the first frame (emulated: the probe passes as short calls)" if split_first
                              else "as the library does it: first frame whole, second frame split", "frames": best, "build_id": api.build_id()}), flush=True)


if __name__ == "__main__":
    main()
