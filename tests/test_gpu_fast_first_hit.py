"""The shipped fast kernels' closest-hit decision for camera rays, ray by ray against binary64 (tests/_first_hit.py): one pass of every
rt_trace_fast_* instance over a scene in which every sphere is an emitter that carries its own index, 96x64 pixels = 6144 camera rays,
the colour plane decoded and held -- hit or miss, the index of the winner, |n.d| within its running-error envelope -- wherever the
exclusion rule decides the ray; K = R.K.measured(), at most 2 % of a scene's pixels left out.  This sees what the probe of
tests/test_gpu_fast_rays.py cannot: each instance's OWN fusing, the rotated candidate loop of RT_OPT_DIRECT_CAMERA, and the hierarchy
walk in its three table placements.  The same frames from the oracle under K.exact(), and a tampered frame that must fail:
tests/test_fast_first_hit_cpu.py.  Run with -s for the figures (recorded in profiles/r26_fast_first_hit.jsonl).

WHICH MACHINE CODE.  The diagnostics library's instances are another compile of the same source than the product library's, so each
case says whose it holds:
  PRODUCT library (librt_hip.so, the scene alone selects the instance):
    rt_trace_fast_coop_w1   demo_plus(16)
    rt_trace_fast_pairs     random_spheres(256) -- not 1024: with every record a light the staged light tables (32 bytes a record) push the
                            1024-sphere tree past the walk's LDS budget, and the library walks it with rt_trace_fast_pairs_m
    rt_trace_fast_pairs_m   random_spheres(1024) and _many_spheres(2000)
    rt_trace_fast_pairs_g   _many_spheres(5000)
  DIAGNOSTICS library (librt_hip_diag.so, a knob reaches the instance):
    rt_trace_fast_w1        the Demo scene (6 spheres; rt_debug_set_coop_min(ctx, 0): on 4 .. 11 spheres the product measures coop against
                            plain and its first launch is the cooperative arm), random_spheres(64) and (65) with the hierarchy off -- either
                            side of the candidate masks' width: 64 are classified and the rotated loop resolves the camera rays of the tiles
                            with few candidates, 65 are not and every ray is swept
    rt_trace_fast_coop      demo_plus(16) with rt_debug_set_wg_waves(ctx, 4)
    rt_trace_fast_pairs     random_spheres(1024), the hierarchy forced (rt_debug_set_walk(ctx, 0, 0, 1)) with its whole tables staged
    rt_trace_fast_g         random_spheres(1024) and _many_spheres(5000) with the hierarchy off (rt_debug_set_bvh(ctx, 0, 0)): with every
                            record a light both tables lie beyond the sweep's LDS budget
The three frames of the 1024-sphere scene face one reference, and so do the two of the 5000-sphere scene."""
import pytest

import _fast_reference as R
import _first_hit as FH

pytestmark = pytest.mark.gpu

NO_COOP = ("rt_debug_set_coop_min", (0,))
NO_BVH = ("rt_debug_set_bvh", (0, 0))
WHOLE_TREE_IN_LDS = ("rt_debug_set_bvh", (1, 152 * 1024))
WALK_FORCED = ("rt_debug_set_walk", (0, 0, 1))
FOUR_WAVES = ("rt_debug_set_wg_waves", (4,))

# (scene, knobs of the diagnostics library or () for the product library, the instance that must have rendered)
CASES = [
    ("demo", (NO_COOP,), "rt_trace_fast_w1"),
    ("random64", (NO_COOP, NO_BVH), "rt_trace_fast_w1"),
    ("random65", (NO_COOP, NO_BVH), "rt_trace_fast_w1"),
    ("demo_plus16", (), "rt_trace_fast_coop_w1"),
    ("demo_plus16", (FOUR_WAVES,), "rt_trace_fast_coop"),
    ("random256", (), "rt_trace_fast_pairs"),
    ("random1024", (), "rt_trace_fast_pairs_m"),
    ("random1024", (WHOLE_TREE_IN_LDS, WALK_FORCED), "rt_trace_fast_pairs"),
    ("random1024", (NO_BVH,), "rt_trace_fast_g"),
    ("many2000", (), "rt_trace_fast_pairs_m"),
    ("many5000", (), "rt_trace_fast_pairs_g"),
    ("many5000", (NO_BVH,), "rt_trace_fast_g"),
]
SHIPPED = {"rt_trace_fast_w1", "rt_trace_fast_coop_w1", "rt_trace_fast_coop", "rt_trace_fast_pairs", "rt_trace_fast_pairs_m",
           "rt_trace_fast_pairs_g", "rt_trace_fast_g"}


def _case_id(case):
    return "%s-%s-%s" % (case[2].replace("rt_trace_fast_", ""), case[0], "diagnostics" if case[1] else "product")


@pytest.fixture(scope="module")
def measured():
    if R.K.measured() is None:
        pytest.skip("not measured yet: profiles/r20_fast_blocks.jsonl has no record (tools/measure_fast_blocks.py writes it)")
    return True


def test_every_shipped_fast_instance_is_a_case():
    assert {c[2] for c in CASES} == SHIPPED
    assert {c[2] for c in CASES if not c[1]} == {"rt_trace_fast_coop_w1", "rt_trace_fast_pairs", "rt_trace_fast_pairs_m", "rt_trace_fast_pairs_g"}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_first_hits_of_a_shipped_fast_instance_against_binary64(measured, case):
    name, knobs, kernel = case
    colors, rendered_by = FH.render(name, knobs=knobs)
    assert rendered_by == kernel, (name, rendered_by)
    FH.check_frame("%s / %s (%s)" % (kernel, name, "diagnostics" if knobs else "product"), colors, FH.reference(name, True))
