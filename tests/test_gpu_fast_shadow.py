"""The shipped fast kernels' shadow rays, pixel by pixel and light by light against binary64 (tests/_shadow_frames.py): one pass of every
rt_trace_fast_* instance over a scene with ONE white diffuse receiver, a red and a blue light and black occluders, 96x64 pixels.  On the
receiver's pixels a channel is nonzero exactly where sample_light wanted a shadow ray and the any-hit sweep found no blocker, and then it
is 8 * rt_div(numer, len * len): lit or dark must be binary64's wherever the exclusion rule decides the answer, a lit channel must lie
within the running-error envelope of 8 k, a decided dark one must be an exact zero; K = R.K.measured(), at most 2 % of a frame's answers
left out.  This sees what no probe can: sweep_any, coop_any (wave ballot, LDS mailbox, lists split over idle lanes), sweep_both (the last
light's shadow ray on the bounce ray's sweep), the walk's any-hit in its three table placements and rt_div, each as the shipped instance
compiles it.  The same frames from the oracle under K.exact(), the cap and the vacuity guards on the reference alone, tampered frames
that must fail: tests/test_shadow_frames_cpu.py.  Run with -s for the figures (recorded in profiles/r28_shadow_frames.jsonl).

WHICH MACHINE CODE.  With two lights the light tables are small, so which scene reaches which instance differs from the first-hit frames
(tests/test_gpu_fast_first_hit.py); the table below was read off the device.  The diagnostics library's instances are another compile of
the same source than the product library's, so each case says whose it holds (CASES: () = the product library, knobs = diagnostics).
  PRODUCT library (librt_hip.so, the scene alone selects the instance):
    rt_trace_fast_coop_w1   demo_plus(16): coop_any with several rays of a wavefront pending, one wavefront per workgroup
    rt_trace_fast_pairs     random_spheres(256): the walk's any-hit, its tables in LDS
    rt_trace_fast_pairs_m   _many_spheres(2000): the pairs staged, the slots in HBM / L2
    rt_trace_fast_pairs_g   _many_spheres(5000): everything in HBM / L2
  DIAGNOSTICS library (librt_hip_diag.so, a knob reaches the instance):
    rt_trace_fast_w1        random_spheres(64) and (65), hierarchy and cooperative any-hit off.  64: the camera rays are classified and the
                            wavefronts of tiles with at most three candidates run the rotated loop -- the earlier light through sweep_any, the
                            later one through sweep_both (99 % of the frame's decided answers lie on such tiles: tests/test_shadow_frames_cpu.py);
                            65: no classification, every wavefront runs the old loop, both lights through sweep_any
    rt_trace_fast_coop      demo_plus(16) with rt_debug_set_wg_waves(ctx, 4): four wavefronts, each with its own LDS mailbox; and
                            random_spheres(256) with the hierarchy off: lists of 256 records split over the idle lanes
    rt_trace_fast_pairs_m, rt_trace_fast_pairs_g   random_spheres(256) with the walk forced and the hierarchy's LDS budget set to 8000 and to
                            3000 bytes (the device chose _pairs down to 12 000, _pairs_m at 9000 and 7000, _pairs_g from 5000 down)
    rt_trace_fast_g         _many_spheres(5000) with the hierarchy off: the plain sweep through the scalar cache (with two lights the sweep
                            stages tables of up to 2556 records; the 2000-sphere scene without its hierarchy is rt_trace_fast_coop's)
The frames of one scene face one reference.

PARITY CONTROL.  The same frame from parity mode must equal the oracle's bit for bit -- colours, seeds, counters: the transformed, scaled
scene is what the reference saw."""
import numpy as np
import pytest

import _fast_reference as R
import _oracle as O
import _shadow_frames as SF

pytestmark = pytest.mark.gpu

NO_COOP = ("rt_debug_set_coop_min", (0,))
NO_BVH = ("rt_debug_set_bvh", (0, 0))
FOUR_WAVES = ("rt_debug_set_wg_waves", (4,))
WALK_FORCED = ("rt_debug_set_walk", (0, 0, 1))
PAIRS_ONLY_IN_LDS = ("rt_debug_set_bvh", (1, 8000))      # random_spheres(256): the whole tables need more than 9000 bytes of LDS, the pairs alone fewer than 7000
NOTHING_IN_LDS = ("rt_debug_set_bvh", (1, 3000))

# (scene, knobs of the diagnostics library or () for the product library, the instance that must have rendered)
CASES = [
    ("random64", (NO_COOP, NO_BVH), "rt_trace_fast_w1"),
    ("random65", (NO_COOP, NO_BVH), "rt_trace_fast_w1"),
    ("demo_plus16", (), "rt_trace_fast_coop_w1"),
    ("demo_plus16", (FOUR_WAVES,), "rt_trace_fast_coop"),
    ("random256", (NO_BVH,), "rt_trace_fast_coop"),
    ("random256", (), "rt_trace_fast_pairs"),
    ("random256", (PAIRS_ONLY_IN_LDS, WALK_FORCED), "rt_trace_fast_pairs_m"),
    ("random256", (NOTHING_IN_LDS, WALK_FORCED), "rt_trace_fast_pairs_g"),
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
    assert {c[0] for c in CASES} == set(SF.SCENES)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_shadow_rays_of_a_shipped_fast_instance_against_binary64(measured, case):
    name, knobs, kernel = case
    colors, rendered_by, _, _ = SF.render(name, knobs=knobs)
    assert rendered_by == kernel, (name, rendered_by)
    SF.check_frame("%s / %s (%s)" % (kernel, name, "diagnostics" if knobs else "product"), colors, SF.reference(name, True))


@pytest.mark.parametrize("name", list(SF.SCENES))
def test_parity_mode_renders_the_oracle_s_frame_bit_for_bit(name):
    sph, cam, _, _ = SF.scene(name)
    colors, rendered_by, seeds, stats = SF.render(name, fast=False)
    assert rendered_by.startswith("rt_trace_parity"), rendered_by
    want = O.render(sph, cam, SF.W, SF.H, 1, threads=16)
    assert R.bits_equal(colors, want["colors"]).all(), (name, int((~R.bits_equal(colors, want["colors"])).sum()))
    assert np.array_equal(seeds, want["seeds"]), name
    g, o = stats, want["stats"]
    assert (g["samples"], g["closest_rays"], g["shadow_rays"], g["sphere_tests"], g["rng_draws"]) == \
           (o["samples"], o["closest_calls"], o["shadow_calls"], o["sphere_tests"], o["rng_draws"]), name
