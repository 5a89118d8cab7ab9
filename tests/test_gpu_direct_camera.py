"""RT_OPT_DIRECT_CAMERA (rt_trace.inc.h, the plain sweep instances rt_trace_parity_w1 / rt_trace_fast_w1): a wavefront whose tile
can reach at most a few spheres (csrc/rt_candidates.h) runs the loop rotated -- camera rays resolved lane by lane against those
candidates, the wave-wide sweep left to bounce rays -- and every other wavefront keeps the old order.  Which spheres a camera ray is
tested against must be invisible: pixels, the colour plane, the final seeds and the five work counters stay bit-equal to the oracle --
across launches, on ragged images, on shards, with records the certificate must not clear (camera inside a sphere, NaN), at every
threshold and against the loop's old form; the cooperative instances (old loop only) and a 65-sphere scene ride along."""
import os

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host, scenes
from raytracing_simple_amd import dist as rdist

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 320, 184


def _gpu(sph, cam, w, h, passes, mode=api.RT_MODE_PARITY, direct=None, kernel=None, no_bvh=False, **shard):
    """The frame after the launches `passes` (a list of pass counts).  `kernel`: the instance that must have rendered it -- on a scene of
    4 .. 11 spheres the library measures the cooperative instance against the plain one, so a test that names one sets the threshold by hand."""
    plain = kernel is not None and kernel.endswith(("parity_w1", "fast_w1"))
    with api.RtContext(w, h, diag=plain or direct is not None or no_bvh or mode >= 100, **shard) as ctx:
        if plain:                       # (0 = the cooperative instances never: the plain one whatever the sphere count)
            ctx._check(ctx._lib.rt_debug_set_coop_min(ctx._h, 0))
        if no_bvh:
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 0, 0))
        if direct is not None:
            ctx._check(ctx._lib.rt_debug_set_direct_camera(ctx._h, direct))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.set_mode(mode)
        for n in passes:
            px = ctx.render_pass(n)
        got = {"pixels": px, "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        if kernel is not None:
            assert ctx.last_kernel == kernel, ctx.last_kernel
        return got


def _same(got, want, stats=True):
    assert np.array_equal(got["pixels"], want["pixels"])
    assert np.array_equal(got["colors"].view(np.uint32), want["colors"].view(np.uint32))
    assert np.array_equal(got["seeds"], want["seeds"])
    if stats:
        g, o = got["stats"], want["stats"]
        assert (g["samples"], g["closest_rays"], g["shadow_rays"], g["sphere_tests"], g["rng_draws"]) == \
               (o["samples"], o["closest_calls"], o["shadow_calls"], o["sphere_tests"], o["rng_draws"])


def _same_gpu(a, b):
    assert np.array_equal(a["pixels"], b["pixels"])
    assert np.array_equal(a["colors"].view(np.uint32), b["colors"].view(np.uint32))
    assert np.array_equal(a["seeds"], b["seeds"])
    assert a["stats"] == b["stats"] or {k: a["stats"][k] for k in ("samples", "closest_rays", "shadow_rays", "sphere_tests", "rng_draws")} == \
        {k: b["stats"][k] for k in ("samples", "closest_rays", "shadow_rays", "sphere_tests", "rng_draws")}


@pytest.fixture(scope="module")
def demo():
    sph = host.demo_scene()
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, W, H)
    return sph, cam, O.render(sph, cam, W, H, 8)


@pytest.fixture(scope="module")
def demo_gpu(demo):
    sph, cam, _ = demo
    return _gpu(sph, cam, W, H, [8], kernel="rt_trace_parity_w1")


def test_demo_frame(demo, demo_gpu):
    _same(demo_gpu, demo[2])


def test_demo_frame_in_two_launches(demo):
    sph, cam, want = demo
    _same(_gpu(sph, cam, W, H, [3, 5], kernel="rt_trace_parity_w1"), want)


def test_ragged_image_edge_tiles_with_invalid_lanes():
    w, h = 323, 181
    sph = host.demo_scene()
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    _same(_gpu(sph, cam, w, h, [4], kernel="rt_trace_parity_w1"), O.render(sph, cam, w, h, 4))


def test_two_shards_assemble_to_the_unsharded_frame(demo):
    """both ranks on the plain instance: the prologue classifies a rank's tiles by their IMAGE rows"""
    sph, cam, want = demo
    parts, total = [], {}
    for r in range(2):
        got = _gpu(sph, cam, W, H, [8], kernel="rt_trace_parity_w1", rank=r, nranks=2, tile_rows=8)
        parts.append(got["pixels"])
        for k, v in got["stats"].items():
            total[k] = total.get(k, 0) + v
    assert np.array_equal(rdist.assemble_numpy(parts, H, W, 2, 8), want["pixels"])
    o = want["stats"]
    assert (total["samples"], total["closest_rays"], total["shadow_rays"], total["sphere_tests"], total["rng_draws"]) == \
           (o["samples"], o["closest_calls"], o["shadow_calls"], o["sphere_tests"], o["rng_draws"])


def test_demo_frame_on_the_cooperative_instance(demo):
    sph, cam, want = demo
    with api.RtContext(W, H, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_coop_min(ctx._h, 4))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        px = ctx.render_pass(8)
        got = {"pixels": px, "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == "rt_trace_parity_coop_w1", ctx.last_kernel
    _same(got, want)


def test_sixteen_spheres_cooperative_instance():
    sph, orig, target = scenes.demo_plus(16)
    cam = host.compute_camera(orig, target, W, H)
    _same(_gpu(sph, cam, W, H, [4], kernel="rt_trace_parity_coop_w1"), O.render(sph, cam, W, H, 4))


@pytest.mark.parametrize("count", [64, 65])
def test_sixty_four_and_sixty_five_spheres(count):
    """the plain instance at the certificate's limit: 64 spheres are classified (one lane, one bit each), 65 are not and every wavefront
    runs the old loop (the hierarchy and the cooperative instances switched off so that rt_trace_parity_w1 renders)"""
    sph, orig, target = scenes.random_spheres(count)
    cam = host.compute_camera(orig, target, 160, 96)
    _same(_gpu(sph, cam, 160, 96, [2], kernel="rt_trace_parity_w1", no_bvh=True), O.render(sph, cam, 160, 96, 2))


@pytest.mark.parametrize("k,threshold", [(1, 4), (2, 4), (5, 4), (3, 4), (7, 3)])
def test_adversarial_fixture(k, threshold):
    """on the plain instance -- 1, 5: the camera inside a sphere; 2: NaN and infinite records; 3: the camera on a surface, a negative radius;
    7: three spheres, every tile rotated"""
    rec = np.load(os.path.join(GOLDEN, "fuzz_candidates.npy"))[k]
    sph = rec["spheres"][:int(rec["n"])].copy()
    cam = host.compute_camera(tuple(float(v) for v in rec["orig"]), tuple(float(v) for v in rec["target"]), 64, 40)
    with np.errstate(all="ignore"):
        _same(_gpu(sph, cam, 64, 40, [3], kernel="rt_trace_parity_w1", no_bvh=True, direct=threshold), O.render(sph, cam, 64, 40, 3))


def test_fast_mode_against_the_swept_form(demo, demo_gpu):
    """fast mode's criterion (PSNR >= 50 dB against parity at equal spp), and the direct form against fast mode with every camera ray swept"""
    sph, cam, _ = demo
    direct = _gpu(sph, cam, W, H, [8], mode=api.RT_MODE_FAST, kernel="rt_trace_fast_w1")
    swept = _gpu(sph, cam, W, H, [8], mode=api.RT_MODE_FAST, direct=-1, kernel="rt_trace_fast_w1")
    assert O.psnr(direct["pixels"], swept["pixels"]) >= 50.0
    assert O.psnr(direct["pixels"], demo_gpu["pixels"]) >= 50.0
    assert direct["stats"]["samples"] == swept["stats"]["samples"]


def test_old_form_instance_renders_the_same_frame(demo, demo_gpu):
    sph, cam, _ = demo
    old = _gpu(sph, cam, W, H, [8], mode=api.instance_mode("rt_trace_parity_w1_sweptcam"), kernel="rt_trace_parity_w1_sweptcam")
    _same_gpu(old, demo_gpu)


@pytest.mark.parametrize("threshold", [-1, 0, 1, 2, 4])
def test_fallback_threshold_is_invisible(demo, threshold):
    """-1: every wavefront runs the old loop; 0: all but those of sky tiles; 1, 2: silhouette tiles do"""
    sph, cam, want = demo
    _same(_gpu(sph, cam, W, H, [8], direct=threshold, kernel="rt_trace_parity_w1"), want)


def test_four_wavefront_cooperative_instance():
    """rt_trace_parity_coop (32x8 workgroups: wavefront k of a workgroup owns columns 8k .. 8k + 7 of its tile)"""
    sph, orig, target = scenes.demo_plus(16)
    cam = host.compute_camera(orig, target, 200, 120)
    with api.RtContext(200, 120, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_wg_waves(ctx._h, 4))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        px = ctx.render_pass(3)
        got = {"pixels": px, "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == "rt_trace_parity_coop", ctx.last_kernel
    _same(got, O.render(sph, cam, 200, 120, 3))


@pytest.mark.parametrize("threshold", [-1, 2, 4])
def test_plain_instance_on_tiles_above_the_threshold(threshold):
    """the 16-sphere scene on the plain instance (cooperative any-hit switched off): tiles with up to 5 candidates, so wavefronts of BOTH
    loop orders in one launch at 2 and 4, and the old order everywhere at -1"""
    sph, orig, target = scenes.demo_plus(16)
    cam = host.compute_camera(orig, target, 200, 120)
    with api.RtContext(200, 120, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_coop_min(ctx._h, 0))
        ctx._check(ctx._lib.rt_debug_set_direct_camera(ctx._h, threshold))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        px = ctx.render_pass(3)
        got = {"pixels": px, "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == "rt_trace_parity_w1", ctx.last_kernel
    _same(got, O.render(sph, cam, 200, 120, 3))
