"""Feature planes through the hierarchy on the device (include/rt_api.h "feature planes"; csrc/rt_walk.inc.h rt_features_pairs / _pairs_m / _pairs_g,
csrc/rt_instance.h features_form).  Every comparison is of bits: rt_read_features after rt_features_async against rt_features_planes of the same
records and camera -- the function tests/test_gpu_feature_planes.py holds the sweep to -- and rt_last_features_kernel is asserted after every call.
The scenes are tests/_features_walk.py's; tests/test_features_walk_cpu.py shows on the CPU that each contains what it is there for."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

import _features_walk as W
from raytracing_simple_amd import api, host
from test_features_cpu import MISS, assert_same_plane
from test_gpu_atrous import assert_device_is_host as assert_atrous_is_host
from test_gpu_reproject import assert_device_is_host as assert_temporal_is_host, side
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, make

sys.path.insert(0, os.path.join(W.ROOT, "tools"))
import bvh_check  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = "rt_features_kernel"
PLACEMENTS = ["rt_features_pairs", "rt_features_pairs_m", "rt_features_pairs_g"]


def context(sph, cam, w, h, diag=True, mode=None):
    ctx = api.RtContext(w, h, diag=diag)
    ctx.set_scene(sph)
    ctx.set_camera(cam)
    if mode is not None:
        ctx.set_mode(mode)
    return ctx


def force(ctx, form, kernel=None):
    """rt_debug_set_features_form, and -- for a placement -- the LDS limit that gives it, as tests/_launch_matrix.py forces the render instances'."""
    ctx._check(ctx._lib.rt_debug_set_features_form(ctx._h, form))
    if kernel is not None:
        b = bvh_check.read_bvh(ctx)
        everything, pairs, _ = W.lds_of(b["n_leaves"], b["n_slots"], b["stack_depth"])
        assert pairs < everything
        limit = {"rt_features_pairs": 152 * 1024, "rt_features_pairs_m": pairs, "rt_features_pairs_g": 1}[kernel]
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, W.BVH_MIN, limit))


def formed(ctx, kernel, stream=None):
    ctx.features_async(stream)
    assert ctx.last_features_kernel() == kernel
    return ctx.read_features()


# ---- 1. the hierarchy forced, over scenes, sizes and placements ---------------------------------------------------------
CASES = [(name, size) for name in W.SCENES for size in W.SIZES] + [("two_sizes", (96, 64))]


@pytest.mark.parametrize("kernel", PLACEMENTS)
@pytest.mark.parametrize("name,size", CASES, ids=["%s_%dx%d" % (n, s[0], s[1]) for n, s in CASES])
def test_the_hierarchy_forced_equals_features_planes_bit_for_bit(name, size, kernel):
    w, h = size
    sph, cam = W.scene(name, w, h)
    with context(sph, cam, w, h) as ctx:
        assert ctx.last_features_kernel() == ""
        force(ctx, 2, kernel)
        want = api.features_planes(sph, cam, w, h)
        got = formed(ctx, kernel)
        assert_same_plane(got, want)
        assert_same_plane(formed(ctx, kernel, ctx.stream), got)          # again, on the context's stream: the same words
        if name == "away":
            assert (got[..., 7].view(np.uint32) == MISS).all() and not got[..., :7].any()


# ---- 2. trees shaped by each builder -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1600, 8200])
def test_trees_of_both_builders(n):
    """1 600 spheres: shaped by surface area on the device; 8 200: halved on the host and copied (tools/bvh_check.py builder_reached)."""
    w, h = 41, 23
    sph, orig, target = W.many(n)
    cam = host.compute_camera(orig, target, w, h)
    with context(sph, cam, w, h) as ctx:
        force(ctx, 2)
        ctx.features_async()
        assert ctx.last_features_kernel() in PLACEMENTS
        got = ctx.read_features()
        assert_same_plane(got, api.features_planes(sph, cam, w, h))
        assert len(np.unique(got[..., 7].view(np.uint32))) > 50


# ---- 3. the rule unforced -------------------------------------------------------------------------------------------------
def test_the_rule_picks_the_kernel_and_both_give_the_same_words():
    w, h = 41, 23
    least = W.walk_min()
    demo = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    smallest = W.scene("smallest", w, h)
    n_large = max(least, 200)
    large = W.small_and_large(n_large - 3, 3), W.camera(w, h)
    for diag in (False, True):                                # the product library holds the kernels and the rule too
        with context(*demo, w, h, diag=diag) as ctx:
            assert_same_plane(formed(ctx, SWEEP), api.features_planes(*demo, w, h))          # no hierarchy
        with context(*smallest, w, h, diag=diag) as ctx:      # 56 records: below the threshold if it lies above 56
            assert_same_plane(formed(ctx, SWEEP if W.BVH_MIN < least else PLACEMENTS[0]), api.features_planes(*smallest, w, h))
        with context(*large, w, h, diag=diag) as ctx:         # at or above it
            assert_same_plane(formed(ctx, PLACEMENTS[0]), api.features_planes(*large, w, h))
    with context(*large, w, h) as ctx:
        walked = formed(ctx, PLACEMENTS[0]).copy()
        b = bvh_check.read_bvh(ctx)
        everything, pairs, _ = W.lds_of(b["n_leaves"], b["n_slots"], b["stack_depth"])
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, W.BVH_MIN, everything - 1))          # the LDS limit lowered: the slots leave LDS ...
        assert_same_plane(formed(ctx, PLACEMENTS[1]), walked)
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, W.BVH_MIN, pairs - 1))               # ... then the pairs
        assert_same_plane(formed(ctx, PLACEMENTS[2]), walked)
        force(ctx, 1)                                         # forced 1 against forced 2 on the same context
        swept = formed(ctx, SWEEP).copy()
        force(ctx, 2)
        assert_same_plane(formed(ctx, PLACEMENTS[2]), swept)
        assert_same_plane(swept, walked)


# ---- 4. moved spheres ------------------------------------------------------------------------------------------------------
def test_moved_spheres_are_seen_through_the_rebuilt_tree():
    """rt_update_spheres_async, then rt_features_async with no launch in between: the pending rebuild runs before the walk."""
    w, h = 41, 23
    sph, orig, target = W.many(1600)
    cam = host.compute_camera(orig, target, w, h)
    with context(sph, cam, w, h) as ctx:
        force(ctx, 2)
        ctx.features_async()
        kernel = ctx.last_features_kernel()
        assert kernel in PLACEMENTS
        first = ctx.read_features().copy()
        assert_same_plane(first, api.features_planes(sph, cam, w, h))
        ids = first[..., 7].view(np.uint32).reshape(-1)
        vals, counts = np.unique(ids[(ids != MISS) & (ids > 1)], return_counts=True)
        at = int(min(vals[np.argsort(-counts)][:3]))          # ten records from a well-seen one on
        at = min(at, len(sph) - 10)
        moved = sph.copy()
        moved["p"][at:at + 10] += np.float32([3.0, 6.0, -2.0])
        ctx.update_spheres(at, moved[at:at + 10])
        _refused(ctx, RT_ERR_STATE, ctx.read_features)
        got = formed(ctx, kernel)
        assert_same_plane(got, api.features_planes(moved, cam, w, h))
        assert not np.array_equal(got.view(np.uint32), first.view(np.uint32))


# ---- 5. a fast-mode context ---------------------------------------------------------------------------------------------------
def test_a_fast_context_forms_the_same_plane_through_the_same_instance():
    w, h = 41, 23
    sph, cam = W.scene("doubled", w, h)
    with context(sph, cam, w, h, mode=api.RT_MODE_FAST) as ctx:
        force(ctx, 2)
        ctx.render_pass(2)                                    # (fast mode's kernels have run on it)
        assert_same_plane(formed(ctx, PLACEMENTS[0]), api.features_planes(sph, cam, w, h))


# ---- 6. the loop on a large scene ---------------------------------------------------------------------------------------------
def test_the_interactive_loop_on_a_large_scene():
    w, h = 41, 23
    sph, orig, target = W.many(1600)
    camS = host.compute_camera(orig, target, w, h)
    camD = host.compute_camera(tuple(np.float32(orig) + np.float32([1.5, 0.5, 0.0])), target, w, h)
    with context(sph, camS, w, h) as S, context(sph, camD, w, h) as D:
        for ctx in (S, D):
            force(ctx, 2)
        S.render_async(1)
        S.features_async()
        D.seed_stream(2)
        D.render_async(1)
        D.features_async()
        assert S.last_features_kernel() in PLACEMENTS and D.last_features_kernel() == S.last_features_kernel()
        D.reproject_async(S)
        T = assert_temporal_is_host(D, api.reproject_planes(side(D, sph, camD), side(S, sph, camS), w, h))
        assert (T[..., 3] > 1.0).mean() > 0.3                 # history was taken: the planes of both contexts agree about what is where
        D.atrous_async()
        assert_atrous_is_host(D, api.atrous_planes(T, api.features_planes(sph, camD, w, h), w, h))
        assert S.last_features_kernel() in PLACEMENTS and D.last_features_kernel() in PLACEMENTS


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_what_is_refused():
    w, h = 41, 23
    demo, cam = host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    with contextlib.ExitStack() as stack:
        ctx = stack.enter_context(context(demo, cam, w, h))
        want = api.features_planes(demo, cam, w, h)
        assert_same_plane(formed(ctx, SWEEP), want)
        force(ctx, 2)                                         # the hierarchy forced on a scene without one
        assert "hierarchy" in _refused(ctx, RT_ERR_STATE, ctx.features_async)
        assert ctx.last_features_kernel() == SWEEP
        assert_same_plane(ctx.read_features(), want)          # the previous plane stays current
        lib = ctx._lib
        for bad in (-1, 3, 100):
            assert lib.rt_debug_set_features_form(ctx._h, bad) == RT_ERR_ARG
        assert lib.rt_debug_set_features_form(None, 0) == RT_ERR_ARG
        _refused(ctx, RT_ERR_STATE, ctx.features_async)       # (a refused knob changed nothing: still forced)
        force(ctx, 0)
        assert_same_plane(formed(ctx, SWEEP), want)
        shard = stack.enter_context(make("demo", w, h, rank=1, nranks=2))
        multi = stack.enter_context(make("demo", w, h, devices=[0, 0]))
        for x in (shard, multi):                              # refused exactly as before
            _refused(x, RT_ERR_ARG, x.features_async)
            _refused(x, RT_ERR_ARG, x.read_features)
            assert x.last_features_kernel() == ""
