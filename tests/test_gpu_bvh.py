"""Large scenes: the hierarchy over the small spheres (csrc/rt_device.h BvhTables, rt_walk.inc.h).  It only selects
which spheres a ray is tested against, so everything must stay BIT-EXACT: frames, colour plane, seeds and the work
counters against the oracle, with the hierarchy forced on small and adversarial scenes too."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host, scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bvh_check  # noqa: E402
from bvh_scenes import _adversarial, _many_spheres, _two_size_classes, _with_repeats  # noqa: E402
from _adversarial_rays import adversarial_rays as _adversarial_rays  # noqa: E402

pytestmark = pytest.mark.gpu


def _render(sph, cam, w, h, spp, bvh_min=1, form=1, mode=api.RT_MODE_PARITY, passes=None, by_area=1, estimate=1, inst=None):
    if inst:
        mode = api.instance_mode(inst)           # a kernel instance of the diagnostics library by its symbol
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_choice_estimate(ctx._h, estimate))
        ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, by_area))
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, bvh_min, 152 * 1024))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, form))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.set_mode(mode)
        px = None
        for n in (passes or [spp]):
            px = ctx.render_pass(n)
        return {"pixels": px, "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats(),
                "pick": ctx._lib.rt_debug_bvh_pick(ctx._h)}


# (rt_set_mode of the _gq / _gt arms builds the pair table they read; _g and _gp walk the product's layout)
L2_WALKS = ["rt_trace_parity_pairs_g", "rt_trace_parity_pairs_gq", "rt_trace_parity_pairs_gt", "rt_trace_parity_pairs_gp"]


def _same(got, want):
    assert np.array_equal(got["pixels"], want["pixels"])
    assert np.array_equal(got["colors"].view(np.uint32), want["colors"].view(np.uint32))
    assert np.array_equal(got["seeds"], want["seeds"])
    g, o = got["stats"], want["stats"]
    assert (g["samples"], g["closest_rays"], g["shadow_rays"], g["sphere_tests"], g["rng_draws"]) == \
           (o["samples"], o["closest_calls"], o["shadow_calls"], o["sphere_tests"], o["rng_draws"])


_BUILD_SCENES = [lambda: scenes.random_spheres(1024), lambda: scenes.random_spheres(97), lambda: scenes.mirror_box(64), lambda: scenes.demo_plus(16),
                 lambda: (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET)]


def _every_build(sph, layout=None):
    """All three builds: the device's fixed shape (leaf ranges halved), the host's of a full scene upload (the shape chosen by surface
    area, leaves of up to 8; the default below 1500 tree spheres) and the device's by surface area (cuts between whole leaves; what
    updates and large uploads get) -- every leaf reached once from the root pair the header names, every sphere in one leaf, inside
    every box above it, lowest scene indices right, the stack deep enough.  layout: rt_debug_set_bvh_layout's arguments, None = the library's
    default.  Returns {by_area: (tables, packed table)}."""
    out, leaves, area = {}, {}, {}
    for by_area in (0, 1, 2):
        with api.RtContext(64, 64, diag=True) as ctx:
            ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, by_area))
            if layout is not None:
                ctx._check(ctx._lib.rt_debug_set_bvh_layout(ctx._h, *layout))
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
            ctx.set_scene(sph)
            b = bvh_check.read_bvh(ctx)
            pk = bvh_check.read_packed(ctx)
        assert b is not None
        assert bvh_check.check_structure(sph, b) == []
        assert b["n_always"] + sum(1 for i in b["index"][b["n_always"]:] if i != 0xffffffff) == len(bvh_check.first_of_equals(sph))
        leaves[by_area] = b["n_leaves"]
        area[by_area] = bvh_check.sum_of_box_areas(b)
        out[by_area] = (b, pk)
    assert leaves[0] <= leaves[1] <= 2 * leaves[0]              # partial leaves only where they pay (below 128 tree spheres both are the device's)
    assert leaves[2] == leaves[0]                               # the device cuts between whole leaves
    n_tree = len(sph) - b["n_always"]
    if n_tree >= 128:                                           # (below that every build is the halved shape)
        assert area[2] < area[0] and area[2] < 1.1 * area[1]    # what the walk pays for: the boxes a ray can meet
    return out


@pytest.mark.parametrize("maker", _BUILD_SCENES)
def test_device_built_tables_are_a_valid_hierarchy_in_the_product_layout(maker):
    """The diagnostics library's trees by default are the product's: the builders' numbering -- the halved shape's root is the pair
    before its middle leaf, a surface-area build's wherever the build put it --, no promoted top, no packed pair table."""
    sph = api.as_spheres(maker()[0])
    for by_area, (b, pk) in _every_build(sph).items():
        assert pk is None
        if b["n_leaves"] > 1:
            if by_area == 0 or len(sph) - b["n_always"] < 128:
                assert b["root"] == b["n_leaves"] // 2 - 1, (by_area, b["root"], b["n_leaves"])
            else:
                assert b["root"] < b["n_leaves"] - 1, (by_area, b["root"], b["n_leaves"])


_TABLES_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh_tables.json")


@pytest.mark.parametrize("case", list(bvh_check.DIGEST_CASES))
def test_every_builder_writes_the_recorded_bits(case):
    """tests/golden/bvh_tables.json (tools/bvh_check.py digests): the tables of the four builders -- device and host, halved and by surface
    area -- on the smallest scenes at which each of their paths can go wrong, recorded before the builders were made of one set of steps.
    Counts, every section of the blob and the surface-area estimate of an upload are still those bits; a failure names what moved."""
    with open(_TABLES_RECORD) as f:
        want = json.load(f)["cases"][case]
    got = bvh_check.digest_case(case)
    assert got["builder"] == got["meant"] == want["meant"], (got["n_tree"], got["builder"])
    assert bvh_check.digest_differences(got, want) == []


def _breadth_first(b):
    """Pair numbers in breadth-first order from the header's root, side 0 before side 1 (rt_bvh.hip rt_bvh_promote_kernel's order)."""
    order, queue = [], [b["root"]]
    while queue:
        p = queue.pop(0)
        if p & 0x8000:
            continue
        order.append(p)
        for side in (0, 1):
            queue.append(int(b["pairs"][4 * p + 2 * side][3:4].view(np.uint32)[0]) & 0xffff)
    return order


@pytest.mark.parametrize("maker", _BUILD_SCENES + [lambda: _many_spheres(5000)])
def test_the_layout_knob_promotes_the_top_and_packs_the_pairs(maker):
    """rt_debug_set_bvh_layout(ctx, 255, 1): the A/B arms' tables after every builder -- the top 255 pairs renumbered breadth-first with the
    root's pair first (a tree of 625 leaves cut off there), the packed pair table behind the blob.  rt_set_mode of an arm that reads one asks
    for it by itself and renders the oracle's frame; with the layout set back to the product's the arm is refused."""
    sph, orig, target = maker()
    sph = api.as_spheres(sph)
    for by_area, (b, pk) in _every_build(sph, (255, 1)).items():
        if b["n_leaves"] > 1:
            assert b["root"] == 0
            top = min(255, b["n_leaves"] - 1)
            assert _breadth_first(b)[:top] == list(range(top))
            assert pk is not None and bvh_check.check_packed(b, pk) == []
    if len(sph) < 1000:
        return
    w, h, spp = 32, 24, 2
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp, threads=16)
    for inst in ("rt_trace_parity_pairs_gt", "rt_trace_parity_pairs_gtp", "rt_trace_parity_pairs_gq"):
        with api.RtContext(w, h, diag=True) as ctx:
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
            ctx.set_scene(sph)
            ctx.set_camera(cam)
            assert bvh_check.read_packed(ctx) is None and bvh_check.read_bvh(ctx)["root"] != 0
            ctx.set_mode(api.instance_mode(inst))               # the arm's table, built at once
            assert (bvh_check.read_bvh(ctx)["root"] == 0) == inst.startswith("rt_trace_parity_pairs_gt")
            assert (bvh_check.read_packed(ctx) is not None) == inst.endswith("_gq")
            got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            assert ctx.last_kernel == inst
            _same(got, want)
            ctx._check(ctx._lib.rt_debug_set_bvh_layout(ctx._h, 0, 0))     # a mis-set arm: the tables rebuilt in the product's layout
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
            ctx.reset()
            with pytest.raises(api.RtError, match="has none"):
                ctx.render_pass(1)


@pytest.mark.parametrize("maker,w,h,spp", [
    (lambda: scenes.random_spheres(1024), 96, 64, 3),
    (lambda: scenes.random_spheres(300), 80, 60, 4),
    (lambda: scenes.mirror_box(64), 64, 64, 4),
    (lambda: scenes.mirror_box(200), 48, 48, 3),
    (lambda: scenes.demo_plus(16), 96, 64, 4),
])
def test_the_walk_equals_the_oracle(maker, w, h, spp):
    """the hierarchy forced on scenes of every kind (open, boxed, too small to get one by default): frames, colour plane,
    seeds and counters are the oracle's"""
    sph, orig, target = maker()
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp)
    got = _render(sph, cam, w, h, spp)
    _same(got, want)
    _same(_render(sph, cam, w, h, spp, by_area=0), want)        # the device build's fixed shape


def test_walk_and_plain_sweep_agree_ray_by_ray():
    """Rays of the scene itself (camera rays, bounce rays off the spheres, rays towards the lights) through the walk and
    through the plain sweep, one lane per ray: closest hit -- distance bits and sphere index; shadow rays -- first
    blocking index."""
    for maker, (w, h) in ((lambda: scenes.random_spheres(1024), (128, 72)), (lambda: scenes.mirror_box(96), (96, 64))):
        sph, orig, target = maker()
        r = bvh_check.agreement(sph, host.compute_camera(orig, target, w, h), w, h)
        assert r is not None and r["closest_hits"] > 10000 and r["shadow_blocked"] > 1000, r
        assert r["closest_differ"] == 0 and r["shadow_differ"] == 0, r


@pytest.mark.parametrize("seed", range(6))
def test_adversarial_scenes_equal_the_oracle_with_the_hierarchy_forced(seed):
    sph, orig, target = _adversarial(seed)
    w, h, spp = 72, 48, 3
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp)
    _same(_render(sph, cam, w, h, spp), want)
    _same(_render(sph, cam, w, h, spp, by_area=0), want)
    for inst in L2_WALKS:                                                           # the walks that read their tables from HBM / L2, every form of them
        _same(_render(sph, cam, w, h, spp, inst=inst), want)
    r = bvh_check.agreement(sph, cam, w, h, 60000)
    assert r["closest_differ"] == 0 and r["shadow_differ"] == 0, r


@pytest.mark.parametrize("seed", range(3))
def test_repeated_records_stay_out_of_the_hierarchy_and_change_no_bit(seed):
    """rt_bvh.hip mark_duplicates: a record that repeats an earlier one in centre and radius^2 is never a ray's answer (the reference keeps the
    first of equals), so the hierarchy leaves it out -- whatever its material says.  Frames, colour plane, seeds and counters are the oracle's
    through every builder; the tables hold exactly the first of each set of equals; and a device-resident update that ends a repeat (the record
    moves away) or creates one brings the record back / takes it out."""
    sph, orig, target = _with_repeats(seed)
    w, h, spp = 80, 56, 4
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp)
    for by_area in (1, 0, 2):
        _same(_render(sph, cam, w, h, spp, by_area=by_area), want)
    keep = bvh_check.first_of_equals(sph)
    assert len(keep) == len(sph) - 39 - 12 - 2                                     # 39 of the 40 phantoms, the 12 repeats, the repeated light and ground
    for by_area in (0, 1, 2):
        with api.RtContext(64, 64, diag=True) as ctx:
            ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, by_area))
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
            ctx.set_scene(sph)
            b = bvh_check.read_bvh(ctx)
        assert bvh_check.check_structure(sph, b) == []
        assert b["n_always"] == 1                                                    # ONE ground
    # updates: record 100 (a repeat) moves away -> it must be rendered; record 50 becomes a repeat of record 45 -> out again
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        assert np.array_equal(ctx.render_pass(spp), want["pixels"])
        moved = api.as_spheres(sph).copy()
        moved["p"][100] = (5.0, 12.0, 20.0)
        moved["rad"][100] = 6.0
        ctx.update_spheres(100, moved[100:101])
        ctx.reset()
        assert np.array_equal(ctx.render_pass(spp), O.render(moved, cam, w, h, spp)["pixels"])
        moved[50] = moved[45]
        moved["refl"][50] = 1
        ctx.update_spheres(50, moved[50:51])
        ctx.reset()
        got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        _same(got, O.render(moved, cam, w, h, spp))
        assert bvh_check.check_structure(moved, bvh_check.read_bvh(ctx)) == []


def test_measured_choice_changes_no_bit_and_probes_split_a_blocking_call():
    """form 0 = the library's behaviour.  Where the surface-area estimate of the uploaded tree is clear it decides and nothing
    is measured (one launch); inside its band -- or with the estimate switched off -- the first launches of a new scene time
    both forms (hierarchy warm, hierarchy timed, sweep warm, sweep timed) and the faster renders the rest.  Whatever is
    picked, and however the passes are split, the frame is the oracle's."""
    sph, orig, target = scenes.random_spheres(200)
    w, h, spp = 96, 64, 20
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp)
    clear = _render(sph, cam, w, h, spp, bvh_min=64, form=0)
    _same(clear, want)
    assert clear["pick"] == 1 and clear["stats"]["launches"] == 1       # 200 spheres scattered on a plane: predicted ratio 0.43
    one = _render(sph, cam, w, h, spp, bvh_min=64, form=0, estimate=0)
    _same(one, want)
    assert one["pick"] in (1, 2)                     # a blocking call of >= 16 passes waits for the verdict
    assert one["stats"]["launches"] == 5             # each form warm and timed, then the rest
    many = _render(sph, cam, w, h, spp, bvh_min=64, form=0, passes=[1, 1, 2, 3, 13], estimate=0)
    _same(many, want)
    box, borig, btarget = scenes.mirror_box(200)     # a packed box of 200: predicted 0.97, inside the band -> measured
    bcam = host.compute_camera(borig, btarget, w, h)
    banded = _render(box, bcam, w, h, spp, bvh_min=64, form=0)
    _same(banded, O.render(box, bcam, w, h, spp))
    assert banded["pick"] in (1, 2) and banded["stats"]["launches"] == 5
    c5, corig, ctarget = scenes.mirror_box(64)       # C5's box: predicted 1.65 -> the sweep, unmeasured
    ccam = host.compute_camera(corig, ctarget, w, h)
    swept = _render(c5, ccam, w, h, spp, bvh_min=56, form=0)
    _same(swept, O.render(c5, ccam, w, h, spp))
    assert swept["pick"] == 2 and swept["stats"]["launches"] == 1
    small = _render(*((lambda s: (s[0], host.compute_camera(s[1], s[2], w, h)))(scenes.demo_plus(16))), w, h, 4, bvh_min=64, form=0)
    assert small["pick"] == 0 and small["stats"]["launches"] == 1      # no hierarchy below bvh_min: nothing to measure
    big, orig, target = scenes.random_spheres(1700)                    # from 1500 spheres on the answer is known: no probe
    bcam = host.compute_camera(orig, target, 48, 32)
    with api.RtContext(48, 32, diag=True) as ctx:
        ctx.set_scene(big)
        ctx.set_camera(bcam)
        px = ctx.render_pass(20)
        assert ctx.stats()["launches"] == 1 and ctx.last_kernel.startswith("rt_trace_parity_pairs") and ctx.scene_choice()["picked"] is None
        assert np.array_equal(px, O.render(big, bcam, 48, 32, 20)["pixels"])


def test_moving_spheres_rebuild_the_hierarchy_on_the_stream():
    sph, orig, target = scenes.random_spheres(160)
    sph = api.as_spheres(sph).copy()
    w, h, spp = 80, 48, 3
    cam = host.compute_camera(orig, target, w, h)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        for step in range(3):
            sph["p"][10:40, 0] += np.float32(1.5)
            sph["p"][10:40, 1] += np.float32(0.25 * step)
            ctx.update_spheres(10, sph[10:40])
            ctx.reset()
            got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            _same(got, O.render(sph, cam, w, h, spp))
            b = bvh_check.read_bvh(ctx)
            assert bvh_check.check_structure(sph, b) == []


def test_an_update_of_the_whole_scene_stays_on_the_stream():
    """rt_update_spheres_async that rewrites EVERY record (the usual animated scene) is still an update: a device build on the
    stream -- full leaves, the shape chosen by surface area by the device's own kernel --, never the host build of rt_set_scene,
    which waits for the staging buffer's previous copy (the range must not decide)."""
    sph, orig, target = scenes.random_spheres(300)
    sph = api.as_spheres(sph).copy()
    w, h, spp = 64, 48, 2
    cam = host.compute_camera(orig, target, w, h)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 0))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        shaped = bvh_check.read_bvh(ctx)
        sph["p"][:, 0] += np.float32(0.5)
        ctx.update_spheres(0, sph)                      # first = 0, count = n: the whole scene
        b = bvh_check.read_bvh(ctx)
        n_tree = b["n_slots"] - b["n_always"]
        assert b["n_leaves"] == (int((np.abs(sph["rad"]) <= 16 * np.median(np.abs(sph["rad"]))).sum()) + 7) // 8
        assert n_tree == 8 * b["n_leaves"]              # (the host's build of the upload makes partial leaves, the device's never)
        assert bvh_check.check_structure(sph, b) == []
        got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        _same(got, O.render(sph, cam, w, h, spp))


def test_updates_get_the_shape_by_surface_area():
    """A moving scene's frames walk a tree shaped by surface area as an upload's do (the device's own build): fewer pair steps per
    ray than through the halved shape, the same bits."""
    sph, orig, target = scenes.random_spheres(1024)
    sph = api.as_spheres(sph).copy()
    w, h, spp = 160, 96, 2
    cam = host.compute_camera(orig, target, w, h)
    moved = sph.copy()
    moved["p"][2:, 0] += np.float32(0.75)
    want = O.render(moved, cam, w, h, spp)
    steps = {}
    for by_area in (0, 1):
        with api.RtContext(w, h, diag=True) as ctx:
            ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, by_area))
            ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
            ctx.set_scene(sph)
            ctx.set_camera(cam)
            ctx.update_spheres(0, moved)
            b = bvh_check.read_bvh(ctx)
            assert bvh_check.check_structure(moved, b) == []
            got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            _same(got, want)
            ctx.set_mode(api.instance_mode("rt_trace_parity_pairs_census"))
            ctx.reset()
            ctx.render_pass(spp, copy=False)
            steps[by_area] = bvh_check.counters_raw(ctx)[21]        # pair steps, summed over lanes
    assert steps[1] < 0.95 * steps[0]


def test_fast_mode_with_the_hierarchy_is_as_close_as_fast_mode_without():
    """Fused arithmetic changes single bounces, and on a scene with mirrors and glass a changed bounce changes a path:
    fast mode's distance from parity mode is a property of the scene (the 50 dB gate is quoted on the Demo scene).
    With the hierarchy it must be what it is with the plain sweep."""
    sph, orig, target = scenes.random_spheres(400)
    w, h, spp = 160, 96, 16
    cam = host.compute_camera(orig, target, w, h)
    par = _render(sph, cam, w, h, spp)
    plain = _render(sph, cam, w, h, spp, bvh_min=0, mode=api.RT_MODE_FAST)
    base = host.psnr(plain["pixels"], par["pixels"])
    assert base >= 30.0
    fast = _render(sph, cam, w, h, spp, mode=api.RT_MODE_FAST)
    assert fast["stats"]["samples"] == par["stats"]["samples"]
    assert host.psnr(fast["pixels"], par["pixels"]) >= min(50.0, base - 3.0)


def test_last_kernel_names_the_instance_the_scene_got():
    """rt_last_kernel: which instance the library picked (what a profiler will list)."""
    w, h = 64, 48
    with api.RtContext(w, h) as ctx:
        assert ctx.last_kernel == ""
        ctx.set_scene(host.demo_scene())
        ctx.set_camera(host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h))
        # six spheres: cooperative any-hit or not is MEASURED on the host's own launches -- coop warm (one launch), coop timed (16 passes), plain warm,
        # plain timed; then the faster one
        seen = []
        for _ in range(19):
            ctx.render_pass(2)
            seen.append(ctx.last_kernel)
        assert seen[:9] == ["rt_trace_parity_coop_w1"] * 9 and seen[9:18] == ["rt_trace_parity_w1"] * 9, seen
        assert seen[18] in ("rt_trace_parity_w1", "rt_trace_parity_coop_w1")
        ctx.set_mode(api.RT_MODE_FAST)
        ctx.render_pass(2)
        assert ctx.last_kernel == seen[18].replace("parity", "fast")            # (the verdict is the scene's, whatever the arithmetic mode)
        ctx.set_mode(api.RT_MODE_PARITY)
        sph, orig, target = scenes.demo_plus(16)
        ctx.set_scene(sph)
        ctx.render_pass(2)
        assert ctx.last_kernel == "rt_trace_parity_coop_w1"
        sph, orig, target = scenes.random_spheres(600)     # 600 spheres scattered on a plane: the estimate is clear, nothing is measured
        ctx.set_scene(sph)
        ctx.set_camera(host.compute_camera(orig, target, w, h))
        ctx.reset()
        for _ in range(3):
            ctx.render_pass(1)
            assert ctx.last_kernel == "rt_trace_parity_pairs"
        ch = ctx.scene_choice()
        assert ch["picked"] == "hierarchy" and ch["hierarchy_ms_per_pass"] == 0 and ch["sweep_ms_per_pass"] == 0
        sph, orig, target = scenes.mirror_box(200)         # a packed box of 200: inside the estimate's band, so it is measured
        ctx.set_scene(sph)
        ctx.set_camera(host.compute_camera(orig, target, w, h))
        ctx.reset()
        ctx.render_pass(1)                    # the first two launches of such a scene walk the hierarchy (warm, timed),
        assert ctx.last_kernel == "rt_trace_parity_pairs"
        ctx.render_pass(1)
        assert ctx.last_kernel == "rt_trace_parity_pairs"
        ctx.render_pass(1)                    # the next two sweep; the faster form renders the rest
        assert ctx.last_kernel == "rt_trace_parity_coop"
        ctx.render_pass(1)
        assert ctx.last_kernel == "rt_trace_parity_coop"
        assert ctx.scene_choice()["picked"] in (None, "hierarchy", "sweep")   # (asked without blocking: may still be open)
        ctx.render_pass(40)
        assert ctx.last_kernel in ("rt_trace_parity_pairs", "rt_trace_parity_coop")
        ch = ctx.scene_choice()                                    # both probes finished before that blocking call returned
        assert ch["picked"] == ("hierarchy" if ctx.last_kernel.endswith("pairs") else "sweep")
        assert ch["hierarchy_ms_per_pass"] > 0 and ch["sweep_ms_per_pass"] > 0


def test_multi_device_context_with_a_large_scene():
    """Every shard builds its own hierarchy; the FIRST shard measures hierarchy against sweep and the others follow its
    verdict, so one kernel instance renders the whole frame; the assembled frames are the oracle's."""
    sph, orig, target = scenes.random_spheres(300)
    w, h = 96, 72
    cam = host.compute_camera(orig, target, w, h)
    with api.RtContext(w, h, devices=[0, 0, 0]) as ctx:
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        done = 0
        for n in (1, 1, 2, 1, 20):               # the first four launches are the first shard's probes
            px = ctx.render_pass(n)
            done += n
            want = O.render(sph, cam, w, h, done)
            assert np.array_equal(px, want["pixels"])
        st = ctx.stats()
        assert (st["samples"], st["sphere_tests"]) == (want["stats"]["samples"], want["stats"]["sphere_tests"])
        assert np.array_equal(ctx.read_seeds(), want["seeds"])


def test_headline_call_on_a_large_scene():
    """rt_render(scene, cam, out, w, h, spp): a blocking call, so a new large scene is probed inside it; repeated
    calls with the same scene reuse the verdict.  Either way the frame is the oracle's."""
    sph, orig, target = scenes.random_spheres(220)
    w, h, spp = 88, 56, 18
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp)["pixels"]
    for _ in range(3):
        assert np.array_equal(api.render(sph, cam, w, h, spp), want)
    box, orig, target = scenes.mirror_box(100)
    cam = host.compute_camera(orig, target, w, h)
    assert np.array_equal(api.render(box, cam, w, h, spp), O.render(box, cam, w, h, spp)["pixels"])
    api.load_library().rt_release_cache()


@pytest.mark.parametrize("maker", [lambda: scenes.random_spheres(1024), lambda: scenes.mirror_box(120), lambda: _adversarial(3)])
def test_walk_equals_sweep_for_adversarial_rays(maker):
    sph = api.as_spheres(maker()[0])
    rng = np.random.default_rng(len(sph))
    rays = _adversarial_rays(sph, rng, 60000)
    with api.RtContext(32, 32, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
        ctx.set_scene(sph)
        out = np.zeros((len(rays), 4), np.uint32)
        with np.errstate(all="ignore"):
            ctx._check(ctx._lib.rt_debug_walk_rays(ctx._h, rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p)))
    differ = np.nonzero((out[:, 0] != out[:, 2]) | (out[:, 1] != out[:, 3]))[0]
    assert len(differ) == 0, (differ[:5], rays[differ[:5]], out[differ[:5]])
    closest = out[0::2]
    assert (closest[:, 0] != 0xffffffff).sum() > 1000          # the harness is not vacuous: thousands of hits
    assert (out[1::2, 0] < len(sph)).sum() > 1000               # ... and of blocked shadow rays


@pytest.mark.parametrize("n", [2000, 5000, 9500, 30000])
def test_scenes_beyond_lds(n):
    """More spheres than the LDS budget holds (the hierarchy's whole tables stop at ~1100 spheres, the sweep's at ~2500: four workgroups per CU): while the PAIRS
    still fit (to ~3200 spheres) they are staged and only the slots read from HBM / L2 (rt_trace_parity_pairs_m, round 5); beyond, the
    walk reads pairs and slots from HBM / L2 (rt_trace_parity_pairs_g); beyond 8192 spheres in the tree the tables are built on the
    host.  Frames, seeds and counters are still the oracle's."""
    sph, orig, target = _many_spheres(n)
    w, h, spp = 48, 32, 2
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp, threads=16)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == ("rt_trace_parity_pairs_m" if n <= 3000 else "rt_trace_parity_pairs_g")
        _same(got, want)
        if n <= 3000:                   # ... and the same scene with everything read from HBM / L2 (the budget set below the pairs)
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 56, 1024))
            ctx.reset()
            got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            assert ctx.last_kernel == "rt_trace_parity_pairs_g"
            _same(got, want)
        b = bvh_check.read_bvh(ctx)
        assert bvh_check.check_structure(api.as_spheres(sph), b) == []
        # the plain sweep over the table in HBM / L2 (what a scene without a hierarchy gets)
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 0, 0))
        ctx.reset()
        got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == ("rt_trace_parity_coop" if 16 * n + 128 <= 40 * 1024 else "rt_trace_parity_g")      # (staged while 4 workgroups fit a CU)
        _same(got, want)


@pytest.mark.parametrize("n", [9729, 9730, 9731, 9732, 12001])
def test_plain_sweep_through_the_scalar_cache(n):
    """rt_trace_parity_g (round 6): the plain sweep over a table beyond LDS reads it four records per scalar load, the next four in flight
    while these are tested, then two and one for what is left -- every residue of the table size modulo 4, records that are not numbers or
    infinite among the spheres (they are tested like the others and never hit), three lights (shadow sweeps that leave early, at every
    position of a group), a pass continued by a second launch."""
    sph, orig, target = _many_spheres(n, seed=n)
    rng = np.random.default_rng(n)
    odd = rng.choice(np.arange(2, n), 600, replace=False)
    sph["p"][odd[:200], 0] = np.float32("nan")
    sph["rad"][odd[200:400]] = np.float32("inf")
    sph["p"][odd[400:], 1] = np.float32("-inf")
    for k, at in enumerate(((-30, 40, 20), (45, 25, -30))):        # two more lights, one of them late in the table
        i = (5, n - 2)[k]
        sph["rad"][i], sph["p"][i], sph["e"][i], sph["refl"][i] = 4.0, at, (9, 8, 7), api.DIFF
    w, h = 40, 24
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, 3, threads=16)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 0, 0))           # no hierarchy: the fallback form
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.render_pass(1)
        got = {"pixels": ctx.render_pass(2), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert ctx.last_kernel == "rt_trace_parity_g"
        _same(got, want)


def test_many_scattered_updates_then_one_launch():
    """Round 6: rt_update_spheres_async sends its records at once and leaves the tables and the hierarchy to the next reader, which builds them
    ONCE (rt_scene.hip refresh_tables) -- 120 scattered spheres moved by 120 calls on two streams, a light switched off and another on; the
    hierarchy read back BEFORE any launch (the diagnostics' reader refreshes too) is a valid tree of the moved scene, the frame the oracle's;
    then more updates and a launch with no reader in between."""
    sph, orig, target = scenes.random_spheres(1024)
    sph = sph.copy()
    w, h, spp = 64, 40, 2
    cam = host.compute_camera(orig, target, w, h)
    rng = np.random.default_rng(8)
    with api.RtContext(w, h, diag=True) as ctx, api.RtContext(8, 8, diag=True) as other:      # (the second context lends its stream)
        side = other.stream
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.render_pass(spp)
        for rnd in range(2):
            who = rng.choice(np.arange(2, len(sph)), 120, replace=False)
            sph["p"][who] += rng.uniform(-3, 3, (120, 3)).astype(np.float32)
            sph["rad"][who[:10]] *= np.float32(1.7)
            sph["e"][who[10]] = (5.0, 4.0, 3.0)                                # a second light appears ...
            sph["e"][who[11]] = (0.0, 0.0, 0.0)
            for k, i in enumerate(who):
                ctx.update_spheres(int(i), sph[int(i):int(i) + 1], side if k % 2 else ctx.stream)
            if rnd == 0:
                assert bvh_check.check_structure(api.as_spheres(sph), bvh_check.read_bvh(ctx)) == []
            ctx.reset_async(ctx.stream)
            ctx.render_async(spp, ctx.stream)
            got = {"pixels": ctx.read_pixels(), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            _same(got, O.render(sph, cam, w, h, spp, threads=16))
        assert bvh_check.check_structure(api.as_spheres(sph), bvh_check.read_bvh(ctx)) == []


def test_staging_is_reused_behind_pending_copies_and_regrown():
    """The three page-locked stagings of a scene (rt_internal.h Staged: the sphere ring of four slots, the host-built tree's buffer, the duplicate
    flags') written again while the copies out of them are pending, given back and regrown -- one context, the hierarchy forced, every frame the
    oracle's bit for bit: the ring wraps behind a long launch (six one-record updates: the fifth and sixth reuse slots 0 and 1); then 200 records with
    a repeat (tree and flags staged, the ring grows to 256), at once 300 others (capacity 256 -> 512: the flags' staging given back and acquired
    again, the tree's grows) with no read in between, and the 200 again (nothing grows: both stagings reused behind their pending copies)."""
    w, h, spp = 48, 32, 2

    def frame(ctx):
        return {"pixels": ctx.read_pixels(), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}

    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        demo = api.as_spheres(host.demo_scene()).copy()                     # (ring capacity 64)
        cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
        ctx.set_scene(demo)
        ctx.set_camera(cam)
        ctx.render_async(spp, ctx.stream)
        _same(frame(ctx), O.render(demo, cam, w, h, spp))
        # the ring wraps: the copies wait behind 64 passes, the host does not
        ctx.render_async(64, ctx.stream)
        for i in range(6):
            demo["p"][i] += np.float32(0.5 + 0.25 * i)
            demo["c"][i] = (0.1 * (i + 1), 0.9 - 0.1 * i, 0.5)
            ctx.update_spheres(i, demo[i:i + 1], ctx.stream)
        ctx.reset_async(ctx.stream)
        ctx.render_async(spp, ctx.stream)
        _same(frame(ctx), O.render(demo, cam, w, h, spp))
        # filled, given back, regrown
        a, orig, target = scenes.random_spheres(200)
        a = api.as_spheres(a).copy()
        a[199] = a[198]
        b = api.as_spheres(scenes.random_spheres(300)[0]).copy()
        b["p"][2:, 0] += np.float32(2.0)
        b[150] = b[17]
        cam = host.compute_camera(orig, target, w, h)
        ctx.set_camera(cam)
        ctx.set_scene(a)
        ctx.set_scene(b)                                                    # (no read in between)
        ctx.reset_async(ctx.stream)
        ctx.render_async(spp, ctx.stream)
        _same(frame(ctx), O.render(b, cam, w, h, spp))
        ctx.set_scene(a)
        ctx.reset_async(ctx.stream)
        ctx.render_async(spp, ctx.stream)
        _same(frame(ctx), O.render(a, cam, w, h, spp))
        assert "_pairs" in ctx.last_kernel, ctx.last_kernel


@pytest.mark.parametrize("n_small,n_large,by_area", [(700, 300, 1), (3000, 600, 1), (3000, 600, 2), (9000, 1500, 1), (300, 700, 1)])
def test_two_size_classes_both_hang_in_the_tree(n_small, n_large, by_area):
    """Round 6: the cut between the tree and the always-list is never below an eighth of the scene's extent, so the larger class of a scene of
    two size classes -- more than 16 x the median radius, yet nowhere near the scene's size -- hangs in the tree instead of being swept by every
    ray (only the ground sphere stays outside).  Host-shaped and device-shaped trees, LDS and L2 walks; frames, seeds and counters are the
    oracle's, the tables a valid hierarchy."""
    sph, orig, target = _two_size_classes(n_small, n_large)
    w, h, spp = 48, 32, 2
    cam = host.compute_camera(orig, target, w, h)
    want = O.render(sph, cam, w, h, spp, threads=16)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, by_area))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        got = {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        assert "_pairs" in ctx.last_kernel
        _same(got, want)
        b = bvh_check.read_bvh(ctx)
        assert b["n_always"] == 1, b["n_always"]                 # the ground; the light (9) and the larger class are in the tree
        assert bvh_check.check_structure(api.as_spheres(sph), b) == []
        # ... and after a device-resident update of some of the larger spheres (the cut is formed again from the mirror)
        sph["p"][-5:] += np.float32([1.0, 0.0, -1.0])
        ctx.update_spheres(len(sph) - 5, sph[-5:], ctx.stream)
        ctx.reset_async(ctx.stream)
        ctx.render_async(spp, ctx.stream)
        got = {"pixels": ctx.read_pixels(), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
        _same(got, O.render(sph, cam, w, h, spp, threads=16))
        assert bvh_check.check_structure(api.as_spheres(sph), bvh_check.read_bvh(ctx)) == []


def test_plain_sweep_through_the_scalar_cache_sees_device_resident_updates():
    """The table rt_trace_parity_g reads through the scalar cache is rewritten on the stream between launches (rt_update_spheres_async ->
    rt_build_tables_kernel): every launch must see the records as they are then -- five frames of spheres moving and a light changing,
    queued without a host wait in between, each against the oracle."""
    n = 9740
    sph, orig, target = _many_spheres(n, seed=5)
    w, h, spp = 40, 24, 2
    cam = host.compute_camera(orig, target, w, h)
    rng = np.random.default_rng(5)
    with api.RtContext(w, h, diag=True) as ctx:
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 0, 0))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        for f in range(5):
            who = np.sort(rng.choice(np.arange(2, n), 40, replace=False))
            sph["p"][who] += rng.uniform(-2, 2, (40, 3)).astype(np.float32)
            sph["rad"][who] *= np.float32(1.5)
            sph["p"][1] += np.float32([3.0, -1.0, 2.0])                        # the light
            for i in who:
                ctx.update_spheres(int(i), sph[int(i):int(i) + 1], ctx.stream)
            ctx.update_spheres(1, sph[1:2], ctx.stream)
            ctx.reset_async(ctx.stream)
            ctx.render_async(spp, ctx.stream)
            got = {"pixels": ctx.read_pixels(), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}
            assert ctx.last_kernel == "rt_trace_parity_g"
            _same(got, O.render(sph, cam, w, h, spp, threads=16))


def test_the_scene_size_limit():
    too_many = np.zeros(262144 + 1, api.SPHERE_DT)
    with api.RtContext(32, 32) as ctx:
        with pytest.raises(api.RtError):
            ctx.set_scene(too_many)


# ---- the product library's own trees: the builders' numbering, no promoted top, no packed table (the suite's other hierarchy tests mostly
# ---- run the diagnostics library).  Every frame against the oracle, every test asserting the walk it meant to reach.
def _product(sph, cam, w, h, spp, mode=api.RT_MODE_PARITY):
    with api.RtContext(w, h) as ctx:
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.set_mode(mode)
        return {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats(),
                "kernel": ctx.last_kernel}


@pytest.mark.parametrize("maker,kernel", [
    (lambda: scenes.random_spheres(1024), "rt_trace_parity_pairs"),
    (lambda: _many_spheres(2000), "rt_trace_parity_pairs_m"),
    (lambda: _many_spheres(2500, seed=3), "rt_trace_parity_pairs_m"),
    (lambda: _many_spheres(5000), "rt_trace_parity_pairs_g"),
    (lambda: _many_spheres(9500), "rt_trace_parity_pairs_g"),
    (lambda: _many_spheres(30000), "rt_trace_parity_pairs_g"),
])
def test_product_library_walks_its_own_trees(maker, kernel):
    """librt_hip.so picks each walk by itself (tables in LDS, pairs in LDS, everything from HBM / L2) on a tree in its own layout:
    frames, colour plane, seeds and counters are the oracle's."""
    sph, orig, target = maker()
    w, h, spp = 48, 32, 2
    cam = host.compute_camera(orig, target, w, h)
    got = _product(sph, cam, w, h, spp)
    assert got["kernel"] == kernel
    _same(got, O.render(sph, cam, w, h, spp, threads=16))


def test_product_library_fast_mode_walk_is_as_close_as_the_fast_sweep():
    """Fast mode through the product's L2 walk (rt_trace_fast_pairs_g): as close to the parity frame as the fast plain sweep is
    (test_fast_mode_with_the_hierarchy_is_as_close_as_fast_mode_without's gate).  Among 5000 small spheres a differently rounded
    bounce or silhouette test changes a path: the fast plain sweep is 23-25 dB from parity here, so the floor is a scene's, not 30 dB."""
    sph, orig, target = _many_spheres(5000)
    w, h, spp = 96, 64, 8
    cam = host.compute_camera(orig, target, w, h)
    par = _product(sph, cam, w, h, spp)
    assert par["kernel"] == "rt_trace_parity_pairs_g"
    _same(par, O.render(sph, cam, w, h, spp, threads=16))
    plain = _render(sph, cam, w, h, spp, bvh_min=0, mode=api.RT_MODE_FAST)          # (the diagnostics library: no hierarchy at all)
    base = host.psnr(plain["pixels"], par["pixels"])
    assert base >= 20.0
    fast = _product(sph, cam, w, h, spp, mode=api.RT_MODE_FAST)
    assert fast["kernel"] == "rt_trace_fast_pairs_g"
    assert fast["stats"]["samples"] == par["stats"]["samples"]
    assert host.psnr(fast["pixels"], par["pixels"]) >= min(50.0, base - 3.0)


def _embedded(records, orig, target, n_fill, seed):
    """Adversarial records in front of a filler of _many_spheres (its ground and light dropped: the records bring their own), so that
    the scene is large enough for the product library to walk it from HBM / L2 without being told to."""
    fill = _many_spheres(n_fill, seed=seed)[0][2:]
    return np.concatenate([api.as_spheres(records), fill]), orig, target


@pytest.mark.parametrize("kind,seed", [("adversarial", 0), ("adversarial", 1), ("adversarial", 2), ("adversarial", 3),
                                       ("repeats", 0), ("repeats", 1)])
def test_adversarial_content_in_the_product_layout(kind, seed):
    """_adversarial / _with_repeats inside thousands of small spheres, through librt_hip.so's own choice: exact ties at higher indices,
    zero and negative radii, NaN / inf records, a far-away tree member, the camera inside glass (odd adversarial seeds), repeated
    records with other materials -- in a tree of the builders' numbering walked by _pairs_m (pairs in LDS) and by _pairs_g."""
    records, orig, target = (_adversarial if kind == "adversarial" else _with_repeats)(seed)
    w, h, spp = 48, 32, 2
    cam = host.compute_camera(orig, target, w, h)
    for n_fill, kernel in ((2200, "rt_trace_parity_pairs_m"), (6000, "rt_trace_parity_pairs_g")):
        sph, _, _ = _embedded(records, orig, target, n_fill, seed)
        got = _product(sph, cam, w, h, spp)
        assert got["kernel"] == kernel, (n_fill, got["kernel"])
        _same(got, O.render(sph, cam, w, h, spp, threads=16))
    if kind == "adversarial" and seed % 2:
        assert records["refl"][3] == api.REFR and np.linalg.norm(np.float32(orig) - records["p"][3]) < records["rad"][3]


def _product_frame(ctx, spp):
    ctx.reset()
    return {"pixels": ctx.render_pass(spp), "colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "stats": ctx.stats()}


def test_product_library_device_resident_updates():
    """rt_update_spheres_async through librt_hip.so on a scene it walks from HBM / L2: the tables and the tree are rebuilt by the next launch
    (the device's surface-area builder, rt_bvh.hip), and the records that repeat an earlier one are found again (mark_duplicates) --
    (a) 200 scattered records moved by 200 calls, then one launch; (b) a record made to repeat an earlier one bit for bit in centre and
    radius^2 with another material; (c) a repeat of the upload broken by moving the EARLIER record; (d) a record set to NaN, then back.
    Every frame is the oracle's for the scene as updated."""
    sph, orig, target = _many_spheres(5000, seed=11)
    sph = api.as_spheres(sph).copy()
    sph[4000] = sph[3000]                                   # a repeat in the upload, with another material
    sph["refl"][4000], sph["c"][4000] = (int(sph["refl"][3000]) + 1) % 3, (0.9, 0.1, 0.1)
    w, h, spp = 48, 32, 2
    cam = host.compute_camera(orig, target, w, h)
    rng = np.random.default_rng(11)
    with api.RtContext(w, h) as ctx:
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        got = _product_frame(ctx, spp)
        assert ctx.last_kernel == "rt_trace_parity_pairs_g"
        _same(got, O.render(sph, cam, w, h, spp, threads=16))

        def step(first, count=1):
            ctx.update_spheres(first, sph[first:first + count])

        def check(what):
            got = _product_frame(ctx, spp)
            assert ctx.last_kernel == "rt_trace_parity_pairs_g", what
            _same(got, O.render(sph, cam, w, h, spp, threads=16))

        who = rng.choice(np.arange(2, len(sph)), 200, replace=False)                  # (a)
        sph["p"][who] += rng.uniform(-4, 4, (200, 3)).astype(np.float32)
        sph["rad"][who[:20]] *= np.float32(1.6)
        for i in who:
            step(int(i))
        check("scattered")
        j, i = 2500, 1200                                                              # (b)
        sph["p"][j], sph["rad"][j] = sph["p"][i], -sph["rad"][i]                       # (-r: the same radius^2)
        sph["refl"][j], sph["e"][j] = (int(sph["refl"][i]) + 1) % 3, (2.0, 2.0, 2.0)
        step(j)
        check("made a repeat")
        sph["p"][3000] += np.float32([0.0, 25.0, 0.0])                                 # (c) record 4000 is the first of its kind now
        step(3000)
        check("broke a repeat")
        keep = sph[1700].copy()                                                        # (d)
        sph["p"][1700, 1] = np.float32("nan")
        step(1700)
        check("NaN")
        sph[1700] = keep
        step(1700)
        check("NaN and back")


@pytest.mark.parametrize("n,leaves", [(262144, 32768), (262137, 32767)])
def test_the_largest_trees(n, leaves):
    """RT_MAX_SPHERES: 262 143 spheres in the tree, 32 768 leaves -- the last the 15-bit leaf reference numbers (kBvhLeafRef) -- and a tree of
    one leaf less, built on the host (beyond the device builders) and walked from HBM / L2 by the product library.  One small frame each."""
    sph, orig, target = _many_spheres(n, seed=n)
    w, h, spp = 32, 24, 1
    cam = host.compute_camera(orig, target, w, h)
    with api.RtContext(8, 8, diag=True) as ctx:
        ctx.set_scene(sph)
        counts = (C.c_uint32 * 4)()
        ctx._check(ctx._lib.rt_debug_read_bvh(ctx._h, None, 0, counts))
        assert (counts[0], counts[1]) == (1, leaves)                 # (the ground outside; every other sphere in the tree, the light too)
    got = _product(sph, cam, w, h, spp)
    assert got["kernel"] == "rt_trace_parity_pairs_g"
    _same(got, O.render(sph, cam, w, h, spp, threads=16))
