"""Feature planes on the device (include/rt_api.h "feature planes", csrc/rt_features.hip).  Every comparison is of bits: rt_read_features after
rt_features_async against rt_features_planes on the same records and camera (which tests/test_features_cpu.py holds to a numpy restatement of
rules 10-12 and to the oracle's sphere test); then the plane's currency and the contexts the calls refuse."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api, host
from test_features_cpu import MISS, assert_same_plane, records, scene, sphere
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, make, snapshot

pytestmark = pytest.mark.gpu

CHUNK = 1024              # records the kernel stages at a time (csrc/rt_features.hip kFtChunk)


def context(sph, cam, w, h, mode=None):
    ctx = api.RtContext(w, h)
    ctx.set_scene(sph)
    ctx.set_camera(cam)
    if mode is not None:
        ctx.set_mode(mode)
    return ctx


@pytest.mark.parametrize("name", ["demo_1x1", "demo_41x23", "demo_70x19", "inside", "identical", "sky", "nonfinite"])
def test_the_device_equals_features_planes_bit_for_bit(name):
    sph, cam, w, h = scene(name)
    with context(sph, cam, w, h) as ctx:
        before = snapshot(ctx)
        ctx.features_async()
        got = ctx.read_features()
        assert_same_plane(got, api.features_planes(sph, cam, w, h))
        ctx.features_async(ctx.stream)                       # again, on the context's stream: the same words
        assert_same_plane(ctx.read_features(), got)
        assert_unchanged(ctx, before)                        # colours, seeds and pass number stay


def test_a_fast_context_forms_the_same_plane():
    sph, cam, w, h = scene("demo_41x23")
    with context(sph, cam, w, h, api.RT_MODE_FAST) as ctx:
        ctx.render_pass(2)                                   # (fast mode's kernels have run on it)
        ctx.features_async()
        assert_same_plane(ctx.read_features(), api.features_planes(sph, cam, w, h))


def chunked_scene(n, tie=True):
    """n records at 40x24: small spheres on a far wall; the NEAREST sphere at index n - 1 (the last chunk), and two identical records either side of
    the chunk boundary (where n reaches past it: at n = CHUNK + 1 they ARE the last chunk's only record and its neighbour, so they are made the
    nearest sphere) or, in a single chunk, at its two ends.  tie False: no tied pair, the nearest sphere at n - 1 whatever n is."""
    rng = np.random.default_rng(n)
    rows = [sphere(1.5, (float(x), float(y), -60.0), c=tuple(rng.uniform(0.1, 0.9, 3))) for x, y in zip(rng.uniform(-70, 70, n), rng.uniform(-45, 45, n))]
    near = sphere(5.0, (9.0, 1.0, 25.0), c=(0.9, 0.2, 0.2))
    tied = lambda c: sphere(6.0, (-11.0, -2.0, 5.0), c=c)    # noqa: E731
    if not tie:
        rows[n - 1] = near
        return records(rows), None, None
    if n == CHUNK + 1:
        tied = lambda c: sphere(6.0, (-11.0, -2.0, 30.0), c=c)      # noqa: E731
        first, second = CHUNK - 1, CHUNK
    elif n > CHUNK:
        first, second = CHUNK - 1, CHUNK
        rows[n - 1] = near
    else:
        first, second = 0, n - 2
        rows[n - 1] = near
    rows[first], rows[second] = tied((0.1, 0.9, 0.1)), tied((0.1, 0.1, 0.9))
    return records(rows), first, second


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_scenes_either_side_of_a_chunk_of_records(n):
    w, h = 40, 24
    sph, first, second = chunked_scene(n)
    cam = host.compute_camera((0.0, 0.0, 50.0), (0.0, 0.0, 0.0), w, h)
    want = api.features_planes(sph, cam, w, h)
    ids = want[..., 7].view(np.uint32)
    assert (ids == first).any() and not (ids == second).any()            # the tie: the lower index, from the earlier chunk
    if n != CHUNK + 1:
        assert (ids == n - 1).any() and want[ids == n - 1][:, 6].max() < want[ids != MISS][:, 6].max()       # the last record is seen, in front
    assert (ids == MISS).any() and len(np.unique(ids)) > 20              # sky, and a good many of the wall's spheres
    with context(sph, cam, w, h) as ctx:
        ctx.features_async()
        assert_same_plane(ctx.read_features(), want)


def test_a_last_chunk_of_one_record_holds_the_nearest_sphere():
    """CHUNK + 1 records, the nearest sphere the last: the pixels that see it depend on a trailing chunk of ONE record being staged and swept."""
    w, h, n = 40, 24, CHUNK + 1
    sph, _, _ = chunked_scene(n, tie=False)
    cam = host.compute_camera((0.0, 0.0, 50.0), (0.0, 0.0, 0.0), w, h)
    want = api.features_planes(sph, cam, w, h)
    ids = want[..., 7].view(np.uint32)
    assert (ids == n - 1).sum() > 10 and want[ids == n - 1][:, 6].max() < want[(ids != MISS) & (ids != n - 1)][:, 6].min()
    with context(sph, cam, w, h) as ctx:
        ctx.features_async()
        assert_same_plane(ctx.read_features(), want)


def test_a_moved_sphere_is_seen_once_the_plane_is_formed_again():
    sph, cam, w, h = scene("demo_41x23")
    with context(sph, cam, w, h) as ctx:
        ctx.features_async()
        first = ctx.read_features().copy()
        moved = sph.copy()
        moved["p"][3] += np.float32([6.0, 4.0, 2.0])                      # the blue sphere, visible
        ctx.update_spheres(3, moved[3:4])
        _refused(ctx, RT_ERR_STATE, ctx.read_features)
        ctx.features_async()                                              # (the table rebuild the update left pending runs first)
        got = ctx.read_features()
        assert_same_plane(got, api.features_planes(moved, cam, w, h))
        assert not np.array_equal(got.view(np.uint32), first.view(np.uint32))


def test_scene_and_camera_end_the_plane_and_nothing_else_does():
    sph, cam, w, h = scene("demo_41x23")
    with context(sph, cam, w, h) as ctx, make("demo", w, h) as src:
        _refused(ctx, RT_ERR_STATE, ctx.read_features)                    # never formed
        enders = {
            "rt_set_camera": lambda: ctx.set_camera(cam),
            "rt_set_scene": lambda: ctx.set_scene(sph),
            "rt_update_spheres_async": lambda: ctx.update_spheres(1, sph[1:2]),
        }
        want = api.features_planes(sph, cam, w, h)
        for name, end in enders.items():
            ctx.features_async()
            assert_same_plane(ctx.read_features(), want)
            end()
            assert "rt_features_async" in _refused(ctx, RT_ERR_STATE, ctx.read_features), name
        ctx.features_async()
        src.render_async(2, src.stream)
        keepers = {
            "rt_render_async": lambda: ctx.render_async(2, ctx.stream),
            "rt_reset_async": lambda: ctx.reset_async(ctx.stream),
            "rt_reset": lambda: ctx.reset(),
            "rt_merge_async": lambda: ctx.merge([src], ctx.stream),
            "rt_set_mode": lambda: ctx.set_mode(api.RT_MODE_FAST),
            "rt_seed_stream_async": lambda: ctx.seed_stream(3, ctx.stream),
        }
        for name, keep in keepers.items():
            keep()
            assert_same_plane(ctx.read_features(), want)


def test_the_contexts_and_states_the_calls_refuse():
    w, h = 41, 23
    sph, cam, _, _ = scene("demo_41x23")
    lib = api.load_library()
    with api.RtContext(w, h) as bare, make("demo", w, h, rank=1, nranks=2) as shard, make("demo", w, h, devices=[0, 0]) as multi:
        _refused(bare, RT_ERR_STATE, bare.features_async)                 # no scene, no camera
        bare.set_scene(sph)
        _refused(bare, RT_ERR_STATE, bare.features_async)                 # no camera
        bare.set_camera(cam)
        bare.features_async()
        assert lib.rt_read_features(bare._h, None) == RT_ERR_ARG
        for x in (shard, multi):
            _refused(x, RT_ERR_ARG, x.features_async)
            _refused(x, RT_ERR_ARG, x.read_features)
            _refused(x, RT_ERR_ARG, x.set_denoise_guide, api.guide_defaults())
            _refused(x, RT_ERR_ARG, x.set_denoise_guide, None)
        for bad in ({"k_albedo": 0.0}, {"k_normal": -1.0}, {"k_depth": float("nan")}, {"k_albedo": float("inf")}, {"reserved": 2}):
            assert list(bad)[0] in _refused(bare, RT_ERR_ARG, bare.set_denoise_guide, bad)
        bare.set_denoise_guide({"k_depth": 0.1})
        bare.set_denoise_guide(None)
