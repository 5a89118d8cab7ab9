"""Temporal reprojection on the device (include/rt_api.h "temporal reprojection", csrc/rt_reproject.hip).  Every comparison is of bits:
rt_read_temporal after rt_reproject_async against rt_reproject_planes on the read-back colour planes, rt_features_planes and the records of both
contexts (which tests/test_reproject_cpu.py holds to a numpy restatement of rules 15-19), the packed plane against the oracle's toInt of the host
plane; then a moved sphere, what the call leaves alone, the plane's currency and the contexts, states and parameters the calls refuse."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api, host
from test_gpu_feature_planes import context
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, pack, snapshot
from test_gpu_tiles import S1, select
from test_reproject_cpu import CASE_IDS, CASES, F, assert_same_temporal, geometry, history, sideways

pytestmark = pytest.mark.gpu


def side(ctx, sph, cam, temporal=False):
    """One side of api.reproject_planes from what the context holds: its colour plane (or temporal plane), pass number, and rt_features_planes."""
    plane = ctx.read_temporal(packed=False) if temporal else (ctx.read_colors() if ctx.current_sample else None)
    return {"plane": plane, "passes": ctx.current_sample, "feat": api.features_planes(sph, cam, ctx.w, ctx.h), "cam": cam, "spheres": sph}


def assert_device_is_host(dst, want):
    """dst's temporal plane is `want` bit for bit, and its packed plane the oracle's toInt of `want` (where `want` is a number)."""
    got, px = dst.read_temporal()
    assert_same_temporal(got, want)
    number = ~np.isnan(want[..., 0:3]).any(axis=-1)[::-1].reshape(-1)            # (the packed plane's rows: row 0 = bottom)
    assert np.array_equal(px[number], pack(np.nan_to_num(want[..., 0:3]).reshape(-1), dst.w, dst.h)[number])
    return got


def planted(ctx):
    """A NaN colour word written into one texel of a rendered context's colour plane (a ground pixel of the Demo frame), the seeds and the pass kept."""
    col = ctx.read_colors().reshape(ctx.h, ctx.w, 3).copy()
    if ctx.w > 8 and ctx.h > 8:
        col[ctx.h - 4, ctx.w // 2, 1] = np.nan
    ctx.write_state(col, ctx.read_seeds(), ctx.current_sample)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_device_equals_reproject_planes_bit_for_bit(case):
    """Every case of the CPU test.  A 3-channel source is S's colour plane at 3 passes with a NaN planted; a 4-channel source is S's temporal plane,
    formed from a third view -- with S at 2 passes and a NaN planted (dst at 2 passes), or with S at pass 0, whose pixels without history hold
    n == 0 (dst at pass 0)."""
    name, channels, nd = case
    sphD, sphS, camD, camS, w, h = geometry(name)
    with context(sphS, camS, w, h) as S, context(sphD, camD, w, h) as D, context(sphS, camD, w, h) as P:
        ns = 3 if channels == 3 else nd
        if ns:
            S.seed_stream(1)
            S.render_async(ns)
            planted(S)
        S.features_async()
        if channels == 4:
            P.render_async(2)
            P.features_async()
            S.reproject_async(P)
            assert_device_is_host(S, api.reproject_planes(side(S, sphS, camS), side(P, sphS, camD), w, h))
        if nd:
            D.seed_stream(2)
            D.render_async(nd)
        D.features_async()
        before = snapshot(D), snapshot(S)
        src = side(S, sphS, camS, temporal=channels == 4)
        assert np.asarray(src["plane"]).size == channels * w * h
        for params in (None, {"k_pos": 1.5, "max_history": 10.0}):
            want = api.reproject_planes(side(D, sphD, camD), src, w, h, params)
            D.reproject_async(S, params)                      # the default stream
            first = assert_device_is_host(D, want)
            D.reproject_async(S, params, D.stream)            # the context's stream: the same words
            assert np.array_equal(bits(assert_device_is_host(D, want)), bits(first))
        assert_unchanged(D, before[0])
        assert_unchanged(S, before[1])
        if channels == 4:
            S.read_temporal()                                 # still current: being a source ends nothing


def test_history_is_handed_on_through_three_frames():
    """A -> B -> A: the second and third calls read the source's TEMPORAL plane, the third into the context the first one read from."""
    w, h = 41, 23
    sph = host.demo_scene()
    o, t = host.DEMO_ORIG, host.DEMO_TARGET
    cams = [host.compute_camera(sideways(o, t, share), t, w, h) for share in (0.0, 0.02, 0.04)]
    with context(sph, cams[0], w, h) as A, context(sph, cams[1], w, h) as B:
        A.render_async(3)
        A.features_async()
        B.seed_stream(2)
        B.render_async(1)
        B.features_async()
        B.reproject_async(A, None, B.stream)
        TB = assert_device_is_host(B, api.reproject_planes(side(B, sph, cams[1]), side(A, sph, cams[0]), w, h))
        _refused(A, RT_ERR_STATE, A.read_temporal)            # A has none yet
        A.set_camera(cams[2])                                 # frame 3 on the older context
        A.seed_stream(3)
        A.features_async()
        A.render_async(1)
        A.reproject_async(B, None, A.stream)
        src = side(B, sph, cams[1], temporal=True)
        assert np.array_equal(bits(src["plane"]), bits(TB))
        TA = assert_device_is_host(A, api.reproject_planes(side(A, sph, cams[2]), src, w, h))
        took = history(TA, 1)
        assert took.mean() > 0.5 and (TA[..., 3][took] > F(1.0) + F(3.0)).any()      # more than B's own pass and A's three: the chain
        B.read_temporal()                                     # B's plane is still current
        B.set_camera(cams[0])
        _refused(B, RT_ERR_STATE, B.read_temporal)
        B.seed_stream(4)
        B.features_async()
        B.reproject_async(A)                                  # a pure warp of A's temporal plane: B holds no pass
        assert_device_is_host(B, api.reproject_planes(side(B, sph, cams[0]), side(A, sph, cams[2], temporal=True), w, h))


def test_a_moved_sphere_on_the_device():
    sphD, sphS, camD, camS, w, h = geometry("demo_41x23_sphere")
    with context(sphS, camS, w, h) as S, context(sphS, camD, w, h) as D:
        S.render_async(3)
        S.features_async()
        D.features_async()
        D.update_spheres(3, sphD[3:4])                        # (the table rebuild is left pending)
        assert "feature plane" in _refused(D, RT_ERR_STATE, D.reproject_async, S)
        D.features_async()
        D.reproject_async(S)
        T = assert_device_is_host(D, api.reproject_planes(side(D, sphD, camD), side(S, sphS, camS), w, h))
        ids = api.features_planes(sphD, camD, w, h)[..., 7].view(np.uint32)
        assert (history(T, 0) & (ids == 3)).any()             # the moved sphere carries its own history
        still = api.reproject_planes(side(D, sphS, camD), side(S, sphS, camS), w, h)
        assert not np.array_equal(bits(T), bits(still))


def whole(ctx):
    return snapshot(ctx), ctx.read_pixels().copy(), ctx.stats(), ctx.last_kernel, bits(ctx.read_features()).copy()


def test_nothing_else_of_either_context_changes():
    sphD, sphS, camD, camS, w, h = geometry("demo_41x23_translated")
    with context(sphS, camS, w, h) as S, context(sphD, camD, w, h, api.RT_MODE_FAST) as D:
        S.render_pass(3)
        D.render_pass(2)
        for x in (S, D):
            x.features_async()
        was = whole(D), whole(S)
        D.reproject_async(S)
        D.read_temporal()
        for x, (snap, px, stats, kernel, feat) in zip((D, S), was):
            assert_unchanged(x, snap)
            now = whole(x)
            assert np.array_equal(now[1], px) and now[2] == stats and now[3] == kernel and np.array_equal(now[4], feat)
        _refused(S, RT_ERR_STATE, S.read_temporal)            # nothing was formed on the source
        # a fast destination packs with fast mode's toInt: the float plane is the host's all the same
        assert_same_temporal(D.read_temporal(packed=False), api.reproject_planes(side(D, sphD, camD), side(S, sphS, camS), w, h))
        # the render goes on from the colour plane, not from T
        D.render_pass(1)
        assert D.current_sample == 3


def test_what_ends_the_temporal_plane_and_what_keeps_it(tmp_path):
    sphD, sphS, camD, camS, w, h = geometry("demo_41x23_translated")
    with context(sphS, camS, w, h) as S, context(sphD, camD, w, h) as D, context(sphD, camD, w, h) as a, context(sphD, camD, w, h) as b:
        S.render_async(3)
        S.features_async()
        a.seed_stream(5)
        a.render_async(1)
        b.seed_stream(6)
        b.render_async(1)
        _refused(D, RT_ERR_STATE, D.read_temporal)            # never formed
        path = tmp_path / "state.bin"

        def form():
            D.reset()
            D.render_async(2)
            D.features_async()
            D.reproject_async(S)
            D.read_temporal()

        form()
        D.save_state(path)
        col, seeds = D.read_colors(), D.read_seeds()

        def subset():
            D.select_tiles(None, 0, D.stream)
            D.render_tiles_async(1, D.stream)

        moves_the_colour_plane = {
            "rt_render_async": lambda: D.render_async(1, D.stream),
            "rt_render_pass": lambda: D.render_pass(1),
            "rt_render_tiles_async": subset,
            "rt_reset": lambda: D.reset(),
            "rt_reset_async": lambda: D.reset_async(D.stream),
            "rt_seed_stream_async": lambda: D.seed_stream(3, D.stream),
            "rt_write_state": lambda: D.write_state(col, seeds, 2),
            "rt_load_state": lambda: D.load_state(path),
            "rt_merge_async": lambda: D.merge([a], D.stream),
            "rt_denoise_async": lambda: D.denoise(a, b),      # (D holds two passes, the halves one each)
        }
        for name, end in moves_the_colour_plane.items():
            form()
            end()
            assert "rt_reproject_async" in _refused(D, RT_ERR_STATE, D.read_temporal), name
        ends_the_feature_plane = {
            "rt_set_camera": lambda: D.set_camera(camD),
            "rt_set_scene": lambda: D.set_scene(sphD),
            "rt_update_spheres_async": lambda: D.update_spheres(1, sphD[1:2]),
        }
        for name, end in ends_the_feature_plane.items():
            form()
            end()
            _refused(D, RT_ERR_STATE, D.read_temporal)
            D.features_async()                                # a new feature plane does not bring the old temporal plane back
            _refused(D, RT_ERR_STATE, D.read_temporal)
        form()
        want = bits(D.read_temporal(packed=False)).copy()
        keepers = {
            "rt_set_mode": lambda: D.set_mode(api.RT_MODE_FAST),
            "rt_features_async": lambda: D.features_async(D.stream),
            "rt_compare": lambda: D.compare(S),
            "rt_read_colors": lambda: D.read_colors(),
            "rt_read_pixels": lambda: D.read_pixels(),
            "rt_read_seeds": lambda: D.read_seeds(),
            "rt_read_features": lambda: D.read_features(),
            "rt_read_temporal": lambda: D.read_temporal(),
            "a reprojection FROM it": lambda: a.features_async() or a.reproject_async(D),
        }
        for name, keep in keepers.items():
            keep()
            assert np.array_equal(bits(D.read_temporal(packed=False)), want), name


def test_the_contexts_states_and_parameters_the_calls_refuse():
    w, h = 41, 23
    sph = host.demo_scene()
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    lib = api.load_library()
    with context(sph, cam, w, h) as D, context(sph, cam, w, h) as S, context(sph, cam, w + 1, h) as wider, make("demo", w, h, rank=1, nranks=2) as shard, \
            make("demo", w, h, devices=[0, 0]) as multi, context(sph[:5], cam, w, h) as fewer:
        S.render_async(2)
        for x in (D, S, wider, fewer):
            x.features_async()
        snaps = snapshot(D), snapshot(S)

        def unchanged():
            assert_unchanged(D, snaps[0])
            assert_unchanged(S, snaps[1])
            _refused(D, RT_ERR_STATE, D.read_temporal)        # and nothing was formed

        # RT_ERR_ARG: the contexts
        assert lib.rt_reproject_async(None, S._h, None, None) == RT_ERR_ARG and lib.rt_reproject_async(D._h, None, None, None) == RT_ERR_ARG
        assert "itself" in _refused(D, RT_ERR_ARG, D.reproject_async, D)
        _refused(D, RT_ERR_ARG, D.reproject_async, wider)
        _refused(wider, RT_ERR_ARG, wider.reproject_async, S)
        for x in (shard, multi):
            _refused(D, RT_ERR_ARG, D.reproject_async, x)
            _refused(x, RT_ERR_ARG, x.reproject_async, S)
            _refused(x, RT_ERR_ARG, x.read_temporal)
        if torch.cuda.device_count() >= 2:                   # (a one-GPU machine cannot make this case)
            with api.RtContext(w, h, device=1) as elsewhere:
                elsewhere.set_scene(sph)
                elsewhere.set_camera(cam)
                elsewhere.features_async()
                assert "device" in _refused(D, RT_ERR_ARG, D.reproject_async, elsewhere)
        # RT_ERR_ARG: the parameters
        nan, inf = float("nan"), float("inf")
        for name in ("k_pos", "max_history"):
            for bad in (0.0, -2.0, nan, inf):
                assert name in _refused(D, RT_ERR_ARG, D.reproject_async, S, {name: bad})
        for word in (0, 1):
            p = api.reproject_defaults()
            p.reserved[word] = 7
            assert "reserved" in _refused(D, RT_ERR_ARG, D.reproject_async, S, p)
        assert lib.rt_read_temporal(D._h, None, None) == RT_ERR_ARG
        unchanged()
        # RT_ERR_STATE: a different record count
        assert "records" in _refused(D, RT_ERR_STATE, D.reproject_async, fewer)
        # ... a source at pass 0 without a temporal plane
        assert "neither" in _refused(S, RT_ERR_STATE, S.reproject_async, D)
        unchanged()
        # ... stale features on either side
        for x in (D, S):
            x.set_camera(cam)
            assert "feature plane" in _refused(D, RT_ERR_STATE, D.reproject_async, S)
            x.features_async()
        unchanged()
        # ... ragged contexts on either side
        with context(sph, cam, w, h) as R:
            R.features_async()
            R.render_async(2, R.stream)
            assert select(R, S1) == (4, 12)
            R.render_tiles_async(1, R.stream)
            assert "ragged" in _refused(D, RT_ERR_STATE, D.reproject_async, R)
            D.render_async(1)
            snap_r = snapshot(D)
            assert "ragged" in _refused(R, RT_ERR_STATE, R.reproject_async, D)
            assert_unchanged(D, snap_r)
        # what was refused left nothing half done
        D.reproject_async(S)
        assert_device_is_host(D, api.reproject_planes(side(D, sph, cam), side(S, sph, cam), w, h))
