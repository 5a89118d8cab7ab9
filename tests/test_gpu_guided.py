"""NL-means guided by feature planes on the device (include/rt_api.h "feature planes", rules 13-14; csrc/rt_denoise.hip).  Every comparison
is of bits: the three filter calls under a guide against rt_denoise_guided_planes / rt_denoise_pair_guided_planes on the same colour planes and the
feature plane the context itself formed (tests/test_guided_cpu.py holds the host functions to a numpy restatement; tests/test_gpu_feature_planes.py
holds the plane to rt_features_planes); then the guide's settings, the plane's currency as the filters see it, and the two adaptive loops."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

import test_tiles_cpu as T
from raytracing_simple_amd import api
from test_denoise_cpu import assert_same_bits, planes
from test_features_cpu import scene
from test_gpu_denoise_pair import N, Halves, metric_of, two_streams
from test_gpu_live_checks import pixels_of, rendered_pair, state_of, three_groups
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, snapshot
from test_gpu_tiles import select
from test_guided_cpu import GUIDE, PARAMS, WIDE

pytestmark = pytest.mark.gpu

SIZES = [(41, 23), (70, 19)]


def guide_on(*ctxs, guide=GUIDE):
    for c in ctxs:
        c.set_denoise_guide(guide)
        c.features_async()


# ---- 1. the three calls equal their host functions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_denoise_under_a_guide_equals_guided_planes_bit_for_bit(w, h):
    with Halves(w, h, extra=1) as t:
        dst = t.all[2]
        guide_on(t.a, t.b)
        Fp = t.a.read_features()
        for kind in ("noisy", "nonfinite"):
            D, A, B = planes(w, h, kind)
            t.write(A, B)
            for params in PARAMS:
                dst.write_state(D, None, 2 * N)
                dst.denoise(t.a, t.b, params)
                got = dst.read_colors()
                assert_same_bits(got, api.denoise_guided_planes(D, A, B, Fp, w, h, params, GUIDE))
                if params["search_radius"] > 1:
                    assert not np.array_equal(bits(got), bits(api.denoise_planes(D, A, B, w, h, params)))      # (the guide did something)


@pytest.mark.parametrize("w,h", SIZES)
def test_denoise_pair_under_a_guide_equals_pair_guided_planes_float_and_packed(w, h):
    with Halves(w, h) as t:
        guide_on(t.a, t.b)
        Fp = t.a.read_features()
        for kind in ("noisy", "nonfinite"):
            D, A, B = planes(w, h, kind)
            if kind == "nonfinite":
                A = D                                         # the half with a NaN, +inf and -inf planted
            t.write(A, B)
            before = snapshot(t.a), snapshot(t.b)
            for params in PARAMS + [{"search_radius": 0, "patch_radius": 1}]:
                t.a.denoise_pair(t.b, params)
                want = api.denoise_pair_guided_planes(A, B, Fp, w, h, params, GUIDE)
                for got, x in zip((t.a.read_filtered(), t.b.read_filtered()), want):
                    assert_same_bits(got, x)
                err, tiles = t.a.compare_filtered(t.b, tiles=True)          # the packed planes, through the exact integer metric and its tile map
                want_err, want_tiles = metric_of(want[0], want[1], w, h)
                assert err == want_err and np.array_equal(tiles, want_tiles), params
                # exchanging a and b exchanges FA and FB: each context's plane stays its own
                t.b.denoise_pair(t.a, params)
                for got, x in zip((t.a.read_filtered(), t.b.read_filtered()), want):
                    assert_same_bits(got, x)
            for c, s in zip((t.a, t.b), before):
                assert_unchanged(c, s)


def test_a_nan_normal_in_the_devices_own_plane_constrains_nothing():
    sph, cam, w, h = scene("nonfinite")
    _, A, B = planes(w, h)
    with api.RtContext(w, h) as a, api.RtContext(w, h) as b:
        for c, X in ((a, A), (b, B)):
            c.set_scene(sph)
            c.set_camera(cam)
            c.write_state(X, None, N)
        guide_on(a, b)
        Fp = a.read_features()
        assert np.isnan(Fp[..., 3:6]).any()
        a.denoise_pair(b)
        want = api.denoise_pair_guided_planes(A, B, Fp, w, h, None, GUIDE)
        assert np.isfinite(want[0]).all()
        assert_same_bits(a.read_filtered(), want[0])
        assert_same_bits(b.read_filtered(), want[1])


@pytest.mark.parametrize("w,h", SIZES)
def test_denoise_pair_tiles_under_a_guide_refreshes_the_selected_groups(w, h):
    mask = three_groups(w, h)                                 # includes the top, partial, group row
    m = pixels_of(mask, w, h)
    for params in PARAMS:
        a, b = rendered_pair(w, h, 3)
        with a, b:
            guide_on(a, b)
            Fp = a.read_features()
            a.denoise_pair(b, params)
            before = a.read_filtered().copy(), b.read_filtered().copy()
            for old, x in zip(before, api.denoise_pair_guided_planes(a.read_colors(), b.read_colors(), Fp, w, h, params, GUIDE)):
                assert_same_bits(old, x)
            assert select(a, mask) == select(b, mask) == (3, int(T.tiles_of(mask, w, h).sum()))
            a.render_tiles_async(2, a.stream)
            b.render_tiles_async(2, b.stream)
            a.denoise_pair_tiles(b, params)
            fresh = api.denoise_pair_guided_planes(a.read_colors(), b.read_colors(), Fp, w, h, params, GUIDE)
            want = []
            for got, new, old in zip((a.read_filtered(), b.read_filtered()), fresh, before):
                x = old.reshape(h, w, 3).copy()
                x[m] = new.reshape(h, w, 3)[m]
                assert_same_bits(got, x)
                assert np.array_equal(bits(got).reshape(h, w, 3)[~m], bits(old).reshape(h, w, 3)[~m])      # nothing else was touched
                want.append(x.reshape(-1))
            assert a.compare_filtered(b) == metric_of(want[0], want[1], w, h)[0]


# ---- 2. on, off, wide ----------------------------------------------------------------------------------------------------------------------
def test_switched_on_and_off_again_the_unguided_calls_return_the_bits_they_returned_before():
    w, h = 41, 23
    D, A, B = planes(w, h)
    with Halves(w, h, extra=1) as t:
        dst = t.all[2]
        t.write(A, B)

        def all_three():
            dst.write_state(D, None, 2 * N)
            dst.denoise(t.a, t.b)
            t.a.denoise_pair(t.b)
            return bits(dst.read_colors()).copy(), bits(t.a.read_filtered()).copy(), bits(t.b.read_filtered()).copy(), t.a.compare_filtered(t.b)

        first = all_three()
        for x, want in zip(first, (api.denoise_planes(D, A, B, w, h),) + api.denoise_pair_planes(A, B, w, h)):
            assert np.array_equal(x, bits(want))
        guide_on(t.a, t.b)
        guided = all_three()
        assert not np.array_equal(guided[0], first[0]) and not np.array_equal(guided[1], first[1])
        guide_on(t.a, t.b, guide=WIDE)                       # every k 1e18 over finite features: wf is exactly 1
        wide = all_three()
        for g, x in zip(wide, first):
            assert np.array_equal(g, x) if isinstance(x, np.ndarray) else g == x
        for c in (t.a, t.b):
            c.set_denoise_guide(None)
        again = all_three()
        for g, x in zip(again, first):
            assert np.array_equal(g, x) if isinstance(x, np.ndarray) else g == x


# ---- 3. settings and currency ------------------------------------------------------------------------------------------------------------------
def test_halves_that_differ_in_their_guide_or_hold_a_stale_plane_are_refused_and_unchanged():
    w, h = 41, 23
    D, A, B = planes(w, h)
    sph, cam, _, _ = scene("demo_41x23")
    with Halves(w, h, extra=1) as t:
        a, b, dst = t.all
        t.write(A, B)
        dst.write_state(D, None, 2 * N)
        a.denoise_pair(b)
        planes_before = bits(a.read_filtered()).copy(), bits(b.read_filtered()).copy()
        snaps = [snapshot(c) for c in (a, b, dst)]

        def every_call_refused(code):
            calls = ((dst.denoise, a, b), (a.denoise_pair, b), (b.denoise_pair, a), (a.denoise_pair_tiles, b), (a.render_converged_filtered, b, 30.0, 1, 8),
                     (a.render_adaptive_filtered, b, 30.0, 4, 1, 8), (a.render_adaptive_filtered_tiles, b, 30.0, 4, 1, 8))
            for call, *args in calls:
                _refused(a, code, call, *args)
            for c, s in zip((a, b, dst), snaps):
                assert_unchanged(c, s)
            assert np.array_equal(bits(a.read_filtered()), planes_before[0]) and np.array_equal(bits(b.read_filtered()), planes_before[1])

        a.set_denoise_guide(GUIDE)                           # on one half only
        a.features_async()
        every_call_refused(RT_ERR_STATE)
        b.set_denoise_guide({**GUIDE, "k_depth": 0.06})      # on both, other bytes
        b.features_async()
        every_call_refused(RT_ERR_STATE)
        b.set_denoise_guide(GUIDE)
        dst.set_denoise_guide({"k_albedo": 3.0})             # dst's setting is ignored
        a.denoise_pair(b)
        planes_before = bits(a.read_filtered()).copy(), bits(b.read_filtered()).copy()
        dst.denoise(a, b)
        dst.write_state(D, None, 2 * N)
        # the plane of either half not current: each of the three calls that end it, on each half
        for c in (a, b):
            for end in (lambda: c.set_camera(cam), lambda: c.set_scene(sph), lambda: c.update_spheres(2, sph[2:3])):
                end()
                _refused(c, RT_ERR_STATE, c.read_features)
                every_call_refused(RT_ERR_STATE)
                c.features_async()
                a.denoise_pair(b)
                assert np.array_equal(bits(a.read_filtered()), planes_before[0])
        # launches, resets and merges leave it current: the guided call still runs
        a.render_async(1, a.stream)
        b.render_async(1, b.stream)
        a.denoise_pair(b)
        a.reset()
        b.reset()
        t.write(A, B)
        dst.reset()
        dst.merge([a, b], dst.stream)
        a.denoise_pair(b)
        assert np.array_equal(bits(a.read_filtered()), planes_before[0])


def test_sharded_and_multi_device_halves_are_refused_under_a_guide():
    w, h = 41, 23
    _, A, B = planes(w, h)
    with Halves(w, h) as t, make("demo", w, h, rank=1, nranks=2) as shard, make("demo", w, h, devices=[0, 0]) as multi:
        t.write(A, B)
        guide_on(t.a, t.b)
        for x in (shard, multi):
            _refused(t.a, RT_ERR_ARG, t.a.denoise_pair, x)
            _refused(t.a, RT_ERR_ARG, x.denoise_pair, t.b)
            _refused(t.a, RT_ERR_ARG, t.a.render_adaptive_filtered_tiles, x, 30.0, 1, 1, 8)
            _refused(t.a, RT_ERR_ARG, x.set_denoise_guide, GUIDE)
            _refused(t.a, RT_ERR_ARG, x.features_async)
        t.a.denoise_pair(t.b)


# ---- 4. the two adaptive loops under a guide -----------------------------------------------------------------------------------------------
def test_the_loop_with_live_checks_equals_the_whole_frame_loop_under_a_guide():
    w, h, args = 96, 64, (28.0, 4, 4, 12)
    out = []
    for live in (False, True):
        a, b = two_streams(w, h)
        with a, b:
            guide_on(a, b)
            loop = a.render_adaptive_filtered_tiles if live else a.render_adaptive_filtered
            reached, last, checks = loop(b, *args)
            assert a.compare_filtered(b) == last              # the last check's planes are current
            assert checks >= 2 and a.current_sample <= 12     # (a second check: the live loop's is the tiles call)
            out.append(((reached, checks), state_of(a), state_of(b)))
    (ret, sa, sb), (ret_l, la, lb) = out
    assert ret_l == ret
    passes = sa[0]
    assert np.array_equal(passes, sb[0]) and (passes < passes.max()).any()      # some group retired before the last check
    for got, want in ((la, sa), (lb, sb)):
        for g, x in zip(got, want):
            assert np.array_equal(g, x) if isinstance(x, np.ndarray) else g == x
    # ... and the guide steered it: the unguided loop leaves another pass map or other checks
    a, b = two_streams(w, h)
    with a, b:
        a.render_adaptive_filtered(b, *args)
        Fa = a.read_filtered()
    a, b = two_streams(w, h)
    with a, b:
        guide_on(a, b)
        a.render_adaptive_filtered(b, *args)
        assert not np.array_equal(bits(a.read_filtered()), bits(Fa))
