"""Shadow-aware history on the device (include/rt_api.h "shadow-aware history", csrc/rt_reproject.hip).  Every comparison is of bits:
rt_read_temporal, rt_read_moments and rt_read_history_flags after rt_reproject_async against rt_reproject_shadow_planes on the read-back inputs
(tests/test_shadow_history_cpu.py holds that function to a numpy restatement of rules 29-32) -- every kernel instance, partial workgroups both ways, a
one-lane image, pair lists of no pair, one pair, exactly one LDS chunk and one pair more -- then the setting turned off again, the flag plane's
currency, and two contexts taking turns while a sphere moves."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api
from test_atrous_cpu import assert_same_plane
from test_gpu_feature_planes import context
from test_gpu_reproject import planted
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, pack, snapshot
from test_reproject_cpu import F
from test_shadow_history_cpu import dust, records

pytestmark = pytest.mark.gpu

ON = {}                                                       # either setting with its defaults
# (the moments arm, floats per source texel): the five kernel instances -- a source's moments plane is current only beside its temporal plane
ARMS = [("none", 3), ("none", 4), ("luminance", 3), ("luminance", 4), ("plane", 4)]
ARM_IDS = ["%s-%dch" % a for a in ARMS]


def source(stack, sphS, camS, camP, w, h, arm, channels):
    """A source context for one kernel instance: its colour plane at 3 passes with a NaN planted (3 floats a texel), or its temporal plane formed from
    a third view (4 floats) -- with its moments plane beside it (arm `plane`) or without.  Returns (the context, its side of the host call, src_m)."""
    S = stack.enter_context(context(sphS, camS, w, h))
    S.seed_stream(1)
    S.render_async(3 if channels == 3 else 2)
    planted(S)
    S.features_async()
    src_m = None
    if channels == 4:
        P = stack.enter_context(context(sphS, camP, w, h))
        P.render_async(2)
        P.features_async()
        if arm == "plane":
            S.set_temporal_moments(ON)
        S.reproject_async(P)
        if arm == "plane":
            src_m = S.read_moments()
    plane = S.read_temporal(packed=False) if channels == 4 else S.read_colors().reshape(h, w, 3)
    return S, {"plane": plane, "passes": S.current_sample, "feat": api.features_planes(sphS, camS, w, h), "cam": camS, "spheres": sphS}, src_m


def destination_side(D, sphD, camD):
    return {"plane": D.read_colors().reshape(D.h, D.w, 3) if D.current_sample else None, "passes": D.current_sample,
            "feat": api.features_planes(sphD, camD, D.w, D.h), "cam": camD, "spheres": sphD}


def assert_device_is_host(D, want, moments):
    """D's temporal plane, its packed plane (where the host's is a number), its moments plane and its flag plane are the host's (T, M, K)."""
    T, M, K = want
    got, px = D.read_temporal()
    assert_same_plane(got, T)
    number = ~np.isnan(T[..., 0:3]).any(axis=-1)[::-1].reshape(-1)
    assert np.array_equal(px[number], pack(np.nan_to_num(T[..., 0:3]).reshape(-1), D.w, D.h)[number])
    if moments:
        assert_same_plane(D.read_moments(), M)
    else:
        _refused(D, RT_ERR_STATE, D.read_moments)
    flags = D.read_history_flags()
    assert flags.dtype == np.uint8 and flags.shape == (D.h, D.w) and np.array_equal(flags, K)


def compare(stack, sphD, sphS, camD, camS, w, h, arm, channels, keeps=(2.0, 0.0), expect_flags=True):
    """One source, one destination at 2 passes and then at pass 0: the device against the host for every `keep`."""
    S, src, src_m = source(stack, sphS, camS, camD, w, h, arm, channels)
    D = stack.enter_context(context(sphS, camD, w, h))
    D.update_spheres(0, sphD)                                 # the records arrive as an update: the table rebuild is pending when the call comes
    moments = arm != "none"
    if moments:
        D.set_temporal_moments(ON)
    D.seed_stream(2)
    D.render_async(2)
    D.features_async()
    dst = destination_side(D, sphD, camD)
    before = snapshot(D), snapshot(S)
    for keep in keeps:
        want = api.reproject_shadow_planes(dst, src, w, h, src_m if moments else None, None, {"keep": keep})
        if expect_flags and w > 8:                            # no case is vacuous: flagged pixels, and pixels with history that are not
            took = want[0][..., 3] != F(2.0)
            assert want[2].any() and (took & (want[2] == 0)).any()
        if not expect_flags:
            assert not want[2].any()
        D.set_shadow_history({"keep": keep})
        D.reproject_async(S, None, D.stream if keep else None)
        assert_device_is_host(D, want, moments)
    assert_unchanged(D, before[0])
    assert_unchanged(S, before[1])
    # pass 0: a pure warp, nothing flagged (invariant c)
    D.reset()
    dst0 = dict(dst, plane=None, passes=0)
    want = api.reproject_shadow_planes(dst0, src, w, h, src_m if moments else None, None, ON)
    assert not want[2].any()
    D.set_shadow_history(ON)
    D.reproject_async(S)
    assert_device_is_host(D, want, moments)
    return D, S, src, dst


@pytest.mark.parametrize("arm,channels", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("name", ["demo_41x23_sphere", "demo_70x19_translated", "demo_1x1_translated"])
def test_the_device_equals_reproject_shadow_planes_bit_for_bit(name, arm, channels):
    """ONE pair (the light and the moved record 3).  41x23 and 70x19 have partial workgroups both ways; of the 1x1 image's workgroup one lane is
    inside, and the other 255 still reach both barriers."""
    sphD, sphS, camD, camS, w, h = records(name, "moved")
    assert api.shadow_history_pairs(sphS, sphD).tolist() == [[5, 3]]
    with contextlib.ExitStack() as stack:
        compare(stack, sphD, sphS, camD, camS, w, h, arm, channels)


@pytest.mark.parametrize("variant", ["radius", "light", "nan"])
def test_a_resized_record_a_moved_light_and_a_nan_centre(variant):
    """The light moved: five pairs, each record with it.  The NaN centre lives in D's records and tables alike."""
    sphD, sphS, camD, camS, w, h = records("demo_41x23_sphere", variant)
    assert len(api.shadow_history_pairs(sphS, sphD)) == {"radius": 1, "light": 5, "nan": 1}[variant]
    with contextlib.ExitStack() as stack:
        compare(stack, sphD, sphS, camD, camS, w, h, "plane", 4)


@pytest.mark.parametrize("arm,channels", [("none", 3), ("plane", 4)], ids=["none-3ch", "plane-4ch"])
@pytest.mark.parametrize("extra", [0, 1], ids=["one-chunk", "one-chunk-and-a-pair"])
def test_a_pair_list_of_exactly_one_chunk_and_of_one_pair_more(extra, arm, channels):
    n = api.SHADOW_PAIR_CHUNK + extra
    sphD, sphS, cam, w, h = dust(n)
    assert len(api.shadow_history_pairs(sphS, sphD)) == n
    with contextlib.ExitStack() as stack:
        compare(stack, sphD, sphS, cam, cam, w, h, arm, channels, keeps=(2.0,))


@pytest.mark.parametrize("arm,channels", [("none", 3), ("luminance", 4), ("plane", 4)], ids=["none-3ch", "luminance-4ch", "plane-4ch"])
def test_invariant_a_with_no_pair_the_planes_are_the_plain_ones_and_no_flag_is_set(arm, channels):
    sphD, sphS, camD, camS, w, h = records("demo_41x23_translated", "none")
    assert len(api.shadow_history_pairs(sphS, sphD)) == 0
    with contextlib.ExitStack() as stack:
        D, S, src, dst = compare(stack, sphD, sphS, camD, camS, w, h, arm, channels, keeps=(0.0,), expect_flags=False)
        D.render_async(2)
        D.reproject_async(S)
        T, px = D.read_temporal()
        assert not D.read_history_flags().any()
        M = D.read_moments() if arm != "none" else None
        D.set_shadow_history(None)
        D.reproject_async(S)
        T0, px0 = D.read_temporal()
        assert np.array_equal(np.isnan(T), np.isnan(T0)) and np.array_equal(bits(np.nan_to_num(T)), bits(np.nan_to_num(T0))) and np.array_equal(px, px0)
        if M is not None:
            assert np.array_equal(bits(np.nan_to_num(M)), bits(np.nan_to_num(D.read_moments())))


def test_invariant_b_and_the_setting_turned_off_again():
    """keep at max_history: T and M are the plain ones while K holds ones.  Then the setting off: the next call is the plain one bit for bit, launches
    what it launched before the setting existed, and leaves no flag plane to read."""
    sphD, sphS, camD, camS, w, h = records("demo_41x23_sphere", "moved")
    with contextlib.ExitStack() as stack:
        D, S, src, dst = compare(stack, sphD, sphS, camD, camS, w, h, "luminance", 4, keeps=(2.0,))
        D.seed_stream(2)
        D.render_async(2)
        dst = destination_side(D, sphD, camD)
        plain = api.reproject_moments_planes(dst, src, w, h, None)
        cut = api.reproject_shadow_planes(dst, src, w, h, None, None, ON)
        assert not np.array_equal(bits(np.nan_to_num(cut[0])), bits(np.nan_to_num(plain[0])))      # the setting does something here
        D.set_shadow_history({"keep": 64.0})
        D.reproject_async(S)
        assert_device_is_host(D, plain + (cut[2],), True)
        assert cut[2].any()
        D.set_shadow_history(ON)
        D.reproject_async(S)
        assert_device_is_host(D, cut, True)
        D.set_shadow_history(None)
        assert np.array_equal(D.read_history_flags(), cut[2])  # turning it off moves no plane
        D.reproject_async(S)
        assert_same_plane(D.read_temporal(packed=False), plain[0])
        assert_same_plane(D.read_moments(), plain[1])
        assert "rt_set_shadow_history" in _refused(D, RT_ERR_STATE, D.read_history_flags)
        D.set_temporal_moments(None)
        D.reproject_async(S)
        assert_same_plane(D.read_temporal(packed=False), api.reproject_planes(dst, src, w, h))


def test_when_the_flag_plane_is_current(tmp_path):
    sphD, sphS, camD, camS, w, h = records("demo_41x23_sphere", "moved")
    with context(sphS, camS, w, h) as S, context(sphD, camD, w, h) as D, context(sphD, camD, w, h) as a, context(sphD, camD, w, h) as b:
        S.render_async(3)
        S.features_async()
        for x, stream in ((a, 5), (b, 6)):
            x.seed_stream(stream)
            x.render_async(1)
        D.render_async(2)
        D.features_async()
        k = np.zeros((h, w), np.uint8)
        assert D._lib.rt_read_history_flags(D._h, None) == RT_ERR_ARG
        _refused(D, RT_ERR_STATE, D.read_history_flags)       # before any reprojection
        D.reproject_async(S)
        _refused(D, RT_ERR_STATE, D.read_history_flags)       # a reprojection with the setting off
        D.set_shadow_history(ON)
        _refused(D, RT_ERR_STATE, D.read_history_flags)       # turning it on forms nothing
        for bad in ({"keep": -1.0}, {"keep": float("nan")}, {"keep": float("inf")}):
            _refused(D, RT_ERR_ARG, D.set_shadow_history, bad)
        path = tmp_path / "state.bin"

        def form():
            D.reset()
            D.render_async(2)
            D.features_async()
            D.reproject_async(S)
            return D.read_history_flags()

        K = form()
        assert K.any() and not K.all()
        D.save_state(path)
        col, seeds = D.read_colors(), D.read_seeds()
        enders = {
            "rt_render_async": lambda: D.render_async(1, D.stream),
            "rt_reset": lambda: D.reset(),
            "rt_seed_stream_async": lambda: D.seed_stream(3, D.stream),
            "rt_write_state": lambda: D.write_state(col, seeds, 2),
            "rt_load_state": lambda: D.load_state(path),
            "rt_merge_async": lambda: D.merge([a], D.stream),
            "rt_denoise_async": lambda: D.denoise(a, b),
            "rt_set_camera": lambda: D.set_camera(camD),
            "rt_set_scene": lambda: D.set_scene(sphD),
            "rt_update_spheres_async": lambda: D.update_spheres(1, sphD[1:2]),
        }
        for name, end in enders.items():
            assert np.array_equal(form(), K), name            # accepted after a new reprojection with the setting on
            end()
            _refused(D, RT_ERR_STATE, D.read_history_flags)
            _refused(D, RT_ERR_STATE, D.read_temporal)
        # what keeps it: the settings, the filter, readers
        form()
        for keep in (lambda: D.set_shadow_history({"keep": 5.0}), lambda: D.set_shadow_history(None), lambda: D.atrous_async(), lambda: D.read_temporal(),
                     lambda: D.set_temporal_moments(ON)):
            keep()
            assert np.array_equal(D.read_history_flags(), K)
        D.reproject_async(S)                                  # ... and a reprojection with the setting off ends it and leaves T
        _refused(D, RT_ERR_STATE, D.read_history_flags)
        D.read_temporal()


def test_two_contexts_take_turns_for_four_frames_while_a_sphere_moves():
    """The interactive loop with both settings on: each frame moves record 3 a step on the OLDER context (rt_update_spheres_async), renders two passes
    on a stream of its own and reprojects from the other, whose temporal and moments planes are its history.  Device against host, frame by frame."""
    sphD, sph0, camD, cam, w, h = records("demo_41x23_sphere", "none")
    step = np.array((4.0, 0.5, -1.0), F)
    with context(sph0, cam, w, h) as A, context(sph0, cam, w, h) as B:
        ctx, sph = (A, B), {0: sph0.copy(), 1: sph0.copy()}
        for c in ctx:
            c.set_temporal_moments(ON)
            c.set_shadow_history(ON)
        A.render_async(3)
        planted(A)
        A.features_async()
        T = M = None
        flagged = 0
        for frame in range(1, 5):
            which = frame % 2
            D, S = ctx[which], ctx[1 - which]
            sph[which] = sph0.copy()
            sph[which]["p"][3] += F(frame) * step
            D.update_spheres(3, sph[which][3:4])
            D.seed_stream(frame + 1)
            D.features_async()
            D.render_async(2)
            src = {"plane": T if T is not None else S.read_colors().reshape(h, w, 3), "passes": S.current_sample,
                   "feat": api.features_planes(sph[1 - which], cam, w, h), "cam": cam, "spheres": sph[1 - which]}
            dst = destination_side(D, sph[which], cam)
            D.reproject_async(S, None, D.stream)
            want = api.reproject_shadow_planes(dst, src, w, h, M, None, ON)
            assert_device_is_host(D, want, True)
            T, M = want[0], want[1]
            flagged += int(want[2].sum())
            assert want[2].any() and not want[2].all()
        assert flagged > 20
