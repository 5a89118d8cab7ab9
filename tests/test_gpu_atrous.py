"""The edge-avoiding wavelet filter on the device (include/rt_api.h "edge-avoiding wavelet filter", csrc/rt_atrous.hip).  Every comparison is of bits:
rt_read_atrous after rt_atrous_async against rt_atrous_planes on the read-back input plane and rt_features_planes (which tests/test_atrous_cpu.py holds
to a numpy restatement of rules 20-23), the packed plane against the oracle's toInt of the host plane -- and, for a fast context, against the fast pack
kernel; then what the call leaves alone, the plane's currency, the contexts, states and parameters the calls refuse, and three frames of the
interactive loop with and without the filter."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api, host
from test_atrous_cpu import PARAMS, assert_same_plane
from test_gpu_feature_planes import context
from test_gpu_reproject import planted
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, pack, snapshot
from test_gpu_tiles import S1, select
from test_reproject_cpu import F, geometry, sideways

pytestmark = pytest.mark.gpu

SIZES = ["41x23", "70x19", "1x1", "96x96"]
INPUTS = ["colour", "temporal", "temporal_pass0"]


def formed(stack, size, kind, mode=None):
    """A context whose filter input is of `kind`, at the new view of the Demo scene's translated geometry: its colour plane at 3 passes with a NaN
    planted; its temporal plane over 2 passes with a NaN planted; or the temporal plane of a context at pass 0, whose pixels without history hold
    n == 0.  Returns (context, feature plane, the input as the host reads it, the passes the colour plane holds)."""
    sphD, sphS, camD, camS, w, h = geometry("demo_%s_translated" % size)
    D = stack.enter_context(context(sphD, camD, w, h, mode))
    passes = {"colour": 3, "temporal": 2, "temporal_pass0": 0}[kind]
    if passes:
        D.seed_stream(2)
        D.render_async(passes)
        planted(D)
    D.features_async()
    if kind == "colour":
        U = D.read_colors().reshape(h, w, 3)
    else:
        S = stack.enter_context(context(sphS, camS, w, h))
        S.render_async(3)
        S.features_async()
        D.reproject_async(S)
        U = D.read_temporal(packed=False)
        if kind == "temporal_pass0" and w > 8:
            assert (U[..., 3] == 0).any() and (U[..., 3] > 0).any()
    if w > 8 and passes:
        assert np.isnan(U).any()
    return D, api.features_planes(sphD, camD, w, h), U, passes


def assert_device_is_host(ctx, want):
    """ctx's filtered plane is `want` bit for bit, and its packed plane the oracle's toInt of `want` (where `want` is a number)."""
    got, px = ctx.read_atrous()
    assert_same_plane(got, want)
    number = ~np.isnan(want[..., 0:3]).any(axis=-1)[::-1].reshape(-1)            # (the packed plane's rows: row 0 = bottom)
    assert np.array_equal(px[number], pack(np.nan_to_num(want[..., 0:3]).reshape(-1), ctx.w, ctx.h)[number])
    return got


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("size", SIZES)
def test_the_device_equals_atrous_planes_bit_for_bit(size, kind):
    """41x23 and 70x19 have partial tiles in both directions and, with five levels, steps beyond the image; 1x1 has the centre tap alone; 96x96 is
    three workgroups by twelve."""
    with contextlib.ExitStack() as stack:
        D, feat, U, passes = formed(stack, size, kind)
        before = snapshot(D)
        for params in PARAMS:
            want = api.atrous_planes(U, feat, D.w, D.h, passes, params or None)
            D.atrous_async(params or None)                    # the default stream
            first = assert_device_is_host(D, want)
            D.atrous_async(params or None, D.stream)          # the context's stream: the same words
            assert np.array_equal(bits(D.read_atrous(packed=False)), bits(first))
        want = api.atrous_planes(U, feat, D.w, D.h, passes, {"levels": 0})
        D.atrous_async({"levels": 0})
        assert_same_plane(assert_device_is_host(D, want)[..., 0:3], U[..., 0:3])      # rule 23: U's rgb bit for bit
        assert_unchanged(D, before)


@pytest.mark.parametrize("kind", ["colour", "temporal"])
def test_a_fast_context_packs_with_fast_modes_to_int(kind):
    """The float plane is the host's all the same; the packed plane is what fast mode's pack kernel makes of those floats, and with no level it is
    the temporal plane's own packed plane."""
    with contextlib.ExitStack() as stack:
        D, feat, U, passes = formed(stack, "41x23", kind, api.RT_MODE_FAST)
        w, h = D.w, D.h
        X = stack.enter_context(context(host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h), w, h, api.RT_MODE_FAST))
        differs = 0
        for params in PARAMS + [{"levels": 0}]:
            D.atrous_async(params or None)
            A, px = D.read_atrous()
            assert_same_plane(A, api.atrous_planes(U, feat, w, h, passes, params or None))
            number = ~np.isnan(A[..., 0:3]).any(axis=-1)[::-1].reshape(-1)
            X.write_state(np.nan_to_num(A[..., 0:3]).reshape(-1), X.read_seeds(), 1)
            assert np.array_equal(px[number], X.read_pixels()[number])
            differs += int((px[number] != pack(np.nan_to_num(A[..., 0:3]).reshape(-1), w, h)[number]).sum())
            if kind == "temporal" and params == {"levels": 0}:
                assert np.array_equal(px[number], D.read_temporal()[1][number])
        print("fast and parity toInt differ in %d packed words" % differs)


def whole(ctx):
    return snapshot(ctx), ctx.read_pixels().copy(), ctx.stats(), ctx.last_kernel, bits(ctx.read_features()).copy()


def test_nothing_else_of_the_context_changes():
    with contextlib.ExitStack() as stack:
        D, feat, U, passes = formed(stack, "41x23", "temporal")
        T, Tpx = D.read_temporal()
        was = whole(D)
        D.atrous_async()
        D.read_atrous()
        D.atrous_async({"levels": 5}, D.stream)
        D.read_atrous()
        now = whole(D)
        assert_unchanged(D, was[0])
        assert np.array_equal(now[1], was[1]) and now[2] == was[2] and now[3] == was[3] and np.array_equal(now[4], was[4])
        T2, Tpx2 = D.read_temporal()
        assert np.array_equal(bits(T2), bits(T)) and np.array_equal(Tpx2, Tpx)
        # the render goes on from the colour plane, not from A
        D.render_pass(1)
        assert D.current_sample == passes + 1


def test_what_ends_the_filtered_plane_and_what_keeps_it(tmp_path):
    sphD, sphS, camD, camS, w, h = geometry("demo_41x23_translated")
    with context(sphS, camS, w, h) as S, context(sphD, camD, w, h) as D, context(sphD, camD, w, h) as a, context(sphD, camD, w, h) as b:
        S.render_async(3)
        S.features_async()
        a.seed_stream(5)
        a.render_async(1)
        b.seed_stream(6)
        b.render_async(1)
        _refused(D, RT_ERR_STATE, D.read_atrous)              # never formed
        path = tmp_path / "state.bin"

        def form(temporal=True):
            D.reset()
            D.render_async(2)
            D.features_async()
            if temporal:
                D.reproject_async(S)
            D.atrous_async()
            D.read_atrous()

        form()
        D.save_state(path)
        col, seeds = D.read_colors(), D.read_seeds()

        def subset():
            D.select_tiles(None, 0, D.stream)
            D.render_tiles_async(1, D.stream)

        enders = {
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
            "rt_reproject_async": lambda: D.reproject_async(S),
        }
        for temporal in (True, False):                        # filtered from the temporal plane, and from the colour plane
            for name, end in enders.items():
                form(temporal)
                end()
                assert "rt_atrous_async" in _refused(D, RT_ERR_STATE, D.read_atrous), (name, temporal)
        for name, end in {"rt_set_camera": lambda: D.set_camera(camD), "rt_set_scene": lambda: D.set_scene(sphD),
                          "rt_update_spheres_async": lambda: D.update_spheres(1, sphD[1:2])}.items():
            form()
            end()
            _refused(D, RT_ERR_STATE, D.read_atrous)
            D.features_async()                                # a new feature plane does not bring the old filtered plane back
            _refused(D, RT_ERR_STATE, D.read_atrous)
        form()
        b.render_async(1)                                     # b at two passes, like D: a pair to cross-filter
        want = bits(D.read_atrous(packed=False)).copy()
        keepers = {
            "rt_read_pixels (packing)": lambda: D.read_pixels(),
            "rt_select_tiles": lambda: D.select_tiles(None, 0, D.stream),
            "rt_denoise_pair_async": lambda: D.denoise_pair(b),
            "a reprojection FROM it": lambda: a.features_async() or a.reproject_async(D),
            "rt_set_mode": lambda: D.set_mode(api.RT_MODE_FAST),
            "rt_features_async": lambda: D.features_async(D.stream),
            "rt_read_temporal": lambda: D.read_temporal(),
            "rt_read_atrous": lambda: D.read_atrous(),
        }
        for name, keep in keepers.items():
            keep()
            assert np.array_equal(bits(D.read_atrous(packed=False)), want), name
        D.read_temporal()                                     # and the temporal plane has outlived all of it


def test_the_contexts_states_and_parameters_the_calls_refuse():
    w, h = 41, 23
    sph = host.demo_scene()
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    lib = api.load_library()
    with context(sph, cam, w, h) as D, make("demo", w, h, rank=1, nranks=2) as shard, make("demo", w, h, devices=[0, 0]) as multi:
        D.render_async(2)
        D.features_async()
        snap = snapshot(D)

        def unchanged():
            assert_unchanged(D, snap)
            _refused(D, RT_ERR_STATE, D.read_atrous)          # and nothing was formed

        # RT_ERR_ARG: the contexts
        assert lib.rt_atrous_async(None, None, None) == RT_ERR_ARG and lib.rt_read_atrous(None, None, None) == RT_ERR_ARG
        for x in (shard, multi):
            _refused(x, RT_ERR_ARG, x.atrous_async)
            _refused(x, RT_ERR_ARG, x.read_atrous)
        # RT_ERR_ARG: the parameters
        nan, inf = float("nan"), float("inf")
        for name in ("k_lum", "k_normal"):
            for bad in (0.0, -2.0, nan, inf):
                assert name in _refused(D, RT_ERR_ARG, D.atrous_async, {name: bad})
        for bad in (-1, 6):
            assert "levels" in _refused(D, RT_ERR_ARG, D.atrous_async, {"levels": bad})
        p = api.atrous_defaults()
        p.reserved = 7
        assert "reserved" in _refused(D, RT_ERR_ARG, D.atrous_async, p)
        assert lib.rt_read_atrous(D._h, None, None) == RT_ERR_ARG
        unchanged()
        # RT_ERR_STATE: a stale feature plane
        D.set_camera(cam)
        assert "feature plane" in _refused(D, RT_ERR_STATE, D.atrous_async)
        D.features_async()
        unchanged()
        # ... neither a temporal plane nor a pass
        with context(sph, cam, w, h) as E:
            E.features_async()
            assert "neither" in _refused(E, RT_ERR_STATE, E.atrous_async)
            _refused(E, RT_ERR_STATE, E.read_atrous)
            E.reproject_async(D)                              # a pure warp: a temporal plane and still no pass
            E.atrous_async()
            assert_device_is_host(E, api.atrous_planes(E.read_temporal(packed=False), api.features_planes(sph, cam, w, h), w, h))
        # ... a ragged context
        with context(sph, cam, w, h) as R:
            R.features_async()
            R.render_async(2, R.stream)
            assert select(R, S1) == (4, 12)
            R.render_tiles_async(1, R.stream)
            snap_r = snapshot(R)
            assert "ragged" in _refused(R, RT_ERR_STATE, R.atrous_async)
            assert_unchanged(R, snap_r)
            _refused(R, RT_ERR_STATE, R.read_atrous)
        # what was refused left nothing half done
        D.atrous_async()
        assert_device_is_host(D, api.atrous_planes(D.read_colors().reshape(h, w, 3), api.features_planes(sph, cam, w, h), w, h, 2))


def interactive_loop(filtered):
    """A -> B -> A as the header's intended use has it, a filter after each reprojection (`filtered`); returns the three temporal planes."""
    w, h = 41, 23
    sph = host.demo_scene()
    o, t = host.DEMO_ORIG, host.DEMO_TARGET
    cams = [host.compute_camera(sideways(o, t, share), t, w, h) for share in (0.0, 0.02, 0.04)]
    frames, shown = [], []

    def show(ctx):
        frames.append(tuple(x.copy() for x in ctx.read_temporal()))
        if filtered:
            ctx.atrous_async(None, ctx.stream)
            shown.append(ctx.read_atrous(packed=False))

    with context(sph, cams[0], w, h) as A, context(sph, cams[1], w, h) as B:
        A.render_async(3)
        A.features_async()
        if filtered:
            A.atrous_async()                                  # frame 0 is shown filtered too: from the colour plane
        B.seed_stream(2)
        B.features_async()
        B.render_async(1)
        B.reproject_async(A, None, B.stream)
        show(B)
        A.set_camera(cams[2])
        A.seed_stream(3)
        A.features_async()
        A.render_async(1)
        A.reproject_async(B, None, A.stream)
        show(A)
        B.set_camera(cams[0])
        B.seed_stream(4)
        B.features_async()
        B.reproject_async(A)                                  # a pure warp of A's temporal plane: B holds no pass
        show(B)
        state = [snapshot(A), snapshot(B)]
    return frames, shown, state


def test_three_frames_of_the_interactive_loop_are_the_same_with_and_without_the_filter():
    """The filter feeds nothing back: every T, its packed plane, and both contexts' colours, seeds and pass numbers are what they are without it."""
    plain, _, state_plain = interactive_loop(False)
    with_filter, shown, state = interactive_loop(True)
    assert len(plain) == len(with_filter) == len(shown) == 3
    for (T0, px0), (T1, px1), A in zip(plain, with_filter, shown):
        assert np.array_equal(bits(T0), bits(T1)) and np.array_equal(px0, px1)
        assert not np.array_equal(bits(A[..., 0:3]), bits(T1[..., 0:3]))         # (and the filter did something)
    for s0, s1 in zip(state_plain, state):
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1]) and s0[2] == s1[2]


def test_contexts_that_filtered_give_their_planes_back():
    """Free device memory after a context that acquired the filter's five planes was closed is what it was before it, within the megabyte
    tests/test_gpu_state.py allows; while it is held, at least the three planes of four floats are gone (the two planes of one word may come out of a
    block the runtime holds already: only the large ones are sure to show)."""
    w, h = 1024, 512
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)

    def cycle():
        ctx = context(host.demo_scene(), cam, w, h)
        ctx.render_async(1)
        ctx.features_async()
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info(0)[0]
        ctx.atrous_async()
        ctx.read_atrous()
        torch.cuda.synchronize()
        return ctx, free - torch.cuda.mem_get_info(0)[0]

    ctx, _ = cycle()                                          # (a first cycle pays the process-wide allocations: not part of the baseline)
    ctx.close()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    ctx, held = cycle()
    assert held >= 3 * 4 * 4 * w * h
    ctx.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free_before - (1 << 20)
