"""Temporal luminance moments on the device (include/rt_api.h "temporal luminance moments", csrc/rt_reproject.hip, csrc/rt_atrous.hip).  Every comparison is of bits:
rt_read_temporal and rt_read_moments after rt_reproject_async against rt_reproject_moments_planes on the read-back inputs, rt_read_atrous after
rt_atrous_async against rt_atrous_moments_planes (tests/test_moments_cpu.py holds both to a numpy restatement of rules 25-28); then the invariants
the header states, the plane's currency, the refusals, what the calls leave alone, and the interactive loop with the setting on and off."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api, host
from test_atrous_cpu import assert_same_plane
from test_gpu_atrous import assert_device_is_host
from test_gpu_feature_planes import context
from test_gpu_reproject import planted
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, pack, snapshot
from test_reproject_cpu import F, sideways

pytestmark = pytest.mark.gpu

SIZES = ["41x23", "70x19", "1x1", "96x96"]
SHARES = (0.0, 0.02, 0.04, 0.05, 0.03)                       # the camera's sideways offset, frame by frame
ON = {}                                                       # rt_set_temporal_moments with the defaults


def cameras(w, h):
    o, t = host.DEMO_ORIG, host.DEMO_TARGET
    return [host.compute_camera(sideways(o, t, share), t, w, h) for share in SHARES]


class Loop:
    """Two contexts taking turns on the Demo scene as the header's INTENDED USE has it, and the host's statement of every frame beside them: frame 0
    is A at 3 passes (a NaN planted in its colour plane); step() moves the OLDER context to the next camera and seed stream, renders `passes` (a NaN
    planted), reprojects from the other and -- `check` -- holds T, the packed plane and M to rt_reproject_moments_planes bit for bit.  With
    `setting` None the contexts leave the feature off and the host states nothing: the twin of invariant (a)."""

    def __init__(self, stack, size, mode=None, setting=ON):
        self.w, self.h = (int(v) for v in size.split("x"))
        self.mode, self.setting = mode, setting
        self.sph = host.demo_scene()
        self.cams = cameras(self.w, self.h)
        self.ctx = [stack.enter_context(context(self.sph, self.cams[0], self.w, self.h, mode)) for _ in range(2)]
        for c in self.ctx:
            if setting is not None:
                c.set_temporal_moments(setting)
        A = self.ctx[0]
        A.render_async(3)
        planted(A)
        A.features_async()
        self.frame = 0
        self.cam = {0: self.cams[0]}                          # the camera each context stands at
        self.T = self.M = None                                # the host's planes of the context that was reprojected into last
        self.last = A

    def side(self, ctx, which):
        cam = self.cam[which]
        return {"feat": api.features_planes(self.sph, cam, self.w, self.h), "cam": cam, "spheres": self.sph}

    def step(self, passes, params=None, check=True, stream=False):
        self.frame += 1
        which = self.frame % 2
        D, S = self.ctx[which], self.ctx[1 - which]
        self.cam[which] = self.cams[self.frame]
        D.set_camera(self.cam[which])
        D.seed_stream(self.frame + 1)
        D.features_async()
        if passes:
            D.render_async(passes)
            planted(D)
        if self.setting is None:
            D.reproject_async(S, params, D.stream if stream else None)
            return D
        # what the source is read through: its temporal plane and (rule 25) its moments plane while they are current, else its colour plane
        src = self.side(S, 1 - which)
        if self.T is not None:
            src.update(plane=self.T, passes=S.current_sample)
        else:
            src.update(plane=S.read_colors().reshape(self.h, self.w, 3), passes=S.current_sample)
        dst = self.side(D, which)
        dst.update(plane=D.read_colors().reshape(self.h, self.w, 3) if passes else None, passes=passes)
        D.reproject_async(S, params, D.stream if stream else None)
        T, M = api.reproject_moments_planes(dst, src, self.w, self.h, self.M, params)
        if check:
            got, px = D.read_temporal()
            assert_same_plane(got, T)
            number = ~np.isnan(T[..., 0:3]).any(axis=-1)[::-1].reshape(-1)
            if self.mode is None:
                assert np.array_equal(px[number], pack(np.nan_to_num(T[..., 0:3]).reshape(-1), self.w, self.h)[number])
            assert_same_plane(D.read_moments(), M)
        self.T, self.M, self.last = T, M, D
        return D, T, M, dst["feat"]


@pytest.mark.parametrize("size", SIZES)
def test_the_device_equals_the_host_frame_by_frame(size):
    """41x23 and 70x19 have partial tiles both ways, 1x1 one lane, 96x96 is three workgroups by twelve.  Frame 1 reads its source through the colour
    plane (rule 25's fallback on 3 channels), frame 2 through the source's T and M, frame 3 runs rule 26's cap (max_history = 3), frame 4 is a pure
    warp: a destination at pass 0."""
    with contextlib.ExitStack() as stack:
        loop = Loop(stack, size)
        D, T, M, _ = loop.step(2)
        assert set(np.unique(M[..., 2])) <= {F(1.0), F(2.0)}
        D, T, M, _ = loop.step(1, stream=True)
        if loop.w > 8:
            assert (M[..., 2] == F(3.0)).any() and np.isnan(T).any()
        D, T3, M3, _ = loop.step(1, {"max_history": 3.0})
        if loop.w > 8:
            assert (T3[..., 3] == F(4.0)).any() and ((M3[..., 2] > F(1.0)) & (M3[..., 2] < F(4.0)) & (M3[..., 2] != F(2.0)) & (M3[..., 2] != F(3.0))).any()      # capped
        before = snapshot(D)
        D, T, M, _ = loop.step(0)
        assert D.current_sample == 0
        if loop.w > 8:
            assert (M[..., 2] == 0).any() and (M[..., 2] > 0).any() and not M[M[..., 2] == 0].view(np.uint32).any()     # no history at pass 0: four +0.0f
        assert_unchanged(loop.ctx[1], before)                 # the source of the last frame is what it was


@pytest.mark.parametrize("size", SIZES)
def test_the_filter_takes_its_variance_from_history_bit_for_bit(size):
    """Three reprojections: k reaches 4 where history held and stays at 1 where there is none, so k_min 1, 2 and 4 each split the frame."""
    with contextlib.ExitStack() as stack:
        loop = Loop(stack, size)
        loop.step(2, check=False)
        loop.step(1, check=False)
        D, T, M, feat = loop.step(1)
        w, h = loop.w, loop.h
        usable = np.isfinite(T[..., 0:3]).all(axis=-1) & (T[..., 3] > 0)
        before = snapshot(D)
        for k_min in (1.0, 2.0, 4.0):
            D.set_temporal_moments({"k_min": k_min})
            applies = usable & (M[..., 2] >= F(k_min))
            if w > 8:
                assert applies.any() and (~applies).any()     # both branches of rule 28
            for levels in (0, 3, 5):
                want = api.atrous_moments_planes(T, feat, w, h, 0, M, {"levels": levels}, {"k_min": k_min})
                D.atrous_async({"levels": levels}, D.stream if levels == 3 else None)
                got = assert_device_is_host(D, want)
                if levels == 0:                               # invariant (c)
                    plain = api.atrous_planes(T, feat, w, h, 0, {"levels": 0})
                    assert np.array_equal(got[..., 3][applies], M[..., 3][applies]) and np.array_equal(got[..., 3][~applies], plain[..., 3][~applies])
                elif w > 8 and k_min == 1.0:
                    assert not np.array_equal(np.nan_to_num(got), np.nan_to_num(api.atrous_planes(T, feat, w, h, 0, {"levels": levels})))
        # invariant (b): k_min beyond any k present is the plain filter; and so is the setting turned off again
        for setting in ({"k_min": 1e9}, None):
            D.set_temporal_moments(setting)
            for levels in (0, 3):
                D.atrous_async({"levels": levels})
                assert_device_is_host(D, api.atrous_planes(T, feat, w, h, 0, {"levels": levels}))
        assert_same_plane(D.read_moments(), M)                # turning the setting off moved no plane
        assert_unchanged(D, before)


def test_a_fast_context_packs_with_fast_modes_to_int():
    """The float planes are the host's all the same; the packed planes are what fast mode's pack kernel makes of those floats."""
    with contextlib.ExitStack() as stack:
        loop = Loop(stack, "41x23", api.RT_MODE_FAST)
        loop.step(2, check=False)
        loop.step(1, check=False)
        D, T, M, feat = loop.step(1, check=False)
        w, h = loop.w, loop.h
        X = stack.enter_context(context(loop.sph, loop.cams[0], w, h, api.RT_MODE_FAST))

        def fast_pack(rgb):
            X.write_state(np.nan_to_num(rgb).reshape(-1), X.read_seeds(), 1)
            return X.read_pixels()

        got, px = D.read_temporal()
        assert_same_plane(got, T)
        assert_same_plane(D.read_moments(), M)
        number = ~np.isnan(T[..., 0:3]).any(axis=-1)[::-1].reshape(-1)
        assert np.array_equal(px[number], fast_pack(T[..., 0:3])[number])
        for levels in (0, 3):
            D.atrous_async({"levels": levels})
            A, apx = D.read_atrous()
            assert_same_plane(A, api.atrous_moments_planes(T, feat, w, h, 0, M, {"levels": levels}))
            assert np.array_equal(apx[number], fast_pack(A[..., 0:3])[number])


def test_the_temporal_plane_is_the_same_with_the_setting_on_or_off():
    """Invariant (a), frame by frame through the cap and the pure warp: T and its packed plane of a twin pair of contexts with the setting off."""
    with contextlib.ExitStack() as stack:
        on, off = Loop(stack, "41x23"), Loop(stack, "41x23", setting=None)
        for passes, params in ((2, None), (1, None), (1, {"max_history": 3.0}), (0, None)):
            D1, D0 = on.step(passes, params, check=False)[0], off.step(passes, params)
            (T1, px1), (T0, px0) = D1.read_temporal(), D0.read_temporal()
            assert np.array_equal(np.isnan(T1), np.isnan(T0)) and np.array_equal(bits(np.nan_to_num(T1)), bits(np.nan_to_num(T0))) and np.array_equal(px1, px0)
            _refused(D0, RT_ERR_STATE, D0.read_moments)
            assert_same_plane(D1.read_moments(), on.M)


def whole(ctx):
    return snapshot(ctx), ctx.read_pixels().copy(), ctx.stats(), ctx.last_kernel, bits(ctx.read_features()).copy()


def test_when_the_moments_plane_is_current(tmp_path):
    sph = host.demo_scene()
    w, h = 41, 23
    cams = cameras(w, h)
    with context(sph, cams[0], w, h) as S, context(sph, cams[1], w, h) as D, context(sph, cams[1], w, h) as a, context(sph, cams[1], w, h) as b:
        S.render_async(3)
        S.features_async()
        for x, stream in ((a, 5), (b, 6)):
            x.seed_stream(stream)
            x.render_async(1)
        D.render_async(2)
        D.features_async()
        assert "rt_set_temporal_moments" in _refused(D, RT_ERR_STATE, D.read_moments)      # before any reprojection
        D.reproject_async(S)
        _refused(D, RT_ERR_STATE, D.read_moments)             # a reprojection with the setting off
        D.set_temporal_moments(ON)
        _refused(D, RT_ERR_STATE, D.read_moments)             # turning it on forms nothing
        D.read_temporal()
        path = tmp_path / "state.bin"

        def form():
            D.reset()
            D.render_async(2)
            D.features_async()
            D.reproject_async(S)
            return D.read_moments()

        form()
        D.save_state(path)
        col, seeds = D.read_colors(), D.read_seeds()
        enders = {
            "rt_render_async": lambda: D.render_async(1, D.stream),
            "rt_render_pass": lambda: D.render_pass(1),
            "rt_reset": lambda: D.reset(),
            "rt_reset_async": lambda: D.reset_async(D.stream),
            "rt_seed_stream_async": lambda: D.seed_stream(3, D.stream),
            "rt_write_state": lambda: D.write_state(col, seeds, 2),
            "rt_load_state": lambda: D.load_state(path),
            "rt_merge_async": lambda: D.merge([a], D.stream),
            "rt_denoise_async": lambda: D.denoise(a, b),
            "rt_set_camera": lambda: D.set_camera(cams[1]),
            "rt_set_scene": lambda: D.set_scene(sph),
            "rt_update_spheres_async": lambda: D.update_spheres(1, sph[1:2]),
        }
        for name, end in enders.items():
            form()                                            # accepted after a new reprojection with the setting on
            end()
            _refused(D, RT_ERR_STATE, D.read_moments)
            _refused(D, RT_ERR_STATE, D.read_temporal)
        form()
        D.set_camera(cams[1])
        D.features_async()                                    # a feature plane formed again does not bring M back
        _refused(D, RT_ERR_STATE, D.read_moments)
        # what keeps it: the setting itself, the filter, readers, a reprojection FROM the context
        M = form()
        snap_d, snap_s = whole(D), whole(S)
        keepers = {
            "another k_min": lambda: D.set_temporal_moments({"k_min": 2.0}),
            "the setting off": lambda: D.set_temporal_moments(None),
            "rt_atrous_async": lambda: D.atrous_async(),
            "the setting on again": lambda: D.set_temporal_moments(ON),
            "rt_read_temporal": lambda: D.read_temporal(),
            "rt_read_atrous": lambda: D.atrous_async() or D.read_atrous(),
            "a reprojection FROM it": lambda: a.features_async() or a.reproject_async(D),
        }
        for name, keep in keepers.items():
            keep()
            assert np.array_equal(bits(D.read_moments()), bits(M)), name
        for ctx, was in ((D, snap_d), (S, snap_s)):           # nothing else of either context has moved
            now = whole(ctx)
            assert_unchanged(ctx, was[0])
            assert np.array_equal(now[1], was[1]) and now[2] == was[2] and now[3] == was[3] and np.array_equal(now[4], was[4])
        # a reprojection into the context with the setting off ends M and leaves T
        D.set_temporal_moments(None)
        D.reproject_async(S)
        _refused(D, RT_ERR_STATE, D.read_moments)
        D.read_temporal()


def test_a_source_whose_temporal_plane_was_formed_without_moments_counts_as_one_frame():
    """S's T is current but was formed with the setting off: D reads it by rule 25's fallback (the 4-channel luminance instance), so k = 2 after one
    blend wherever history held -- and the device is the host with src_m = NULL."""
    sph = host.demo_scene()
    w, h = 41, 23
    cams = cameras(w, h)
    with context(sph, cams[0], w, h) as P, context(sph, cams[1], w, h) as S, context(sph, cams[2], w, h) as D:
        P.render_async(3)
        P.features_async()
        S.seed_stream(2)
        S.render_async(2)
        S.features_async()
        S.reproject_async(P)                                  # the setting is off for S
        TS = S.read_temporal(packed=False)
        D.set_temporal_moments(ON)
        D.seed_stream(3)
        D.render_async(1)
        planted(D)
        D.features_async()
        D.reproject_async(S)
        dst = {"plane": D.read_colors().reshape(h, w, 3), "passes": 1, "feat": api.features_planes(sph, cams[2], w, h), "cam": cams[2], "spheres": sph}
        src = {"plane": TS, "passes": 2, "feat": api.features_planes(sph, cams[1], w, h), "cam": cams[1], "spheres": sph}
        T, M = api.reproject_moments_planes(dst, src, w, h, None)
        assert_same_plane(D.read_temporal(packed=False), T)
        got = D.read_moments()
        assert_same_plane(got, M)
        took = T[..., 3] != F(1.0)
        assert took.mean() > 0.5 and np.array_equal(got[..., 2], np.where(took, F(2.0), F(1.0)))
        # ... and turning S's setting on now changes nothing: its T was formed without M
        S.set_temporal_moments(ON)
        D.reproject_async(S)
        assert_same_plane(D.read_moments(), M)


def test_the_contexts_and_parameters_the_calls_refuse():
    w, h = 41, 23
    sph = host.demo_scene()
    cam = cameras(w, h)[0]
    lib = api.load_library()
    with context(sph, cam, w, h) as D, context(sph, cam, w, h) as S, make("demo", w, h, rank=1, nranks=2) as shard, make("demo", w, h, devices=[0, 0]) as multi:
        S.render_async(2)
        S.features_async()
        D.render_async(1)
        D.features_async()
        D.set_temporal_moments({"k_min": 2.0})
        D.reproject_async(S)
        M = D.read_moments()
        snap = snapshot(D)
        assert lib.rt_set_temporal_moments(None, None) == RT_ERR_ARG and lib.rt_read_moments(None, None) == RT_ERR_ARG
        for x in (shard, multi):
            _refused(x, RT_ERR_ARG, x.set_temporal_moments, ON)
            _refused(x, RT_ERR_ARG, x.set_temporal_moments, None)
            _refused(x, RT_ERR_ARG, x.read_moments)
        nan, inf = float("nan"), float("inf")
        for bad in (0.0, 0.999, -4.0, nan, inf):
            assert "k_min" in _refused(D, RT_ERR_ARG, D.set_temporal_moments, {"k_min": bad})
        p = api.moments_defaults()
        p.reserved[2] = 9
        assert "reserved" in _refused(D, RT_ERR_ARG, D.set_temporal_moments, p)
        assert lib.rt_read_moments(D._h, None) == RT_ERR_ARG
        # the other structures' reserved words keep being refused
        rp = api.reproject_defaults()
        rp.reserved[0] = 1
        assert "reserved" in _refused(D, RT_ERR_ARG, D.reproject_async, S, rp)
        ap = api.atrous_defaults()
        ap.reserved = 1
        assert "reserved" in _refused(D, RT_ERR_ARG, D.atrous_async, ap)
        # a refused call changed nothing: the setting is still k_min 2, M and T are what they were
        assert_unchanged(D, snap)
        assert np.array_equal(bits(D.read_moments()), bits(M))
        T = D.read_temporal(packed=False)
        feat = api.features_planes(sph, cam, w, h)
        D.atrous_async()
        assert_device_is_host(D, api.atrous_moments_planes(T, feat, w, h, 0, M, None, {"k_min": 2.0}))


def interactive_loop(setting):
    """tests/test_gpu_atrous.py's three frames A -> B -> A, a filter after each reprojection, with the setting as given on both contexts; returns the
    temporal planes, the filtered planes and what is left of the two contexts."""
    w, h = 41, 23
    sph = host.demo_scene()
    cams = cameras(w, h)
    frames, shown = [], []

    def show(ctx):
        frames.append(tuple(x.copy() for x in ctx.read_temporal()))
        ctx.atrous_async(None, ctx.stream)
        shown.append(tuple(x.copy() for x in ctx.read_atrous()))

    with context(sph, cams[0], w, h) as A, context(sph, cams[1], w, h) as B:
        for ctx in (A, B):
            if setting is not None:
                ctx.set_temporal_moments(setting)
        A.render_async(3)
        A.features_async()
        A.atrous_async()                                      # frame 0 is shown filtered too: from the colour plane, where M is not consulted
        shown.append(tuple(x.copy() for x in A.read_atrous()))
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
        state = [whole(A), whole(B)]
    return frames, shown, state


def test_the_interactive_loop_is_the_same_with_the_setting_on_as_off():
    """Colour planes, seeds, pass numbers, pixels, counters and every T with the setting on (at k_min 2, which the first reprojection reaches, and at
    one no pixel reaches) are what they are with it off; with the unreachable k_min every filtered frame is too (invariant b), with k_min 2 every frame
    filtered from a temporal plane differs."""
    plain, shown_plain, state_plain = interactive_loop(None)
    for setting in ({"k_min": 2.0}, {"k_min": 1e9}):
        with_, shown, state = interactive_loop(setting)
        assert len(plain) == len(with_) == 3 and len(shown) == len(shown_plain) == 4
        for (T0, px0), (T1, px1) in zip(plain, with_):
            assert np.array_equal(bits(T0), bits(T1)) and np.array_equal(px0, px1)
        for s0, s1 in zip(state_plain, state):
            assert np.array_equal(s0[0][0], s1[0][0]) and np.array_equal(s0[0][1], s1[0][1]) and s0[0][2] == s1[0][2]
            assert np.array_equal(s0[1], s1[1]) and s0[2] == s1[2] and s0[3] == s1[3] and np.array_equal(s0[4], s1[4])
        same = [np.array_equal(bits(a0), bits(a1)) and np.array_equal(p0, p1) for (a0, p0), (a1, p1) in zip(shown_plain, shown)]
        assert same[0]                                        # filtered from the colour plane: M is not consulted
        assert same[1:] == [setting["k_min"] > 8.0] * 3


def test_contexts_that_used_the_feature_give_their_planes_back():
    """As tests/test_gpu_atrous.py checks for A: free device memory after a context that acquired T, M and the filter's planes was closed is what it
    was before it, within the megabyte tests/test_gpu_state.py allows; while it is held, at least T, M and the filter's three planes of four floats
    are gone."""
    w, h = 1024, 512
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)

    with context(host.demo_scene(), cam, w, h) as S:
        S.render_async(1)
        S.features_async()

        def cycle():
            ctx = context(host.demo_scene(), cam, w, h)
            ctx.set_temporal_moments(ON)
            ctx.render_async(1)
            ctx.features_async()
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info(0)[0]
            ctx.reproject_async(S)
            ctx.read_moments()
            ctx.atrous_async()
            ctx.read_atrous()
            torch.cuda.synchronize()
            return ctx, free - torch.cuda.mem_get_info(0)[0]

        ctx, _ = cycle()                                      # (a first cycle pays the process-wide allocations: not part of the baseline)
        ctx.close()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        ctx, held = cycle()
        assert held >= 5 * 4 * 4 * w * h
        ctx.close()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] >= free_before - (1 << 20)
