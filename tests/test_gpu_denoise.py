"""Denoising on the device (include/rt_api.h "denoising", csrc/rt_denoise.hip).  Every comparison is of bits: rt_read_colors(dst) after
rt_denoise_async against rt_denoise_planes on the same three planes (which tests/test_denoise_cpu.py holds to a numpy restatement of the
rules).  Synthetic planes -- the non-finite ones included -- go in through rt_write_state: n passes on a and b, 2n on dst, as their merge
would hold; then rendered frames, merged whole and per tile."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as raytracing_simple_amd.dist does for the suite as a whole: torch
#                            brings a HIP runtime of its own, and it finds no device when the library's has initialised before it is even loaded)

from raytracing_simple_amd import api
from test_denoise_cpu import OTHER, PARAMS, assert_same_bits, planes, planted
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, pack, snapshot

pytestmark = pytest.mark.gpu

N = 3                     # passes the synthetic halves claim to hold


class Trio:
    """dst, a, b: three contexts of one size with the Demo scene; planes are written, not rendered."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.dst, self.a, self.b = make("demo", w, h), make("demo", w, h), make("demo", w, h)

    def write(self, D, A, B, n=N):
        self.a.write_state(A, None, n)
        self.b.write_state(B, None, n)
        self.dst.write_state(D, None, 2 * n)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for c in (self.dst, self.a, self.b):
            c.close()


def everything(ctx):
    """What a call that leaves a context alone leaves alone: colours, seeds, pass number, packed pixels, counters, tile counts, last kernel."""
    return snapshot(ctx) + (ctx.read_pixels().copy(), ctx.stats(), ctx.tile_passes().copy(), ctx.last_kernel)


def assert_everything_unchanged(ctx, before):
    now = everything(ctx)
    for got, want in zip(now, before):
        assert np.array_equal(got, want) if isinstance(want, np.ndarray) else got == want


def beside_colours(ctx):
    """What rt_denoise_async leaves of dst: everything but the colour plane and the pixels packed from it."""
    return ctx.read_seeds().copy(), ctx.current_sample, ctx.stats(), ctx.tile_passes().copy(), ctx.last_kernel


def assert_beside_colours_unchanged(ctx, before):
    for got, want in zip(beside_colours(ctx), before):
        assert np.array_equal(got, want) if isinstance(want, np.ndarray) else got == want


# ---- 1. synthetic planes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (41, 23), (70, 40), (523, 9)],
                         ids=["one-pixel", "one-partial-tile", "partial-tiles", "halo-taller-than-a-tile", "wide-single-strip"])
def test_the_device_equals_denoise_planes_bit_for_bit(w, h):
    cases = [("noisy", p) for p in PARAMS]
    if (w, h) == (41, 23):
        cases += [("noisy", OTHER)] + [(kind, p) for kind in ("equal", "nonfinite") for p in PARAMS]
    with Trio(w, h) as t:
        written = None
        for kind, params in cases:
            D, A, B = planes(w, h, kind)
            if written != kind:
                t.write(D, A, B)
                halves = everything(t.a), everything(t.b)
                written = kind
            else:
                t.dst.write_state(D, None, 2 * N)
            rest = beside_colours(t.dst)
            launches = t.dst.stats()["launches"]
            t.dst.denoise(t.a, t.b, params)
            got = t.dst.read_colors()
            want = api.denoise_planes(D, A, B, w, h, params)
            assert_same_bits(got, want)
            if w * h > 1 and kind == "noisy":
                assert not np.array_equal(bits(got), bits(D))
            assert_beside_colours_unchanged(t.dst, rest)
            assert t.dst.stats()["launches"] == launches
            assert_everything_unchanged(t.a, halves[0])
            assert_everything_unchanged(t.b, halves[1])
            if params is PARAMS[0]:                           # the packed frame follows: the oracle's toInt of the filtered plane
                assert np.array_equal(t.dst.read_pixels(), pack(got, w, h))
        if (w, h) == (41, 23):                                # the non-finite case ran last: exactly the planted values of D
            bad = np.zeros((h, w, 3), bool)
            for y, x, c, _ in planted(w, h):
                bad[y, x, c] = True
            assert np.array_equal(~np.isfinite(got).reshape(h, w, 3), bad)


def test_two_calls_on_rewritten_planes_give_the_same_bits_and_a_second_call_filters_the_filtered_plane():
    w, h = 41, 23
    D, A, B = planes(w, h)
    with Trio(w, h) as t:
        t.write(D, A, B)
        t.dst.denoise(t.a, t.b)
        first = t.dst.read_colors()
        assert_same_bits(first, api.denoise_planes(D, A, B, w, h))
        t.dst.denoise(t.a, t.b)                               # the planes have changed places: the call reads what the last one wrote
        assert_same_bits(t.dst.read_colors(), api.denoise_planes(first, A, B, w, h))
        t.dst.write_state(D, None, 2 * N)                     # ... and written again, into whichever plane is the colour plane now
        t.dst.denoise(t.a, t.b)
        assert np.array_equal(bits(t.dst.read_colors()), bits(first))
        t.dst.write_state(D, None, 2 * N)
        t.dst.denoise(t.a, t.b, api.denoise_defaults())
        assert np.array_equal(bits(t.dst.read_colors()), bits(first))


def test_radius_0_launches_nothing_and_leaves_dst_as_it_is():
    w, h = 41, 23
    D, A, B = planes(w, h, "nonfinite")
    with Trio(w, h) as t:
        t.write(D, A, B)
        before = everything(t.dst)
        for P in (0, 1, 2):
            t.dst.denoise(t.a, t.b, {"search_radius": 0, "patch_radius": P})
        assert_everything_unchanged(t.dst, before)
        assert_same_bits(t.dst.read_colors(), D)
        assert t.dst.stats()["launches"] == before[4]["launches"]


def test_on_the_callers_stream_a_read_on_that_stream_alone_sees_the_filtered_frame():
    w, h = 70, 40
    D, A, B = planes(w, h)
    with Trio(w, h) as t:
        t.write(D, A, B)
        want = pack(api.denoise_planes(D, A, B, w, h), w, h)
        stream = torch.cuda.Stream()
        out = np.zeros(w * h, np.uint32)
        t.dst.pin_output(out)
        t.dst.denoise(t.a, t.b, None, stream.cuda_stream)
        t.dst.read_pixels_async(out, stream.cuda_stream)
        stream.synchronize()                                  # the caller's stream and nothing else
        assert np.array_equal(out, want)
        t.dst.pin_output(None)
        t.dst.write_state(D, None, 2 * N)
        t.dst.denoise(t.a, t.b)                               # the null stream
        assert np.array_equal(t.dst.read_pixels(), want)


# ---- 2. rendered frames ------------------------------------------------------------------------------------------------
def test_rendered_merged_and_filtered_the_frame_gains_3_db():
    """Demo at 96x64: streams 1 and 2, 8 passes each, merged into a fresh context, filtered at the defaults; against 2048 passes of stream 3.
    The bound is the CPU test's: a little under half of what the arithmetic gained when it was prototyped (7.3 dB at 4 passes per half,
    5.1 at 16)."""
    w, h, n = 96, 64, 8
    with make("demo", w, h) as a, make("demo", w, h) as b, make("demo", w, h) as dst, make("demo", w, h) as ref:
        for ctx, s, passes in ((a, 1, n), (b, 2, n), (ref, 3, 2048)):
            ctx.seed_stream(s, ctx.stream)
            ctx.render_async(passes, ctx.stream)
        dst.merge([a, b], dst.stream)
        assert dst.current_sample == 2 * n
        A, B, D = a.read_colors(), b.read_colors(), dst.read_colors()
        before = api.error_psnr(dst.compare(ref))
        halves = everything(a), everything(b)
        dst.denoise(a, b, None, dst.stream)
        got = dst.read_colors()
        assert np.isfinite(got).all()
        assert_same_bits(got, api.denoise_planes(D, A, B, w, h))
        after = api.error_psnr(dst.compare(ref))
        print("\n[denoise] Demo 96x64, %d passes per half: merged %.2f dB, filtered %.2f dB (gain %.2f dB)" % (n, before, after, after - before))
        assert after - before >= 3.0
        assert_everything_unchanged(a, halves[0])
        assert_everything_unchanged(b, halves[1])
        assert dst.current_sample == 2 * n


def test_after_render_adaptive_the_per_tile_merge_is_filtered_like_any_other():
    """Demo at 96x64, at least 4 passes, 4 per check, at most 12, 16 dB per tile: by the oracle's frames 40 of the 96 tiles retire at 4 passes,
    16 at 8, and 40 render to 12 -- the pair is ragged, tile for tile alike."""
    w, h = 96, 64
    with make("demo", w, h) as a, make("demo", w, h) as b, make("demo", w, h) as dst:
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
        reached, _, _ = a.render_adaptive(b, 16.0, 4, 4, 12)
        passes = a.tile_passes()
        assert not reached and a.current_sample == b.current_sample == 12
        assert np.array_equal(passes, b.tile_passes()) and sorted(set(passes.reshape(-1).tolist())) == [4, 8, 12]
        dst.merge([a, b], dst.stream)
        assert dst.current_sample == 24 and np.array_equal(dst.tile_passes(), 2 * passes)
        A, B, D = a.read_colors(), b.read_colors(), dst.read_colors()
        rest = beside_colours(dst)
        dst.denoise(a, b)
        got = dst.read_colors()
        assert_same_bits(got, api.denoise_planes(D, A, B, w, h))
        assert not np.array_equal(bits(got), bits(D))
        assert_beside_colours_unchanged(dst, rest)
        assert np.array_equal(dst.tile_passes(), 2 * passes)
        assert np.array_equal(a.tile_passes(), passes) and np.array_equal(b.tile_passes(), passes)
        assert np.array_equal(dst.read_pixels(), pack(got, w, h))


# ---- 3. refusals change nothing ----------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_three_contexts_as_they_were():
    w, h = 41, 23
    D, A, B = planes(w, h)
    with Trio(w, h) as t, make("demo", 40, 23) as other_size, make("demo", w, h, rank=1, nranks=2) as shard, \
            make("demo", w, h, devices=[0, 0]) as multi:
        t.write(D, A, B)
        other_size.write_state(np.zeros(3 * 40 * 23, np.float32), None, N)
        dst, a, b = t.dst, t.a, t.b
        snaps = [snapshot(c) for c in (dst, a, b)]

        def refused(code, *args):
            text = _refused(dst, code, *args)
            for c, s in zip((dst, a, b), snaps):
                assert_unchanged(c, s)
            return text

        # RT_ERR_ARG: the contexts
        lib = api.load_library()
        for trio in ((None, a._h, b._h), (dst._h, None, b._h), (dst._h, a._h, None)):
            assert lib.rt_denoise_async(*trio, None, None) == RT_ERR_ARG and b"null" in lib.rt_last_error()
        for c, s in zip((dst, a, b), snaps):
            assert_unchanged(c, s)
        refused(RT_ERR_ARG, dst.denoise, dst, b)
        refused(RT_ERR_ARG, dst.denoise, a, dst)
        refused(RT_ERR_ARG, dst.denoise, a, a)
        refused(RT_ERR_ARG, dst.denoise, other_size, b)
        refused(RT_ERR_ARG, dst.denoise, a, other_size)
        refused(RT_ERR_ARG, other_size.denoise, a, b)
        for x in (shard, multi):
            refused(RT_ERR_ARG, dst.denoise, x, b)
            refused(RT_ERR_ARG, dst.denoise, a, x)
            refused(RT_ERR_ARG, x.denoise, a, b)
        if torch.cuda.device_count() > 1:
            with make("demo", w, h, device=1) as elsewhere:
                elsewhere.write_state(A, None, N)
                assert "device" in refused(RT_ERR_ARG, dst.denoise, elsewhere, b)
                assert "device" in refused(RT_ERR_ARG, dst.denoise, a, elsewhere)
        # RT_ERR_ARG: the parameters
        nan, inf = float("nan"), float("inf")
        for bad in ({"search_radius": -1}, {"search_radius": 9}, {"patch_radius": -1}, {"patch_radius": 3}, {"alpha": -0.25}, {"alpha": nan},
                    {"alpha": inf}, {"k": 0.0}, {"k": -1.0}, {"k": nan}, {"k": inf}):
            assert list(bad)[0] in refused(RT_ERR_ARG, dst.denoise, a, b, bad)
        # RT_ERR_STATE: the pass numbers
        b.write_state(B, None, N + 1)
        snaps[2] = snapshot(b)
        refused(RT_ERR_STATE, dst.denoise, a, b)              # the halves differ
        b.write_state(B, None, N)
        snaps[2] = snapshot(b)
        dst.write_state(D, None, 2 * N + 1)
        snaps[0] = snapshot(dst)
        assert "merge" in refused(RT_ERR_STATE, dst.denoise, a, b)      # dst is not their sum
        dst.write_state(D, None, N)
        snaps[0] = snapshot(dst)
        refused(RT_ERR_STATE, dst.denoise, a, b)
        a.write_state(None, None, 0)
        b.write_state(None, None, 0)
        dst.write_state(None, None, 0)
        snaps = [snapshot(c) for c in (dst, a, b)]
        refused(RT_ERR_STATE, dst.denoise, a, b)              # nobody holds a pass
        # ... and the call still works afterwards
        t.write(D, A, B)
        dst.denoise(a, b)
        assert_same_bits(dst.read_colors(), api.denoise_planes(D, A, B, w, h))

