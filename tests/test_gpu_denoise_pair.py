"""The error of the filtered frame on the device (include/rt_api.h "the error of the filtered frame", csrc/rt_denoise.hip, csrc/rt_compare.hip).
Every comparison is of bits: rt_read_filtered of both contexts after rt_denoise_pair_async against rt_denoise_pair_planes on the same two planes
(which tests/test_denoise_pair_cpu.py holds to a numpy restatement of the rules), and rt_compare_filtered against the integer metric computed in
numpy over the oracle's toInt of those host planes.  Synthetic planes go in through rt_write_state, as in tests/test_gpu_denoise.py; then the two
loops on rendered frames of the Demo scene."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

import test_tiles_cpu as T
from raytracing_simple_amd import api
from test_compare_cpu import frame_error_restated
from test_denoise_cpu import OTHER, PARAMS, assert_same_bits, planes
from test_denoise_pair_cpu import demo_halves
from test_gpu_denoise import assert_everything_unchanged, everything
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_unchanged, bits, make, pack, snapshot

pytestmark = pytest.mark.gpu

N = 3                     # passes the synthetic halves claim to hold


class Halves:
    """a, b (and, where a test asks, more): contexts of one size with the Demo scene; planes are written, not rendered."""

    def __init__(self, w, h, extra=0):
        self.w, self.h = w, h
        self.all = [make("demo", w, h) for _ in range(2 + extra)]
        self.a, self.b = self.all[:2]

    def write(self, A, B, n=N):
        self.a.write_state(A, None, n)
        self.b.write_state(B, None, n)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for c in self.all:
            c.close()


def metric_of(FA, FB, w, h):
    """rt_compare's metric and tile map over the oracle's toInt of two host planes, in the pixel buffer's layout."""
    return frame_error_restated(pack(FA, w, h), pack(FB, w, h), w, h)


def stale(a, b):
    """Both ways of asking for a's plane say RT_ERR_STATE."""
    _refused(a, RT_ERR_STATE, a.read_filtered)
    _refused(a, RT_ERR_STATE, a.compare_filtered, b)
    _refused(a, RT_ERR_STATE, b.compare_filtered, a)


# ---- 1. synthetic planes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (41, 23), (70, 40), (523, 9)],
                         ids=["one-pixel", "one-partial-tile", "partial-tiles", "halo-taller-than-a-tile", "wide-single-strip"])
def test_the_device_equals_pair_planes_bit_for_bit(w, h):
    cases = [("noisy", p) for p in PARAMS]
    if (w, h) == (41, 23):
        cases += [("noisy", OTHER)] + [("nonfinite", p) for p in PARAMS]
    with Halves(w, h) as t:
        written = None
        for kind, params in cases:
            D, A, B = planes(w, h, kind)
            if kind == "nonfinite":
                A = D                                         # the half with a NaN, +inf and -inf planted; the other half is finite
            if written != kind:
                t.write(A, B)
                before = everything(t.a), everything(t.b)
                written = kind
            t.a.denoise_pair(t.b, params)
            got = t.a.read_filtered(), t.b.read_filtered()
            want = api.denoise_pair_planes(A, B, w, h, params)
            for g, wnt, X in zip(got, want, (A, B)):
                assert_same_bits(g, wnt)
                if kind == "noisy":
                    assert np.array_equal(bits(g), bits(wnt))
                    if w * h > 1:
                        assert not np.array_equal(bits(g), bits(X))
            # the packed words: the oracle's toInt of those planes, through the integer metric (at 41x23 with the tile map)
            want_err, want_tiles = metric_of(want[0], want[1], w, h)
            if (w, h) == (41, 23):
                err, tiles = t.a.compare_filtered(t.b, tiles=True)
                assert err == want_err and np.array_equal(tiles, want_tiles)
            assert t.a.compare_filtered(t.b) == want_err
            if w * h > 1 and kind == "noisy":
                assert want_err["differing"] > 0
            assert_everything_unchanged(t.a, before[0])
            assert_everything_unchanged(t.b, before[1])
        if (w, h) == (41, 23):                                # the non-finite case ran last: non-finite exactly where the half is, the other finite
            assert np.array_equal(~np.isfinite(got[0]), ~np.isfinite(A)) and np.isfinite(got[1]).all()


def test_radius_0_copies_the_halves_and_swapped_contexts_swap_the_planes():
    w, h = 41, 23
    D, _, B = planes(w, h, "nonfinite")
    with Halves(w, h) as t:
        t.write(D, B)
        for P in (0, 1, 2):
            t.a.denoise_pair(t.b, {"search_radius": 0, "patch_radius": P})
            assert_same_bits(t.a.read_filtered(), D)
            assert np.array_equal(bits(t.b.read_filtered()), bits(B))
            assert t.a.compare_filtered(t.b) == metric_of(D, B, w, h)[0]
        _, A, B = planes(w, h)
        t.write(A, B)
        t.a.denoise_pair(t.b)
        first = bits(t.a.read_filtered()).copy(), bits(t.b.read_filtered()).copy()
        err = t.a.compare_filtered(t.b)
        t.b.denoise_pair(t.a)                                 # b as the first half: the same two planes, each in its own context still
        assert np.array_equal(bits(t.a.read_filtered()), first[0]) and np.array_equal(bits(t.b.read_filtered()), first[1])
        assert t.b.compare_filtered(t.a) == err


def test_two_calls_give_the_same_bits_and_a_read_on_the_callers_stream_alone_sees_the_planes():
    w, h = 70, 40
    _, A, B = planes(w, h)
    with Halves(w, h) as t:
        t.write(A, B)
        t.a.denoise_pair(t.b)
        first = bits(t.a.read_filtered()).copy(), bits(t.b.read_filtered()).copy()
        want, want_tiles = t.a.compare_filtered(t.b, tiles=True)
        assert (want, want_tiles.tolist()) == (lambda e, m: (e, m.tolist()))(*metric_of(*api.denoise_pair_planes(A, B, w, h), w, h))
        t.a.denoise_pair(t.b)
        assert np.array_equal(bits(t.a.read_filtered()), first[0]) and np.array_equal(bits(t.b.read_filtered()), first[1])
        # on the caller's stream: the planes are rewritten with another filter, and the comparison queued behind it on that stream sees them
        other = {"search_radius": 2, "patch_radius": 0}
        stream = torch.cuda.Stream()
        res = torch.full((12,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tiles = torch.full(want_tiles.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.a.denoise_pair(t.b, other, stream.cuda_stream)
        t.a.compare_filtered_async(t.b, res.data_ptr(), tiles.data_ptr(), stream.cuda_stream)
        stream.synchronize()                                  # the caller's stream and nothing else
        want2, want_tiles2 = metric_of(*api.denoise_pair_planes(A, B, w, h, other), w, h)
        assert want2 != want
        assert api.FrameError.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict() == want2
        assert np.array_equal(tiles.cpu().numpy().view(np.uint32), want_tiles2)
        t.a.denoise_pair(t.b)                                 # the null stream
        assert t.a.compare_filtered(t.b) == want


def test_the_packed_planes_are_what_the_pack_kernel_of_each_contexts_mode_makes_of_them():
    """The words beside the planes come from the library's toInt -- parity's for a parity context, fast mode's for a fast one: writing the
    filtered planes into two contexts of those modes and comparing their packed frames gives the same sums."""
    w, h = 41, 23
    _, A, B = planes(w, h)
    with Halves(w, h, extra=2) as t:
        c, d = t.all[2:]
        for modes in ((api.RT_MODE_PARITY, api.RT_MODE_PARITY), (api.RT_MODE_FAST, api.RT_MODE_PARITY), (api.RT_MODE_FAST, api.RT_MODE_FAST)):
            for ctx, other, mode in ((t.a, c, modes[0]), (t.b, d, modes[1])):
                ctx.set_mode(mode)
                other.set_mode(mode)
            t.write(A, B)
            t.a.denoise_pair(t.b)
            c.write_state(t.a.read_filtered(), None, N)
            d.write_state(t.b.read_filtered(), None, N)
            got, got_tiles = t.a.compare_filtered(t.b, tiles=True)
            want, want_tiles = c.compare(d, tiles=True)
            assert got == want and np.array_equal(got_tiles, want_tiles), modes


# ---- 2. staleness ------------------------------------------------------------------------------------------------------
def test_whatever_moves_the_colour_plane_ends_the_plane_and_a_fresh_pair_call_brings_it_back():
    w, h = 41, 23
    D, A, B = planes(w, h)
    with Halves(w, h, extra=2) as t:
        a, b, c, d = t.all
        c.write_state(A, None, N)
        d.write_state(B, None, N)
        want = [bits(x) for x in api.denoise_pair_planes(A, B, w, h)]
        stale(a, b)                                           # never made

        def fresh():
            t.write(A, B)
            stale(a, b)                                       # (rt_write_state moved it)
            a.denoise_pair(b)
            assert np.array_equal(bits(a.read_filtered()), want[0]) and np.array_equal(bits(b.read_filtered()), want[1])
            return a.compare_filtered(b)

        err = fresh()
        movers = {
            "rt_render_async": lambda: a.render_async(1, a.stream),
            "rt_reset_async": lambda: a.reset_async(a.stream),
            "rt_reset": lambda: a.reset(),
            "rt_seed_stream_async": lambda: a.seed_stream(7, a.stream),
            "rt_write_state": lambda: a.write_state(A, None, N),
            "rt_merge_async into a": lambda: a.merge([c], a.stream),
        }
        for name, move in movers.items():
            move()
            stale(a, b)
            assert np.array_equal(bits(b.read_filtered()), want[1]), name      # b's plane has not moved: it can be read, not compared with a's
            assert fresh() == err, name
        # rt_denoise_async into a: a holds 2N passes as the merge of c and d would, and a current plane made with b at 2N passes
        a.write_state(D, None, 2 * N)
        b.write_state(B, None, 2 * N)
        a.denoise_pair(b)
        made = bits(b.read_filtered()).copy()
        assert a.compare_filtered(b)["pixels"] == w * h
        a.denoise(c, d)
        stale(a, b)
        assert np.array_equal(bits(b.read_filtered()), made)
        assert fresh() == err
        # the two planes must come from ONE call: a and c filtered together leave b's plane current and no partner of a's
        a.denoise_pair(c)
        _refused(a, RT_ERR_STATE, a.compare_filtered, b)
        assert np.array_equal(bits(b.read_filtered()), want[1])
        assert a.compare_filtered(c)["pixels"] == w * h
        # a merge that only READS a context leaves its plane
        a.denoise_pair(b)
        d.merge([a], d.stream)
        assert a.compare_filtered(b) == err


# ---- 3. refusals change nothing ----------------------------------------------------------------------------------------
def test_every_refusal_leaves_both_contexts_as_they_were():
    w, h = 41, 23
    _, A, B = planes(w, h)
    with Halves(w, h) as t, make("demo", 40, 23) as other_size, make("demo", w, h, rank=1, nranks=2) as shard, \
            make("demo", w, h, devices=[0, 0]) as multi:
        t.write(A, B)
        other_size.write_state(np.zeros(3 * 40 * 23, np.float32), None, N)
        a, b = t.a, t.b
        a.denoise_pair(b)
        planes_before = bits(a.read_filtered()).copy(), bits(b.read_filtered()).copy()
        err = a.compare_filtered(b)
        snaps = [snapshot(c) for c in (a, b)]

        def refused(code, *args):
            text = _refused(a, code, *args)
            for c, s in zip((a, b), snaps):
                assert_unchanged(c, s)
            return text

        lib = api.load_library()
        for pair in ((None, b._h), (a._h, None)):
            assert lib.rt_denoise_pair_async(*pair, None, None) == RT_ERR_ARG and b"null" in lib.rt_last_error()
        refused(RT_ERR_ARG, a.denoise_pair, a)
        refused(RT_ERR_ARG, a.denoise_pair, other_size)
        refused(RT_ERR_ARG, other_size.denoise_pair, b)
        for x in (shard, multi):
            refused(RT_ERR_ARG, a.denoise_pair, x)
            refused(RT_ERR_ARG, x.denoise_pair, b)
            refused(RT_ERR_ARG, a.compare_filtered, x)
            refused(RT_ERR_ARG, x.compare_filtered, b)
            refused(RT_ERR_ARG, x.read_filtered)
            refused(RT_ERR_ARG, a.render_converged_filtered, x, 30.0, 1, 8)
            refused(RT_ERR_ARG, x.render_adaptive_filtered, b, 30.0, 1, 1, 8)
        refused(RT_ERR_ARG, a.compare_filtered, a)
        refused(RT_ERR_ARG, a.compare_filtered, other_size)
        refused(RT_ERR_ARG, a.compare_filtered_async, b, 0)   # no place for the result
        nan, inf = float("nan"), float("inf")
        for bad in ({"search_radius": -1}, {"search_radius": 9}, {"patch_radius": -1}, {"patch_radius": 3}, {"alpha": -0.25}, {"alpha": nan},
                    {"alpha": inf}, {"k": 0.0}, {"k": -1.0}, {"k": nan}, {"k": inf}):
            assert list(bad)[0] in refused(RT_ERR_ARG, a.denoise_pair, b, bad)
            assert list(bad)[0] in refused(RT_ERR_ARG, a.render_converged_filtered, b, 30.0, 1, 8, bad)
            assert list(bad)[0] in refused(RT_ERR_ARG, a.render_adaptive_filtered, b, 30.0, 1, 1, 8, bad)
        # the loops' own refusals are those of rt_render_converged and rt_render_adaptive
        refused(RT_ERR_ARG, a.render_converged_filtered, b, 30.0, 0, 8)
        refused(RT_ERR_ARG, a.render_converged_filtered, b, 30.0, 1, N - 1)
        refused(RT_ERR_ARG, a.render_converged_filtered, b, math.nan, 1, 8)
        refused(RT_ERR_ARG, a.render_adaptive_filtered, b, 30.0, -1, 1, 8)
        # ... and every one of them left the planes current
        assert np.array_equal(bits(a.read_filtered()), planes_before[0]) and np.array_equal(bits(b.read_filtered()), planes_before[1])
        assert a.compare_filtered(b) == err
        # RT_ERR_STATE: the pass numbers
        b.write_state(B, None, N + 1)
        snaps[1] = snapshot(b)
        refused(RT_ERR_STATE, a.denoise_pair, b)              # the halves differ
        refused(RT_ERR_STATE, a.render_converged_filtered, b, 30.0, 1, 8)
        a.write_state(None, None, 0)
        b.write_state(None, None, 0)
        snaps = [snapshot(c) for c in (a, b)]
        refused(RT_ERR_STATE, a.denoise_pair, b)              # nobody holds a pass
        assert "default" in refused(RT_ERR_STATE, a.render_converged_filtered, b, 30.0, 1, 8)
        # ... and the call still works afterwards
        t.write(A, B)
        a.denoise_pair(b)
        assert np.array_equal(bits(a.read_filtered()), planes_before[0]) and a.compare_filtered(b) == err


# ---- 4. rendered frames: the two loops ---------------------------------------------------------------------------------
def two_streams(w, h):
    a, b = make("demo", w, h), make("demo", w, h)
    a.seed_stream(1, a.stream)
    b.seed_stream(2, b.stream)
    return a, b


def test_render_converged_filtered_stops_at_4_passes_where_render_converged_renders_all_64():
    """Demo at 96x64, a 27 dB target, 4 passes per check, at most 64.  By the oracle's frames the cross-filtered pair stands at 28.00 dB after the
    first check; the raw pair reaches 26.41 dB at 64 passes and never 27."""
    w, h = 96, 64
    A, B = demo_halves(4)
    want = metric_of(*api.denoise_pair_planes(A, B, w, h), w, h)[0]
    assert api.error_psnr(want) >= 27.0
    a, b = two_streams(w, h)
    with a, b:
        reached, last, checks = a.render_converged_filtered(b, 27.0, 4, 64)
        print("\n[filtered error] Demo 96x64: cross-filtered pair %.2f dB after %d passes per half" % (api.error_psnr(last), a.current_sample))
        assert (reached, checks) == (True, 1) and a.current_sample == b.current_sample == 4
        assert last == want                                   # field for field: parity mode is bit-exact and so is the filter
        assert np.array_equal(bits(a.read_colors()), bits(A)) and np.array_equal(bits(b.read_colors()), bits(B))
        assert a.compare_filtered(b) == want                  # the planes of the last check are current
        # no pass left to render: one check of the frames as they are; with other parameters, another figure
        assert a.render_converged_filtered(b, 27.0, 4, 4) == (True, want, 1)
        other = {"search_radius": 1, "patch_radius": 0}
        assert a.render_converged_filtered(b, math.inf, 4, 4, other) == (False, metric_of(*api.denoise_pair_planes(A, B, w, h, other), w, h)[0], 1)
        assert a.current_sample == b.current_sample == 4
    a, b = two_streams(w, h)
    with a, b:
        reached, last, checks = a.render_converged(b, 27.0, 4, 64)
        print("[filtered error] Demo 96x64: raw pair %.2f dB after %d passes per half" % (api.error_psnr(last), a.current_sample))
        assert (reached, checks) == (False, 16) and a.current_sample == b.current_sample == 64


def test_render_adaptive_filtered_selects_from_the_cross_filtered_map_on_both_contexts():
    """Demo at 96x64, 28 dB per tile, at least 4 passes, 4 per check, at most 8: the first check is at 4 passes, and what it selects is what the
    host planes' tile map selects -- 12 of the 24 groups by the oracle's frames; those hold 8 passes afterwards, the others 4."""
    w, h, db = 96, 64, 28.0
    A, B = demo_halves(4)
    _, tile_map = metric_of(*api.denoise_pair_planes(A, B, w, h), w, h)
    ty, tx, gx = T.shape(w, h)
    mask, counts = T.select_restated(w, h, np.full((ty, tx), 4), 4, tile_map, T.threshold(db))
    assert 0 < counts[0] < ty * gx                            # the test's own precondition: a partial selection
    want_passes = T.advance_restated(np.full((ty, tx), 4), mask, 4, w, h)
    a, b = two_streams(w, h)
    with a, b, make("demo", w, h) as dst:
        reached, last, checks = a.render_adaptive_filtered(b, db, 4, 4, 8)
        assert checks == 2 and a.current_sample == b.current_sample == 8
        pa, pb = a.tile_passes(), b.tile_passes()
        assert np.array_equal(pa, pb)                         # word for word
        assert pa.min() >= 4                                  # no tile below min_passes
        assert np.array_equal(pa, want_passes)                # the first check's selection: these groups, and so these counts
        assert int((pa == 8).sum()) == counts[1]
        assert last["pixels"] == w * h and reached in (True, False)
        assert a.compare_filtered(b) == last                  # the last check's planes are current: nothing rendered after it
        # the caller goes on: a per-tile merge, and the filter with the same parameters
        dst.merge([a, b], dst.stream)
        assert dst.current_sample == 16 and np.array_equal(dst.tile_passes(), 2 * pa)
        Ac, Bc, D = a.read_colors(), b.read_colors(), dst.read_colors()
        dst.denoise(a, b)
        assert_same_bits(dst.read_colors(), api.denoise_planes(D, Ac, Bc, w, h))
        _refused(a, RT_ERR_STATE, a.render_adaptive_filtered, b, db, 4, 4, 16)      # ragged on entry, as rt_render_adaptive
