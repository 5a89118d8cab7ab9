"""Adaptive sampling on the device (include/rt_api.h "adaptive sampling", csrc/rt_tiles.hip) against the CPU oracle.  The oracle for
everything here: pixels are independent, so a tile that has received p passes holds the colours, seeds and packed pixels of a uniform
p-pass render, bit for bit, whatever happened to the other tiles.  Selection, tile list, per-tile merge and the driver are compared with
the numpy restatement of tests/test_tiles_cpu.py; every comparison is of bits or of exact integers."""
import ctypes as C

import numpy as np
import pytest

from raytracing_simple_amd import api, host, scenes
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE, _refused, assert_counters, assert_unchanged, bits, make, merge_restated, oracle, snapshot
import test_tiles_cpu as T

pytestmark = pytest.mark.gpu

W, H = 41, 23            # 6 x 3 tiles, 2 x 3 groups; the right group holds two tiles, one of them 1 pixel wide; the top row is 7 pixels high


def dev_map(tile_map):
    """A tile map as a device array (keep it alive while the library reads it)."""
    return api.DeviceWords(tile_map)


def select(ctx, mask, mark_also=None):
    """rt_select_tiles with above = 0 from a hand-made map: 1 in ONE tile (the last) of every group of `mask` -- and of `mark_also`, groups
    the front rule must leave out.  Returns the counts."""
    w, h = ctx.w, ctx.h
    ty, tx, gx = T.shape(w, h)
    marked = np.asarray(mask, bool) | (np.zeros((ty, gx), bool) if mark_also is None else np.asarray(mark_also, bool))
    err = np.zeros((ty, tx), np.uint32)
    for y, g in zip(*np.nonzero(marked)):
        err[y, min(4 * g + 3, tx - 1)] = 1
    d = dev_map(err)
    return ctx.select_tiles(d.ptr, 0, ctx.stream)


def per_pixel(tile_passes, w, h):
    return np.repeat(np.repeat(np.asarray(tile_passes, np.int64), 8, axis=0), 8, axis=1)[:h, :w]       # row 0 = bottom, as the pixel buffer


def assert_tiles(ctx, tile_passes, ref_at):
    """tile_passes() equals the map, and for every distinct count p the colours, seeds and packed pixels of the tiles at p are those of
    ref_at(p) -- a dict with "colors", "seeds", "pixels" of a uniform p-pass render."""
    w, h = ctx.w, ctx.h
    assert np.array_equal(ctx.tile_passes(), np.asarray(tile_passes, np.uint32))
    pp = per_pixel(tile_passes, w, h)
    col = bits(ctx.read_colors()).reshape(h, w, 3)[::-1]
    seeds, px = ctx.read_seeds().reshape(h, w, 2), ctx.read_pixels().reshape(h, w)
    for p in np.unique(pp):
        m, want = pp == p, ref_at(int(p))
        assert np.array_equal(col[m], bits(want["colors"]).reshape(h, w, 3)[::-1][m]), p
        assert np.array_equal(seeds[m], np.asarray(want["seeds"]).reshape(h, w, 2)[m]), p
        assert np.array_equal(px[m], np.asarray(want["pixels"]).reshape(h, w)[m]), p
    return pp


# the sequence of tests 1 and 2: 2 full passes, then three subset launches over shrinking selections.  S1 holds both kinds of partial-edge
# group (the right column, the top row); every later map also marks the groups that have fallen behind, which the device must leave out
S1 = np.array([[0, 1], [1, 0], [1, 1]], bool)
S2 = np.array([[0, 0], [1, 0], [0, 1]], bool)
S3 = np.array([[0, 0], [0, 0], [0, 1]], bool)               # one group, partial at both edges: 9 x 7 pixels
EVERY = np.ones((3, 2), bool)


def ragged_sequence(ctx):
    """Returns the restated tile pass map; the launches: 1 full + 3 subset."""
    ctx.render_async(2, ctx.stream)
    full_kernel = ctx.last_kernel
    passes = np.full((3, 6), 2, np.uint32)
    for mask, also, n, counts in ((S1, None, 1, (4, 12)), (S2, ~S1, 3, (2, 6)), (S3, ~S2, 1, (1, 2))):
        want_mask, want_counts = T.select_restated(W, H, passes, ctx.current_sample, T.tiles_of(mask | (also if also is not None else mask), W, H), 0)
        assert np.array_equal(want_mask, mask) and want_counts == counts           # (the restatement, on the marked map, keeps the front only)
        assert select(ctx, mask, also) == counts
        ctx.render_tiles_async(n, ctx.stream)
        passes = T.advance_restated(passes, mask, n, W, H)
    assert ctx.current_sample == 7 and ctx.last_kernel == full_kernel     # the form the context's last launch used
    return passes


# ---- 1. ragged equals uniform per tile ----------------------------------------------------------------------------
# Which instance renders: the Demo scene's first launches belong to the cooperative-or-plain measurement (either one-wavefront instance);
# with the diagnostics library's threshold at 0 it is the plain one for certain.  16 spheres get the cooperative one-wavefront instance;
# the diagnostics library's workgroup knob makes it the four-wavefront one.
def _knob(name, value):
    def apply(ctx):
        ctx._check(getattr(ctx._lib, name)(ctx._h, value))
    return apply


@pytest.mark.parametrize("name,kw,knob,kernels,pixel_write", [
    ("demo", {}, None, ("rt_trace_parity_w1", "rt_trace_parity_coop_w1"), 1),
    ("demo", {"diag": True}, _knob("rt_debug_set_coop_min", 0), ("rt_trace_parity_w1",), 1),
    ("coop16", {}, None, ("rt_trace_parity_coop_w1",), 1),
    ("coop16", {"diag": True}, _knob("rt_debug_set_wg_waves", 4), ("rt_trace_parity_coop",), 1),
    ("demo", {}, None, ("rt_trace_parity_w1", "rt_trace_parity_coop_w1"), 0)],
    ids=["demo", "demo-plain-one-wavefront", "16-spheres-one-wavefront", "16-spheres-four-wavefronts", "demo-pixel-store-off"])
def test_a_tile_at_p_passes_holds_the_uniform_p_pass_render(name, kw, knob, kernels, pixel_write):
    with make(name, **kw) as ctx:
        if knob:
            knob(ctx)
        ctx.set_pixel_write(pixel_write)
        passes = ragged_sequence(ctx)
        assert passes.tolist() == [[2, 2, 2, 2, 3, 3], [6, 6, 6, 6, 2, 2], [3, 3, 3, 3, 7, 7]]
        assert ctx.last_kernel in kernels
        pp = assert_tiles(ctx, passes, lambda p: oracle(name, W, H, p))
        st = ctx.stats()
        assert st["samples"] == int(pp.sum()) == int((T.tile_pixels(W, H) * passes).sum())
        assert st["launches"] == 4


# ---- 2. the hierarchy instance ------------------------------------------------------------------------------------
def test_the_hierarchy_instance_renders_subsets_too():
    sph, orig, target = scenes.random_spheres(66)            # 64 small spheres: a hierarchy
    cam = host.compute_camera(orig, target, W, H)

    def forced():
        ctx = api.RtContext(W, H, diag=True)
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        return ctx

    with forced() as plain, forced() as ctx:
        ref = {}
        for p in (2, 3, 6, 7):                                # progressive launches equal one launch bit for bit (tests/test_gpu_parity.py)
            px = plain.render_pass(p - plain.current_sample)
            ref[p] = {"colors": plain.read_colors(), "seeds": plain.read_seeds(), "pixels": px}
        assert plain.last_kernel == "rt_trace_parity_pairs"
        passes = ragged_sequence(ctx)
        assert ctx.last_kernel == "rt_trace_parity_pairs"
        pp = assert_tiles(ctx, passes, ref.__getitem__)
        assert ctx.stats()["samples"] == int(pp.sum()) and ctx.stats()["launches"] == 4


# ---- 3. the front rule ----------------------------------------------------------------------------------------------
def test_a_group_that_fell_behind_stays_retired():
    with make("demo") as ctx:
        ctx.render_async(2, ctx.stream)
        # every group selected on a whole context: it stays whole, and full launches go on
        assert ctx.select_tiles(None, 0, ctx.stream) == (6, 18)
        ctx.render_tiles_async(1, ctx.stream)
        assert ctx.current_sample == 3 and np.all(ctx.tile_passes() == 3)
        ctx.render_async(1, ctx.stream)
        assert ctx.current_sample == 4 and ctx.stats()["launches"] == 3
        want = oracle("demo", W, H, 4)
        assert_tiles(ctx, np.full((3, 6), 4), lambda p: want)
        assert_counters(ctx, want)
        # one group is left out and falls behind
        keep = EVERY.copy()
        keep[1, 1] = False
        assert select(ctx, keep) == (5, 16)
        ctx.render_tiles_async(2, ctx.stream)
        passes = T.advance_restated(np.full((3, 6), 4), keep, 2, W, H)
        snap = snapshot(ctx)
        # selected again on its own: nothing
        only = ~keep
        assert select(ctx, only) == (0, 0)
        ctx.render_tiles_async(5, ctx.stream)                 # an empty selection: RT_OK, nothing done
        assert ctx.current_sample == 6 and ctx.stats()["launches"] == 4
        assert_unchanged(ctx, snap)
        # ... and with everything else, by a NULL map: the five at the front
        assert ctx.select_tiles(None, 0, ctx.stream) == (5, 16)
        ctx.render_tiles_async(1, ctx.stream)
        passes = T.advance_restated(passes, keep, 1, W, H)
        assert passes[1].tolist() == [7, 7, 7, 7, 4, 4]
        assert_tiles(ctx, passes, lambda p: oracle("demo", W, H, p))       # the retired group: floats, seeds, pixels and count of pass 4
        assert ctx.render_tiles_async(0, ctx.stream) is None and ctx.current_sample == 7


# ---- 4. more than one chunk, order kept -------------------------------------------------------------------------------
def test_a_list_longer_than_a_chunk_follows_the_heavy_first_order():
    w, h = 528, 136                                          # 66 x 17 = 1122 one-wavefront tiles: two chunks of the list kernel
    ty, tx, gx = T.shape(w, h)
    mask = (np.add.outer(np.arange(ty), np.arange(gx)) % 2) == 0       # a checkerboard of groups
    with make("demo", w, h, diag=True) as ctx, make("demo", w, h, diag=True) as plain:
        lib = ctx._lib
        for x in (ctx, plain):
            x._check(lib.rt_debug_set_coop_min(x._h, 0))     # no cooperative-or-plain measurement: the plain one-wavefront instance

        def schedule():
            order, cost = np.zeros(tx * ty, np.uint32), np.zeros(tx * ty, np.uint32)
            n, valid = C.c_uint32(), C.c_int()
            ctx._check(lib.rt_debug_read_tile_order(ctx._h, order.ctypes.data, cost.ctypes.data, order.size, C.byref(n), C.byref(valid)))
            return order[:n.value], cost[:n.value], valid.value

        ctx.render_pass(8)                                   # a long launch prices the tiles ...
        ctx.reset()
        ctx.render_pass(8)                                   # ... and the next one sorts them: a heavy-first order exists
        assert ctx.last_kernel == "rt_trace_parity_w1"
        order, cost, valid = schedule()
        assert valid == 1 and order.size == tx * ty and sorted(order.tolist()) == list(range(tx * ty))
        choice = ctx.scene_choice()
        counts = select(ctx, mask)
        assert counts == T.select_restated(w, h, np.full((ty, tx), 8), 8, T.tiles_of(mask, w, h), 0)[1]
        ctx.render_tiles_async(2, ctx.stream)
        assert ctx.current_sample == 10 and ctx.last_kernel == "rt_trace_parity_w1"
        # the list the launch walked: the restated stable filter of the order, padded with the sentinel to whole grid rows
        want_list, grid = T.list_restated(w, h, 1, mask, order.tolist())
        got = np.zeros(tx * (ty + 1), np.uint32)
        slots, n_launch, by_order = C.c_uint32(), C.c_uint32(), C.c_int()
        ctx._check(lib.rt_debug_read_tile_list(ctx._h, got.ctypes.data, got.size, C.byref(slots), C.byref(n_launch), C.byref(by_order)))
        assert (slots.value, n_launch.value, by_order.value) == (grid[0] * grid[1], tx * ty, 1)
        assert np.array_equal(got[:slots.value], want_list)
        # schedule and verdicts are what they were
        order2, cost2, valid2 = schedule()
        assert valid2 == 1 and np.array_equal(order2, order) and np.array_equal(cost2, cost) and ctx.scene_choice() == choice
        # selected tiles: a plain context at 10 passes; the others: at 8
        ref = {}
        for p in (8, 10):
            px = plain.render_pass(p - plain.current_sample)
            ref[p] = {"colors": plain.read_colors(), "seeds": plain.read_seeds(), "pixels": px}
        pp = assert_tiles(ctx, T.advance_restated(np.full((ty, tx), 8), mask, 2, w, h), ref.__getitem__)
        assert ctx.stats()["samples"] == int(pp.sum())


# ---- 5. merge per tile --------------------------------------------------------------------------------------------------
def test_merge_weights_every_tile_by_its_own_count():
    with make("demo") as a, make("demo") as b, make("demo") as c:
        for k, ctx in enumerate((a, b, c)):
            ctx.seed_stream(k + 1, ctx.stream)
        # a: 2 passes everywhere, 5 in S1;  b: 3 everywhere, 4 in S2;  c: an old frame, then reset_async and 2 passes in S3 only -- 0 elsewhere
        a.render_async(2, a.stream)
        assert select(a, S1) == (4, 12)
        a.render_tiles_async(3, a.stream)
        b.render_async(3, b.stream)
        assert select(b, S2) == (2, 6)
        b.render_tiles_async(1, b.stream)
        c.render_async(2, c.stream)
        c.reset_async(c.stream)
        c.seed_stream(3, c.stream)
        assert select(c, S3) == (1, 2)
        c.render_tiles_async(2, c.stream)
        maps = [T.advance_restated(np.full((3, 6), 2), S1, 3, W, H), T.advance_restated(np.full((3, 6), 3), S2, 1, W, H),
                T.advance_restated(np.zeros((3, 6)), S3, 2, W, H)]
        for ctx, m in zip((a, b, c), maps):
            assert np.array_equal(ctx.tile_passes(), m)
        assert_tiles(c, maps[2], lambda p: oracle("demo", W, H, 2, 3) if p else
                     {"colors": c.read_colors(), "seeds": host_stream(3), "pixels": c.read_pixels()})      # the tiles at 0 passes hold the stream's first seeds
        planes = [x.read_colors() for x in (a, b, c)]
        seeds_a = a.read_seeds()
        a.merge([b, c], a.stream)
        want, counts = T.merge_tiles_restated(planes, maps, W, H)
        assert a.current_sample == 5 + 4 + 2
        assert np.array_equal(bits(a.read_colors()), bits(want))
        assert np.array_equal(a.tile_passes(), counts) and counts.tolist() == [[5, 5, 5, 5, 8, 8], [9, 9, 9, 9, 5, 5], [8, 8, 8, 8, 11, 11]]
        assert np.array_equal(a.read_seeds(), seeds_a)        # dst's seeds stay; the sources are only read
        for ctx, m, p in zip((b, c), maps[1:], planes[1:]):
            assert np.array_equal(ctx.tile_passes(), m) and np.array_equal(bits(ctx.read_colors()), bits(p))
        _refused(a, RT_ERR_STATE, a.render_async, 1, a.stream)         # the merged context is ragged
    # whole contexts only: the old kernel, the old bits
    with make("demo") as a, make("demo") as b, make("demo") as c:
        for k, (ctx, n) in enumerate(zip((a, b, c), (3, 5, 2))):
            ctx.seed_stream(k + 1, ctx.stream)
            ctx.render_async(n, ctx.stream)
        a.merge([b, c], a.stream)
        want = merge_restated([oracle("demo", W, H, n, k + 1)["colors"] for k, n in enumerate((3, 5, 2))], (3, 5, 2))
        assert np.array_equal(bits(a.read_colors()), bits(want)) and np.all(a.tile_passes() == 10)
        a.render_async(1, a.stream)                           # ... and it is whole
        assert a.current_sample == 11


def host_stream(stream_id):
    return api.stream_seeds(stream_id, 2 * W * H)


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------
# 64 x 48, Demo, streams 1 and 2, min_passes 4, 4 passes per check, at most 24.  The figures were chosen on the CPU from the oracle's frames
# alone (test_tiles_cpu.adaptive_restated): at 14 dB five of the twelve groups retire at the first check, ten before pass 24, and the last
# one passes its check AT pass 24 -- six checks, return value 1.  At 18 dB four groups are still above the target at pass 24: return value 0.
DRIVER = {
    14.0: (True, 6, [[8] * 8, [12] * 4 + [8] * 4, [16] * 4 + [24] * 4, [4] * 4 + [8] * 4, [4] * 8, [4] * 8]),
    18.0: (False, 6, [[12] * 4 + [16] * 4, [24] * 8, [24] * 8, [12] * 8, [4] * 4 + [8] * 4, [4] * 8]),
}


@pytest.mark.parametrize("tile_db", sorted(DRIVER))
def test_the_driver_retires_the_tiles_the_reference_retires(tile_db):
    w, h = 64, 48
    reached, checks, passes, cur = T.adaptive_restated(lambda p: oracle("demo", w, h, p, 1)["pixels"], lambda p: oracle("demo", w, h, p, 2)["pixels"],
                                                       w, h, tile_db, 4, 4, 24)
    assert (reached, checks, passes.tolist()) == DRIVER[tile_db] and cur == 24         # the reference alone deciding
    retired_early = int((passes[:, ::4] < 24).sum())
    assert retired_early >= 3 and int((passes[:, ::4] == 4).sum()) < 12                 # a quarter of the groups and more; not all at the first check
    with make("demo", w, h) as a, make("demo", w, h) as b:
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
        got_reached, last, got_checks = a.render_adaptive(b, tile_db, 4, 4, 24)
        assert (got_reached, got_checks) == (reached, checks)
        assert a.current_sample == b.current_sample == 24
        assert np.array_equal(a.tile_passes(), passes) and np.array_equal(b.tile_passes(), passes)
        assert_tiles(a, passes, lambda p: oracle("demo", w, h, p, 1))
        assert_tiles(b, passes, lambda p: oracle("demo", w, h, p, 2))
        frames = [T.compose(lambda p, s=s: oracle("demo", w, h, p, s)["pixels"], passes, w, h) for s in (1, 2)]
        assert last == T.frame_error_restated(frames[0], frames[1], w, h)[0]           # *last: the last whole-frame comparison
        # merged afterwards, exact per tile
        planes = [a.read_colors(), b.read_colors()]
        a.merge([b], a.stream)
        want, counts = T.merge_tiles_restated(planes, [passes, passes], w, h)
        assert np.array_equal(bits(a.read_colors()), bits(want)) and np.array_equal(a.tile_passes(), counts)


# ---- 7. refusals change nothing ------------------------------------------------------------------------------------------
def test_refusals_change_nothing(tmp_path):
    with make("demo") as ctx, make("demo") as other, make("demo", rank=1, nranks=2) as shard, make("demo", devices=[0, 0]) as multi:
        lib = api.load_library()
        other.seed_stream(2, other.stream)
        ctx.seed_stream(1, ctx.stream)
        ctx.render_async(2, ctx.stream)
        other.render_async(2, other.stream)
        snap = snapshot(ctx)
        assert "selection" in _refused(ctx, RT_ERR_STATE, ctx.render_tiles_async, 1, ctx.stream)       # nothing selected yet
        _refused(ctx, RT_ERR_ARG, ctx.render_adaptive, other, 30.0, -1, 4, 8)                          # min_passes < 0
        assert_unchanged(ctx, snap)
        assert select(ctx, S1) == (4, 12)
        _refused(ctx, RT_ERR_ARG, ctx.render_tiles_async, -1, ctx.stream)
        ctx.render_tiles_async(1, ctx.stream)
        other.render_async(1, other.stream)                   # (both at pass 3: what is refused below is the ragged context)
        snap, snap_other, passes = snapshot(ctx), snapshot(other), ctx.tile_passes()
        _refused(ctx, RT_ERR_STATE, ctx.render_pass, 1)
        _refused(ctx, RT_ERR_STATE, ctx.render_async, 1, ctx.stream)
        _refused(ctx, RT_ERR_STATE, ctx.render_converged, other, 30.0, 1, 8)
        _refused(ctx, RT_ERR_STATE, ctx.render_adaptive, other, 30.0, 0, 1, 8)
        _refused(ctx, RT_ERR_STATE, ctx.save_state, tmp_path / "ragged.bin")
        assert not (tmp_path / "ragged.bin").exists()
        assert_unchanged(ctx, snap)
        assert np.array_equal(ctx.tile_passes(), passes) and ctx.stats()["launches"] == 2
        assert_unchanged(other, snap_other)
        # sharded and multi-device contexts: out of scope for every new call
        for x in (shard, multi):
            buf, counts = np.zeros(64, np.uint32), (C.c_uint32 * 2)()
            assert lib.rt_tile_passes(x._h, buf.ctypes.data) == RT_ERR_ARG
            assert lib.rt_select_tiles(x._h, None, 0, None, counts) == RT_ERR_ARG
            assert lib.rt_render_tiles_async(x._h, 1, None) == RT_ERR_ARG
        with make("demo", rank=0, nranks=2) as shard0:
            shard0.seed_stream(3)
            _refused(shard, RT_ERR_ARG, shard.render_adaptive, shard0, 30.0, 1, 1, 4)
        # rt_reset makes the context whole again
        ctx.reset()
        assert np.all(ctx.tile_passes() == 0)
        _refused(ctx, RT_ERR_STATE, ctx.render_tiles_async, 1, ctx.stream)                             # the selection went with the reset
        px = ctx.render_pass(3)
        want = oracle("demo", W, H, 3)
        assert np.array_equal(px, want["pixels"])
        assert_tiles(ctx, np.full((3, 6), 3), lambda p: want)
        assert_counters(ctx, want)
