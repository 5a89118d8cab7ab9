"""The two small kernels of adaptive sampling at their own edges (csrc/rt_tiles.hip): rt_select_tiles_kernel with a threshold -- edge tiles, error
words that need the 64-bit product, more than one workgroup, a ragged context -- and rt_tile_list_kernel in image order over more than one chunk
and for the four-wavefront shape.  Everything is compared with the numpy restatement of tests/test_tiles_cpu.py; all figures are exact integers.
Which groups a selection flagged is read off the device by rendering one pass on them: rt_tile_passes shows who moved."""
import ctypes as C

import numpy as np
import pytest

import test_tiles_cpu as T
from raytracing_simple_amd import api
from test_gpu_state import make
from test_gpu_tiles import assert_tiles, select

pytestmark = pytest.mark.gpu

W, H = 41, 23
TOP = 2 ** 32 - 1


def flags_after(ctx, base):
    """One pass on the selection: the groups whose tiles moved from `base` (an int, or the tile map before).  Returns bool [tiles_y, groups_x]."""
    ctx.render_tiles_async(1, ctx.stream)
    moved = ctx.tile_passes().astype(np.int64) - base
    assert np.isin(moved, (0, 1)).all()
    return moved[:, ::4] == 1                                # (a group's tiles hold one count: test_tiles_cpu.tiles_of is checked by the caller)


def read_list(ctx):
    ty, tx, _ = T.shape(ctx.w, ctx.h)
    got = np.zeros(tx * (ty + 1), np.uint32)
    slots, n_launch, by_order = C.c_uint32(), C.c_uint32(), C.c_int()
    ctx._check(ctx._lib.rt_debug_read_tile_list(ctx._h, got.ctypes.data, got.size, C.byref(slots), C.byref(n_launch), C.byref(by_order)))
    return got[:slots.value], n_launch.value, by_order.value


# ---- 1. selection with a threshold ------------------------------------------------------------------------------------------------
# One tile of each kind carries a word, each in a group of its own: a full tile (64 pixels), the right edge (1 x 8), the top edge (8 x 7), the
# corner (1 x 7).  The rule is err * 64 > above * pixels: words at floor(above * pixels / 64) + delta.
KINDS = {(0, 0): 64, (1, 5): 8, (2, 1): 56, (2, 5): 7}


def threshold_maps():
    maps = []
    for above in (1, 1000, TOP):
        for delta in (-1, 0, 1):
            err = np.zeros((3, 6), np.uint32)
            for (y, x), pixels in KINDS.items():
                err[y, x] = min(max(above * pixels // 64 + delta, 0), TOP)
            maps.append((above, err))
        maps.append((above, np.full((3, 6), TOP, np.uint32)))                    # 2^32 - 1 everywhere: err * 64 needs 38 bits
    big = np.zeros((3, 6), np.uint32)
    big[0, 0], big[1, 5], big[2, 1], big[2, 5] = 2 ** 26, 2 ** 26, 2 ** 31, 2 ** 30       # err * 64 is 0 modulo 2^32
    return maps + [(1000, big), (TOP, big)]


def test_selection_with_a_threshold_at_edge_tiles_and_with_words_that_need_64_bits():
    assert T.tile_pixels(W, H)[tuple(zip(*KINDS))].tolist() == list(KINDS.values())
    seen = set()
    with make("demo") as ctx:
        for above, err in threshold_maps():
            ctx.reset_async(ctx.stream)                       # whole at pass 0: every group at the front
            want, counts = T.select_restated(W, H, np.zeros((3, 6)), 0, err, above)
            seen.add(tuple(want.reshape(-1).tolist()))
            d = api.DeviceWords(err)
            assert ctx.select_tiles(d.ptr, above, ctx.stream) == counts, (above, err.tolist())
            assert np.array_equal(flags_after(ctx, 0), want), (above, err.tolist())
            assert np.array_equal(ctx.tile_passes() == 1, T.tiles_of(want, W, H))
            d.close()
    assert len(seen) >= 5                                     # (the maps do tell the kinds apart: nothing, everything, and mixtures)


# ---- 2. selection over more than one workgroup ------------------------------------------------------------------------------------
def test_selection_over_a_second_workgroup_and_on_a_ragged_context():
    w, h = 264, 232                                           # 33 x 29 tiles, 9 groups per row: 261 groups -- a second workgroup with 5 live lanes
    ty, tx, gx = T.shape(w, h)
    assert (ty, tx, gx) == (29, 33, 9) and ty * gx == 261
    rng = np.random.default_rng(11)
    mask = rng.random((ty, gx)) < 0.5
    mask[-1, -1] = True                                       # (the last group: one tile, the last live lane of the second workgroup)
    with make("demo", w, h) as ctx:
        ctx.render_async(1, ctx.stream)
        assert ctx.select_tiles(None, 0, ctx.stream) == (261, 957)
        assert select(ctx, np.ones((ty, gx), bool)) == (261, 957)
        want, counts = T.select_restated(w, h, np.full((ty, tx), 1), 1, T.tiles_of(mask, w, h), 0)
        assert np.array_equal(want, mask) and counts[0] == int(mask.sum())
        assert select(ctx, mask) == counts
        assert np.array_equal(flags_after(ctx, 1), mask)
        passes = T.advance_restated(np.full((ty, tx), 1), mask, 1, w, h)
        assert np.array_equal(ctx.tile_passes(), passes)
        # ragged: `passes` is read.  The map marks half of the front and every group that fell behind; those come back unselected
        second = mask & (rng.random((ty, gx)) < 0.5)
        want, counts = T.select_restated(w, h, passes, 2, T.tiles_of(second | ~mask, w, h), 0)
        assert np.array_equal(want, second) and 0 < counts[0] < int(mask.sum())
        assert select(ctx, second, ~mask) == counts
        assert np.array_equal(flags_after(ctx, passes.astype(np.int64)), second)
        assert ctx.select_tiles(None, 0, ctx.stream) == T.select_restated(w, h, T.advance_restated(passes, second, 1, w, h), 3, None, 0)[1]


# ---- 3. the list in image order, several chunks -----------------------------------------------------------------------------------
def test_a_list_in_image_order_carries_its_base_from_chunk_to_chunk():
    w, h = 528, 136                                           # 66 x 17 = 1122 one-wavefront tiles: two chunks of 1024 ids; id 1024 is tile 34 of row 15
    ty, tx, gx = T.shape(w, h)
    late = np.zeros((ty, gx), bool)
    late[15, 9:] = True                                       # (group 8 of row 15 holds the ids 1022 .. 1025: left out of both)
    late[16] = True
    early = ~late
    early[15, 8] = False
    checker = (np.add.outer(np.arange(ty), np.arange(gx)) % 2) == 0
    kept = [T.list_restated(w, h, 1, m)[0] for m in (late, early)]
    assert kept[0].min() >= 1024 and kept[1][kept[1] < tx * ty].max() < 1024      # nothing of the first chunk; nothing of the second
    with make("demo", w, h, diag=True) as ctx, make("demo", w, h, diag=True) as plain:
        lib = ctx._lib
        for x in (ctx, plain):
            x._check(lib.rt_debug_set_tile_order(x._h, 0))    # no schedule: the list kernel's `order` is null
            x._check(lib.rt_debug_set_coop_min(x._h, 0))      # the plain one-wavefront instance
        ref = {}
        for p in (1, 2):
            px = plain.render_pass(1)
            ref[p] = {"colors": plain.read_colors(), "seeds": plain.read_seeds(), "pixels": px}
        for mask in (late, early, checker):
            ctx.reset_async(ctx.stream)
            ctx.render_async(1, ctx.stream)
            assert select(ctx, mask) == (int(mask.sum()), int(T.tiles_of(mask, w, h).sum()))
            ctx.render_tiles_async(1, ctx.stream)
            assert ctx.last_kernel == "rt_trace_parity_w1"
            want, grid = T.list_restated(w, h, 1, mask)
            got, n_launch, by_order = read_list(ctx)
            assert (got.size, n_launch, by_order) == (grid[0] * grid[1], tx * ty, 0)
            assert np.array_equal(got, want)
            pp = assert_tiles(ctx, T.advance_restated(np.full((ty, tx), 1), mask, 1, w, h), ref.__getitem__)
            assert ctx.stats()["samples"] == int(pp.sum())


# ---- 4. the list for the four-wavefront shape -------------------------------------------------------------------------------------
def test_a_list_of_groups_for_the_four_wavefront_shape():
    w, h = 1056, 256                                          # 33 x 32 = 1056 launch tiles of 32 x 8: two chunks, per_group == 1
    ty, tx, gx = T.shape(w, h)
    assert (ty, gx) == (32, 33)
    mask = (np.add.outer(np.arange(ty), np.arange(gx)) % 2) == 0
    with make("coop16", w, h, diag=True) as ctx, make("coop16", w, h, diag=True) as plain:
        lib = ctx._lib
        for x in (ctx, plain):
            x._check(lib.rt_debug_set_wg_waves(x._h, 4))
        ref = {}
        for p in (1, 2):
            px = plain.render_pass(1)
            ref[p] = {"colors": plain.read_colors(), "seeds": plain.read_seeds(), "pixels": px}
        assert plain.last_kernel == "rt_trace_parity_coop"
        ctx.render_async(1, ctx.stream)
        assert select(ctx, mask) == (int(mask.sum()), int(T.tiles_of(mask, w, h).sum()))
        ctx.render_tiles_async(1, ctx.stream)
        assert ctx.last_kernel == "rt_trace_parity_coop"
        got, n_launch, by_order = read_list(ctx)
        order = None
        if by_order:
            order, cost, n, valid = np.zeros(ty * gx, np.uint32), np.zeros(ty * gx, np.uint32), C.c_uint32(), C.c_int()
            ctx._check(lib.rt_debug_read_tile_order(ctx._h, order.ctypes.data, cost.ctypes.data, order.size, C.byref(n), C.byref(valid)))
            assert valid.value == 1 and n.value == ty * gx
            order = order.tolist()
        want, grid = T.list_restated(w, h, 4, mask, order)
        assert (got.size, n_launch) == (grid[0] * grid[1], ty * gx)
        assert np.array_equal(got, want)
        pp = assert_tiles(ctx, T.advance_restated(np.full((ty, tx), 1), mask, 1, w, h), ref.__getitem__)
        assert ctx.stats()["samples"] == int(pp.sum())
