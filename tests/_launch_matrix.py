"""Launch path x kernel instance: the table, the scripts and the comparison of tests/test_gpu_launch_matrix.py (on the device) and
tests/test_launch_matrix_cpu.py (the preconditions, on the oracle alone).

THE INVARIANT.  Pixels are independent, a wavefront's arithmetic depends on its tile alone, and nothing crosses wavefronts but booleans
(any-hit answers, ballots).  So whatever way the host code puts an instance on a stream -- split launches, the pixel store switched off,
the heavy-first order with its cost writes, a subset launch padded with sentinel workgroups, an in-place reset, a seed stream, a state
written from the host, a row-tile shard -- every pixel that holds p passes holds the words of the SAME instance's straight p-pass render
(one launch on a fresh context): colour plane as bits, seeds, packed pixels, and the five work counters.  In parity mode those words are
the oracle's (asserted before a reference is handed out); in fast mode the straight render is the only reference there is -- other modules
hold it to binary64 -- and the equality asked for here is exact, with no tolerance.

ROWS.  The eight shipped names in both arithmetics, each BY NAME on the diagnostics library (set up as test_gpu_bvh._render(inst=...):
hierarchy forced, walk knobs set, rt_set_mode of the instance's row) over test_gpu_parity._glass_and_mirror_scene(); and the four instances
a scene alone reaches on the PRODUCT library, in both arithmetics, over the makers' own scenes.  Every context is a `Checked` one: after
every launch it asserts that rt_last_kernel names the row's instance.  41 x 23: ragged against the 8x8 and the 32x8 tile.

A WORKGROUP IN WHICH NO LANE IS VALID (the sentinel id tiles_x * tiles_y of a subset launch; read in csrc/rt_trace.inc.h and
csrc/rt_walk.inc.h before the first run on a device).  tile_by = tiles_y, so pixel_at() finds lrow >= local_rows in every lane:
own.valid is false and s_end = first_sample in all 64 * waves lanes.
  * The sweep (rt_trace.inc.h) has two workgroup barriers outside RT_OPT_STAMPS: behind the table staging and stage_k2, and behind the
    per-wavefront adds into s_stat.  Both stand outside the sample loop and outside every `if (own.valid)`: every thread reaches them.
    The staging in front of the first reads the scene's tables by thread number, never by tile.  The loop's first statement is
    `if (need_ray && s >= s_end) break` with need_ray true and s == s_end: every lane leaves before the first ballot.  The cooperative
    mailbox (s_coop, one slice per wavefront) is synchronised by wave barriers and wavefront-scope fences inside the shadow sweep only:
    a four-wavefront workgroup has no workgroup barrier inside the loop, so wavefronts that leave at different trips cannot wait for
    each other -- and here all four leave at once.
  * The walk (rt_walk.inc.h) stages header, pairs and slots as its table placement says (all three by thread number), then the same
    barrier; its loop ends on `ballot(!finished) == 0`, finished = (state kNew && s >= s_end), true in every lane at the first trip;
    the second barrier follows the epilogue as in the sweep.
  * The epilogue stores under `valid_e` (s_end != first_sample: false) only, adds zeros to the counters, and the cost store is behind
    `Q.tile_cost != null`, which launch_tiles never passes.  Nothing is loaded from or stored to the frame.
So a sentinel workgroup can neither hang nor write; what the scripts below can still find is a wrong word."""
import collections
import functools
import itertools

import numpy as np

import _oracle as O
from raytracing_simple_amd import api, host, scenes
from test_gpu_state import assert_state
from test_gpu_tiles import S1, S2, S3, assert_tiles, ragged_sequence, select     # (helpers only: importing them needs no device)
from test_state_cpu import restated_stream
import test_tiles_cpu as T

W, H = 41, 23                       # 6 x 3 tiles, 2 x 3 groups, a 7-pixel top row
SHIPPED = ("", "_w1", "_coop", "_coop_w1", "_pairs", "_pairs_m", "_pairs_g", "_g")
STREAM = 3                          # the seed stream of script 6
PASS_MAP = [[2, 2, 2, 2, 3, 3], [6, 6, 6, 6, 2, 2], [3, 3, 3, 3, 7, 7]]        # what test_gpu_tiles.ragged_sequence leaves

# The glass-and-mirror scene's own camera (the fixture's: (20, 100, 300) towards (0, 25, 0)) leaves the top seven pixel rows of a 41 x 23 frame
# all sky -- both groups of the top tile row, S3's among them, the one whose launch pads its list with sentinels: a tile left at the wrong
# pass count there would hold the right colours, exact zeros.  This camera looks down on the same records from nearer by and no group is all
# sky at any pass count (tests/test_launch_matrix_cpu.py holds that, and that glass and mirror still matter, on the oracle alone).
GLASS_CAMERA = ((20.0, 180.0, 120.0), (0.0, 10.0, 0.0))

Row = collections.namedtuple("Row", "kernel fast library scene")


def _rows():
    diag = [Row(("rt_trace_fast" if fast else "rt_trace_parity") + k, fast, "diagnostics", "glass") for fast in (False, True) for k in SHIPPED]
    # the instances a scene alone reaches on the product library (the table of tests/test_gpu_fast_shadow.py; the parity names are the counterparts)
    reach = (("_coop_w1", "demo_plus16"), ("_pairs", "random256"), ("_pairs_m", "many2000"), ("_pairs_g", "many5000"))
    return diag + [Row(("rt_trace_fast" if fast else "rt_trace_parity") + k, fast, "product", s) for fast in (False, True) for k, s in reach]


ROWS = _rows()
# A product row whose library changes instance in the middle of a script is a diagnostics-only row for that script: (row id, script) -> why.
# None so far: every launch stays below the 16 passes from which a call is split into probes, the surface-area estimate decides
# random_spheres(256) without a measurement, and from 1500 spheres in the tree the hierarchy is never measured against.
DIAGNOSTICS_ONLY = {}
# A fast row whose straight render is not a function of its inputs (the control of test_gpu_launch_matrix.py): row id -> the cause read from the code.
NOT_A_FUNCTION_OF_ITS_INPUTS = {}


def row_id(row):
    return "%s-%s" % (row.kernel, row.library)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(spheres, camera at 41 x 23) of a row's scene."""
    if name == "glass":
        from test_gpu_parity import _glass_and_mirror_scene
        sph, orig, target = _glass_and_mirror_scene()
        orig, target = GLASS_CAMERA
    elif name == "demo_plus16":
        sph, orig, target = scenes.demo_plus(16)
    elif name == "random256":
        sph, orig, target = scenes.random_spheres(256)
    else:
        from test_gpu_bvh import _many_spheres
        sph, orig, target = _many_spheres({"many2000": 2000, "many5000": 5000}[name])
    return sph, host.compute_camera(orig, target, W, H)


def frozen(frame):
    for v in frame.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return frame


def counters_of(stats):
    """The five work counters, from rt_get_stats' names or the oracle's."""
    return tuple(int(stats[a] if a in stats else stats[b]) for a, b in (("samples", "samples"), ("closest_rays", "closest_calls"), ("shadow_rays", "shadow_calls"),
                                                                        ("sphere_tests", "sphere_tests"), ("rng_draws", "rng_draws")))


@functools.lru_cache(maxsize=None)
def oracle_frame(scene_name, p, stream_id=0):
    """`p` straight passes of the oracle on seed stream `stream_id` (the restated stream, tests/test_state_cpu.py); computed once, read-only."""
    sph, cam = scene(scene_name)
    seeds = None if stream_id == 0 else restated_stream(stream_id, 2 * W * H)
    out = O.render(sph, cam, W, H, p, seeds_in=seeds, threads=16)
    return frozen({"colors": out["colors"], "seeds": out["seeds"], "pixels": out["pixels"], "counters": counters_of(out["stats"])})


# ---- the comparison: needs no device -------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def per_pixel(tile_passes):
    """A tile map spread over the pixels, [H, W] in the pixel buffer's orientation (row 0 = bottom)."""
    return np.repeat(np.repeat(np.asarray(tile_passes, np.int64), 8, axis=0), 8, axis=1)[:H, :W]


def group_pixels(mask):
    """The pixels of the groups of `mask` ([tiles_y, groups_x]), bool [H, W]."""
    return per_pixel(T.tiles_of(mask, W, H)).astype(bool)


def compare(got, want, where=None, parts=("colors", "seeds", "pixels", "counters"), what=""):
    """Every word of `got` equals `want`'s -- colour plane as BITS (a -0.0 is not a +0.0), seeds, packed pixels, on the pixels of `where` (bool
    [H, W], row 0 = bottom as the pixel and seed buffers have it; the colour plane is y-flipped, .cl:579; None: every pixel) -- and the five
    counters.  Frames are dicts of "colors" [3 W H], "seeds" [2 W H], "pixels" [W H], "counters" (5)."""
    m = np.ones((H, W), bool) if where is None else np.asarray(where, bool)
    for part, per, flip in (("colors", 3, True), ("seeds", 2, False), ("pixels", 1, False)):
        if part not in parts:
            continue
        g, w = (bits(x[part]).reshape(H, W, per) for x in (got, want))
        if flip:
            g, w = g[::-1], w[::-1]
        bad = (g != w).any(axis=2) & m
        assert not bad.any(), "%s: %d pixels differ in %s, the first at (row, x) = %s" % (what, int(bad.sum()), part, tuple(np.argwhere(bad)[0]))
    if "counters" in parts:
        assert tuple(got["counters"]) == tuple(want["counters"]), "%s: counters %s, expected %s" % (what, tuple(got["counters"]), tuple(want["counters"]))


def compare_at(got, tile_passes, ref_at, parts=("colors", "seeds", "pixels"), what=""):
    """... where every tile holds its own pass count: the pixels at p passes against ref_at(p)."""
    pp = per_pixel(tile_passes)
    for p in np.unique(pp):
        compare(got, ref_at(int(p)), pp == p, parts, "%s, tiles at %d passes" % (what, p))


class FrameCtx:
    """A frame that answers the reads test_gpu_tiles.assert_tiles makes of a context (for the checks of that helper without a device)."""

    def __init__(self, frame, tile_passes):
        self.w, self.h, self._f, self._p = W, H, frame, np.asarray(tile_passes, np.uint32)

    def tile_passes(self):
        return self._p

    def read_colors(self):
        return self._f["colors"]

    def read_seeds(self):
        return self._f["seeds"]

    def read_pixels(self):
        return self._f["pixels"]


# ---- contexts: needs a device from here on ---------------------------------------------------------------------------------------------------
class Checked(api.RtContext):
    """A context of a row: every launch is followed by the assertion that the row's instance rendered it."""
    expect, launches, after = None, 0, None

    def _launched(self):
        assert self.last_kernel == self.expect, "launch %d: %s rendered, the row is %s's" % (self.launches + 1, self.last_kernel, self.expect)
        self.launches += 1
        if self.after and self.launches in self.after:
            self.after[self.launches]()

    def render_pass(self, n_samples, copy=True, out=None):
        out = super().render_pass(n_samples, copy, out)
        self._launched()
        return out

    def render_async(self, n_samples, stream=None):
        super().render_async(n_samples, stream)
        self._launched()

    def render_tiles_async(self, n_samples, stream=None):
        super().render_tiles_async(n_samples, stream)
        self._launched()


def waves_of(row):
    return 1 if row.kernel.endswith("_w1") else 4


def make(row, **kw):
    """A fresh context of the row's library with the row's scene, set up so that the row's instance renders."""
    sph, cam = scene(row.scene)
    ctx = Checked(W, H, diag=row.library == "diagnostics", **kw)
    ctx.expect = row.kernel
    if row.library == "diagnostics":            # (as test_gpu_bvh._render(inst=...): the tables every instance may want exist)
        ctx._check(ctx._lib.rt_debug_set_choice_estimate(ctx._h, 1))
        ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, 1))
        ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
        ctx._check(ctx._lib.rt_debug_set_walk(ctx._h, 0, 0, 1))
    ctx.set_scene(sph)
    ctx.set_camera(cam)
    ctx.set_mode(api.instance_mode(row.kernel) if row.library == "diagnostics" else (api.RT_MODE_FAST if row.fast else api.RT_MODE_PARITY))
    return ctx


def frame_of(ctx, pixels=None):
    """What a context holds: colour plane, seeds, packed pixels (rt_read_pixels, or the buffer a launch returned) and the five counters."""
    return {"colors": ctx.read_colors(), "seeds": ctx.read_seeds(), "pixels": ctx.read_pixels() if pixels is None else pixels,
            "counters": counters_of(ctx.stats())}


def straight(row, p, stream_id=0):
    """One launch of `p` passes on a fresh context (on seed stream `stream_id`)."""
    with make(row) as ctx:
        if stream_id:
            ctx.seed_stream(stream_id, ctx.stream)
        px = ctx.render_pass(p)
        assert ctx.current_sample == p and ctx.stats()["launches"] == 1
        return frozen(frame_of(ctx, px))


@functools.lru_cache(maxsize=None)
def reference(row, p, stream_id=0):
    """The row's own straight p-pass render; computed once, read-only.  A parity row's must first be the oracle's."""
    got = straight(row, p, stream_id)
    if not row.fast:
        compare(got, oracle_frame(row.scene, p, stream_id), what="%s against the oracle, %d passes, stream %d" % (row_id(row), p, stream_id))
    return got


def minus(a, b):
    return tuple(x - y for x, y in zip(a, b))


# ---- the scripts: each ends in a comparison of every word against the reference at the pass count the pixel holds -------------------------------
def split_launches(row):
    want = reference(row, 6)
    for split in ((4, 2), (1, 1, 1, 3)):
        with make(row) as ctx:
            for n in split:
                px = ctx.render_pass(n)
            assert ctx.current_sample == 6 and ctx.launches == len(split)
            compare(frame_of(ctx, px), want, what="launches of %s" % (split,))
            compare(frame_of(ctx), want, what="launches of %s, rt_read_pixels" % (split,))


def pixel_store_off(row):
    for last in (True, False):
        with make(row) as ctx:
            first = ctx.render_pass(2)
            compare(frame_of(ctx, first), reference(row, 2), what="the first two passes")
            ctx.set_pixel_write(0)
            held = ctx.render_pass(2)               # (the buffer itself: rt_read_pixels would pack it first)
            compare({"pixels": held}, reference(row, 2), parts=("pixels",), what="the pixel buffer behind a launch with the store off")
            if last:
                ctx.set_pixel_write(1)
                px = ctx.render_pass(2)
                assert ctx.current_sample == 6 and ctx.launches == 3
                compare(frame_of(ctx, px), reference(row, 6), what="2 + 2 (store off) + 2")
            else:
                assert ctx.current_sample == 4 and ctx.launches == 2
                compare(frame_of(ctx), reference(row, 4), what="2 + 2 (store off), packed by rt_read_pixels")


def heavy_first_order(row):
    """(The forced-shape block of test_every_kernel_instance_in_the_libraries_has_parity: the first launch leaves its tiles' costs, the second sorts
    from them, walks the order and leaves its own, the third walks the order.)"""
    want = reference(row, 8)
    with make(row) as ctx:
        for k in range(3):
            ctx.reset()
            px = ctx.render_pass(8)
            compare(frame_of(ctx, px), want, what="frame %d of three under the heavy-first order" % k)
        assert ctx.launches == 3
        if row.library == "diagnostics":        # the instance took part: an order sorted from costs is in hand, a permutation of the launch's tiles
            import ctypes as C
            tiles = 3 * (-(-W // (8 * waves_of(row))))
            order, cost = np.zeros(18, np.uint32), np.zeros(18, np.uint32)
            n, valid = C.c_uint32(), C.c_int()
            ctx._check(ctx._lib.rt_debug_read_tile_order(ctx._h, order.ctypes.data, cost.ctypes.data, order.size, C.byref(n), C.byref(valid)))
            assert valid.value == 1 and n.value == tiles and sorted(order[:tiles].tolist()) == list(range(tiles))


def subset_launches(row):
    pixels_in = T.tile_pixels(W, H)
    for store_off in (False, True):
        with make(row) as ctx:
            if store_off:
                ctx.after = {1: lambda: ctx.set_pixel_write(0)}        # during the subset launches; rt_read_pixels packs every tile at the end
            passes = ragged_sequence(ctx)
            assert passes.tolist() == PASS_MAP and ctx.launches == 4
            # S3 leaves a list shorter than a grid row in either tile shape: sentinel workgroups ran
            m = int(S3.sum()) if waves_of(row) == 4 else int(T.tiles_of(S3, W, H).sum())
            tiles_x = -(-W // (8 * waves_of(row)))
            assert m % tiles_x != 0, (m, tiles_x)
            assert_tiles(ctx, passes, lambda p: reference(row, p))
            compare_at(frame_of(ctx), passes, lambda p: reference(row, p), what="ragged sequence%s" % (", store off" if store_off else ""))
            st = ctx.stats()
            assert st["samples"] == int((pixels_in * passes).sum()) and st["launches"] == 4
            # the other four counters: every group's share of the straight renders' (a pixel's work is its own) cannot be had from whole-frame
            # counters; what can: two full passes, then only additions -- no counter below the 2-pass frame's, none above the 7-pass frame's
            got = counters_of(st)
            assert all(a <= g <= b for a, g, b in zip(reference(row, 2)["counters"], got, reference(row, 7)["counters"])), got


def reset_in_place_then_subset(row):
    with make(row) as ctx:
        ctx.render_async(2, ctx.stream)
        ctx.reset_async(ctx.stream)
        assert ctx.current_sample == 0
        assert select(ctx, S1) == (4, 12)
        ctx.render_tiles_async(2, ctx.stream)
        assert ctx.current_sample == 2 and ctx.launches == 2
        passes = T.advance_restated(np.zeros((3, 6)), S1, 2, W, H)
        assert np.array_equal(ctx.tile_passes(), passes)
        got, chosen = frame_of(ctx), group_pixels(S1)
        compare(got, reference(row, 2), chosen, ("colors", "seeds", "pixels"), "the selected groups behind an in-place reset")
        pristine = {"colors": np.zeros(3 * W * H, np.float32), "seeds": host.default_seeds(2 * W * H)}
        compare(got, pristine, ~chosen, ("colors", "seeds"), "the groups left out behind an in-place reset")
        assert got["counters"][0] == int((T.tile_pixels(W, H) * passes).sum())
        ctx.reset()
        px = ctx.render_pass(3)
        assert np.all(ctx.tile_passes() == 3)
        compare(frame_of(ctx, px), reference(row, 3), what="rt_reset and three passes behind the subset launch")


def seed_stream_and_resume(row):
    early, want = reference(row, 3, STREAM), reference(row, 7, STREAM)
    with make(row) as a, make(row) as b:
        a.seed_stream(STREAM, a.stream)
        px = a.render_pass(3)
        compare(frame_of(a, px), early, what="three passes on stream %d" % STREAM)
        b.write_state(a.read_colors(), a.read_seeds(), 3)
        assert b.current_sample == 3 and b.launches == 0
        px = b.render_pass(4)
        assert b.current_sample == 7
        got = frame_of(b, px)
        compare(got, want, parts=("colors", "seeds", "pixels"), what="four more passes from the written state")
        assert got["counters"] == minus(want["counters"], early["counters"])       # (a written state restarts the counters)


def shards(row):
    want = reference(row, 6)
    for nranks, tile_rows in ((3, 8), (2, 16)):
        total, owned = (0,) * 5, np.zeros(H, int)
        for r in range(nranks):
            with make(row, rank=r, nranks=nranks, tile_rows=tile_rows) as ctx:
                ctx.render_pass(2)
                px = ctx.render_pass(4)
                assert ctx.current_sample == 6 and ctx.launches == 2
                assert_state(ctx, want, px)
                assert_state(ctx, want)                 # ... and through rt_read_pixels
                owned[ctx.local_row_map()] += 1
                total = tuple(x + y for x, y in zip(total, counters_of(ctx.stats())))
        assert np.all(owned == 1)                       # (the shards' rows tile the image)
        assert total == want["counters"], (nranks, tile_rows, total, want["counters"])


SCRIPTS = collections.OrderedDict((f.__name__, f) for f in (split_launches, pixel_store_off, heavy_first_order, subset_launches,
                                                            reset_in_place_then_subset, seed_stream_and_resume, shards))
CELLS = [(row, script) for row, script in itertools.product(ROWS, SCRIPTS) if (row_id(row), script) not in DIAGNOSTICS_ONLY]
