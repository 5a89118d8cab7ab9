"""A frame walked through every state transition on the device, call by call -- the device-side counterpart of DESIGN.md section 5.10's table
(tests/test_frame_state_cpu.py holds csrc/rt_frame_state.h to that table; this file holds the CALL SITES to it: whether every API call reports
the right event at the right moment).  Each script below is a literal list of calls on one or more contexts at 41 x 23 (Demo scene), every call
mirrored on a shadow (tests/_frame_shadow.py: numpy and the CPU oracle) and followed by check(): pass number, tile counts, colour bits, seeds,
packed pixels and counters.  The scripts meet where two features meet: a subset launch after an in-place reset, rendering on after a merge,
calls that make a ragged context whole, the filter and the pixel store across subset launches.  tests/test_frame_shadow_cpu.py runs the same
scripts without a device against the compiled record, so a mistake in a script is found there."""
import ctypes as C
import tempfile

import numpy as np
import pytest
import torch  # noqa: F401  (before the library first touches the device, as tests/test_gpu_denoise.py explains)

import test_tiles_cpu as T
from _frame_shadow import ACCEPTED, H, RT_ERR_STATE, W, Actor, check
from test_compare_cpu import frame_error_restated
from test_gpu_state import _refused, assert_counters, assert_unchanged, bits, make, oracle, snapshot
from test_gpu_tiles import S1, S2, S3, select

pytestmark = pytest.mark.gpu

ALL = W * H                                                  # 943 pixels: what a context at pass 0 leaves out of the pixel comparison
OUT1, OUT2, OUT3 = 328, 624, 880                             # ... and what lies outside S1, S2, S3 (test_tiles_cpu: 64, 56, 8 and 7 pixels per tile)


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def equals_straight(sh, passes, stream=0):
    """The shadow is the straight oracle render of `passes` passes: colours, seeds, pass number."""
    want = oracle("demo", W, H, passes, stream)
    return sh.cur == passes and not sh.ragged and np.array_equal(bits(sh.colors), bits(want["colors"])) and np.array_equal(sh.seeds, want["seeds"])


def script_a(cast):
    """In-place reset, then a subset on the default stream: launch_tiles' `seeds_default && !all` branch."""
    x = cast("x")
    x.render_async(2)
    x.reset_async(left_out=ALL)
    x.select(S1, counts=(4, 12), left_out=ALL)
    x.render_tiles_async(2, left_out=OUT1)                    # the tiles left out: 0 passes, the pristine default stream (check: assert_straight)
    assert x.sh.passes.tolist() == [[0, 0, 0, 0, 2, 2], [2, 2, 2, 2, 0, 0], [2, 2, 2, 2, 2, 2]]
    x.select_all(counts=(4, 12), left_out=OUT1)               # the front: exactly the groups of S1
    assert np.array_equal(x.sh.mask, S1)
    x.render_tiles_async(1, left_out=OUT1)
    x.reset(left_out=ALL)
    x.render_pass(3)
    assert equals_straight(x.sh, 3)
    x.counters(oracle("demo", W, H, 3))


def script_b(cast):
    """... with a custom stream first: seeds_custom is still set after the in-place reset, and the default stream must be read."""
    x = cast("x")
    x.seed_stream(3, left_out=ALL)
    x.render_async(1)
    x.reset_async(left_out=ALL)
    x.select(S2, counts=(2, 6), left_out=ALL)
    x.render_tiles_async(1, left_out=OUT2)
    m = T.pixel_weights(T.tiles_of(S2, W, H), W, H) != 0       # the floats of the S2 tiles
    assert np.array_equal(bits(x.sh.colors)[m], bits(oracle("demo", W, H, 1, 0)["colors"])[m])
    assert not np.array_equal(bits(x.sh.colors)[m], bits(oracle("demo", W, H, 1, 3)["colors"])[m])


def script_c(cast):
    """Every group selected after an in-place reset: the frame stays whole, the pristine stream is read in place."""
    x = cast("x")
    x.render_async(2)
    x.reset_async(left_out=ALL)
    x.select_all(counts=(6, 18), left_out=ALL)
    x.render_tiles_async(2)
    assert not x.sh.ragged
    x.render_async(1)
    assert equals_straight(x.sh, 3) and x.sh.launches == 2


def script_d(cast):
    """A selection outlives a whole-frame launch (launched() keeps have_selection; the selected groups stay at the front)."""
    x = cast("x")
    x.render_async(2)
    x.select(S1, counts=(4, 12))
    x.render_async(1)
    x.render_tiles_async(1)
    assert x.sh.passes.tolist() == [[3, 3, 3, 3, 4, 4], [4, 4, 4, 4, 3, 3], [4, 4, 4, 4, 4, 4]]
    x.render_tiles_async(2)                                   # no new selection
    assert x.sh.passes.tolist() == [[3, 3, 3, 3, 6, 6], [6, 6, 6, 6, 3, 3], [6, 6, 6, 6, 6, 6]] and x.sh.cur == 6


def script_e(cast):
    """Render on after a per-tile merge: the front moves to the sum, only the tiles whose sum equals it continue, from the merged floats."""
    a, b, c = cast("a"), cast("b"), cast("c")
    for k, x in enumerate((a, b, c)):
        x.seed_stream(k + 1, left_out=ALL)
    a.render_async(2)                                         # (the contexts of test_merge_weights_every_tile_by_its_own_count)
    a.select(S1, counts=(4, 12))
    a.render_tiles_async(3)
    b.render_async(3)
    b.select(S2, counts=(2, 6))
    b.render_tiles_async(1)
    c.render_async(2)
    c.reset_async(left_out=ALL)
    c.seed_stream(3, left_out=ALL)
    c.select(S3, counts=(1, 2), left_out=ALL)
    c.render_tiles_async(2, left_out=OUT3)
    a.merge([b, c])
    assert a.sh.cur == 11 and a.sh.passes.tolist() == [[5, 5, 5, 5, 8, 8], [9, 9, 9, 9, 5, 5], [8, 8, 8, 8, 11, 11]]
    a.render_async(1, expect=RT_ERR_STATE)
    a.select_all(counts=(1, 2))                               # the one group at 11
    assert np.array_equal(a.sh.mask, S3)
    a.render_tiles_async(2)                                   # first_sample = 11, a's own seeds
    assert a.sh.cur == 13 and a.sh.passes[2].tolist() == [8, 8, 8, 8, 13, 13]
    a.compare(b)


def script_f(cast):
    """A tile nobody holds keeps dst's floats and gets count 0."""
    dst, src = cast("dst"), cast("src")
    for k, x in enumerate((dst, src)):
        x.render_async(2)
        x.reset_async(left_out=ALL)
        x.seed_stream(k + 1, left_out=ALL)
        x.select(S3, counts=(1, 2), left_out=ALL)
        x.render_tiles_async(2, left_out=OUT3)
    old = bits(dst.sh.colors).copy()
    dst.merge([src], left_out=OUT3)
    held = T.pixel_weights(T.tiles_of(S3, W, H), W, H) != 0
    assert np.array_equal(bits(dst.sh.colors)[~held], old[~held]) and not np.array_equal(bits(dst.sh.colors)[held], old[held])
    assert dst.sh.cur == 4 and dst.sh.passes.tolist() == [[0] * 6, [0] * 6, [0, 0, 0, 0, 4, 4]]


def script_g(cast):
    """Whole and ragged mixed, six sources: both kinds of passes[k] in the unrolled loop, a whole source at pass 0 that must not contribute."""
    dst = cast("dst")
    dst.seed_stream(1, left_out=ALL)
    dst.render_async(2)
    dst.select(S1, counts=(4, 12))
    dst.render_tiles_async(1)
    three, zero = cast("three"), cast("zero")
    three.seed_stream(2, left_out=ALL)
    three.render_async(3)
    zero.seed_stream(3, left_out=ALL)
    zero.render_async(2)
    zero.reset_async(left_out=ALL)                            # pass 0, an old frame in the plane
    ones = [cast("one%d" % k) for k in range(4)]
    for k, x in enumerate(ones):
        x.seed_stream(4 + k, left_out=ALL)
        x.render_async(1)
    dst.merge([three, zero] + ones)
    assert dst.sh.cur == 10 and dst.sh.passes.tolist() == [[9, 9, 9, 9, 10, 10], [10, 10, 10, 10, 9, 9], [10] * 6]


def ragged(x):
    """test_gpu_tiles.ragged_sequence, call by call."""
    x.render_async(2)
    for mask, also, n, counts in ((S1, None, 1, (4, 12)), (S2, ~S1, 3, (2, 6)), (S3, ~S2, 1, (1, 2))):
        x.select(mask, also, counts=counts)
        x.render_tiles_async(n)
    assert x.sh.passes.tolist() == [[2, 2, 2, 2, 3, 3], [6, 6, 6, 6, 2, 2], [3, 3, 3, 3, 7, 7]] and x.sh.ragged


def script_h_write_state(cast):
    """Calls that make a ragged context whole: rt_write_state of a straight 5-pass state."""
    x = cast("x")
    ragged(x)
    five = oracle("demo", W, H, 5)
    x.write_state(five["colors"], five["seeds"], 5)
    assert np.all(x.sh.tile_map() == 5)
    x.render_tiles_async(1, expect=RT_ERR_STATE)              # the selection went with it
    x.render_async(1)
    assert equals_straight(x.sh, 6)


def script_h_load_state(cast):
    """... rt_load_state of a checkpoint saved from a whole context."""
    x, whole = cast("x"), cast("whole")
    ragged(x)
    whole.render_async(5)
    x.load_state(whole)
    assert np.all(x.sh.tile_map() == 5)
    x.render_tiles_async(1, expect=RT_ERR_STATE)
    x.render_async(1)
    assert equals_straight(x.sh, 6)


def script_h_seed_stream(cast):
    """... rt_seed_stream_async."""
    x = cast("x")
    ragged(x)
    x.seed_stream(4, left_out=ALL)
    x.render_tiles_async(1, expect=RT_ERR_STATE, left_out=ALL)
    x.render_async(2)
    assert equals_straight(x.sh, 2, 4)


def script_h_default_route(cast):
    """... rt_write_state(NULL, NULL, 0), the seeds_default route; then as script A."""
    x = cast("x")
    ragged(x)
    x.write_state(None, None, 0, left_out=ALL)
    x.render_tiles_async(1, expect=RT_ERR_STATE, left_out=ALL)
    x.select(S1, counts=(4, 12), left_out=ALL)
    x.render_tiles_async(1, left_out=OUT1)
    assert x.sh.passes.tolist() == [[0, 0, 0, 0, 1, 1], [1, 1, 1, 1, 0, 0], [1] * 6]


def script_i(cast):
    """A whole-frame merge drops the selection (and the list, which it leaves marked valid, must be built again for the next one)."""
    a, b = cast("a", diag=True), cast("b", diag=True)
    a.seed_stream(1, left_out=ALL)
    a.render_async(2)
    b.seed_stream(2, left_out=ALL)
    b.render_async(3)
    a.select(S1, counts=(4, 12))
    a.merge([b])
    assert a.sh.cur == 5 and not a.sh.ragged
    a.render_tiles_async(1, expect=RT_ERR_STATE)
    a.select(S1, counts=(4, 12))
    a.render_tiles_async(1)                                   # the S1 tiles continue the merged floats
    a.tile_list(S1)
    assert a.sh.passes.tolist() == [[5, 5, 5, 5, 6, 6], [6, 6, 6, 6, 5, 5], [6] * 6]


def script_j(cast, pixel_write=1):
    """The filter, then everything else; whoever reads the packed frame after a merge or the filter has to pack it first."""
    a, b, dst = cast("a"), cast("b"), cast("dst")
    for k, x in enumerate((a, b)):
        x.set_pixel_write(pixel_write, left_out=ALL)
        x.seed_stream(k + 1, left_out=ALL)
        x.render_async(4, read_pixels=False)
    dst.set_pixel_write(pixel_write, left_out=ALL)
    dst.merge([a, b], read_pixels=False)
    dst.compare(a)                                            # merged() left the pixels stale: the pack runs inside rt_compare
    dst.denoise(a, b, read_pixels=False)
    dst.compare(a)                                            # ... and so did colours_replaced()
    dst.read_pixels_async()
    dst.render_async(1, read_pixels=False)                    # continues the filtered plane
    dst.read_pixels_async()                                   # (store off: packed on the caller's stream)
    dst.select(S2, counts=(2, 6), read_pixels=False)
    dst.render_tiles_async(1)
    assert dst.sh.cur == 10 and dst.sh.ragged


def script_j_store_off(cast):
    script_j(cast, 0)


def script_k(cast):
    """Pixel store toggled across subset launches: a launch with the store on leaves pixels_current false while tiles it left out were never packed."""
    x = cast("x")
    x.set_pixel_write(0, left_out=ALL)
    x.render_async(2, read_pixels=False)
    x.select(S1, counts=(4, 12), read_pixels=False)
    x.render_tiles_async(1, read_pixels=False)
    x.set_pixel_write(1, read_pixels=False)
    x.select(S2, counts=(2, 6), read_pixels=False)
    x.render_tiles_async(1)                                   # read: tiles rendered with the store off, with it on, and not at all since
    assert x.sh.passes.tolist() == [[2, 2, 2, 2, 3, 3], [4, 4, 4, 4, 2, 2], [3, 3, 3, 3, 4, 4]]


SCRIPTS = [script_a, script_b, script_c, script_d, script_e, script_f, script_g, script_h_write_state, script_h_load_state, script_h_seed_stream,
           script_h_default_route, script_i, script_j, script_j_store_off, script_k]


# ---- the cast on the device ---------------------------------------------------------------------------------------------------
class OnDevice(Actor):
    def __init__(self, key, diag=False):
        super().__init__(key)
        self.ctx = make("demo", diag=diag)
        if diag:
            self.ctx._check(self.ctx._lib.rt_debug_set_coop_min(self.ctx._h, 0))     # the plain one-wavefront instance for certain
        self.tmp = None

    def _call(self, call, args):
        ctx = self.ctx
        if call in ("reset", "render_pass", "set_pixel_write", "write_state"):
            return getattr(ctx, call), args
        if call in ("reset_async", "seed_stream", "render_async", "render_tiles_async"):
            return getattr(ctx, call), args + (ctx.stream,)
        if call == "merge":
            return ctx.merge, ([s.ctx for s in args[0]], ctx.stream)
        if call == "denoise":
            return ctx.denoise, (args[0].ctx, args[1].ctx, None, ctx.stream)
        if call == "load_state":
            self.tmp = self.tmp or tempfile.TemporaryDirectory()
            path = self.tmp.name + "/state.bin"
            args[0].ctx.save_state(path)
            return ctx.load_state, (path,)
        raise KeyError(call)

    def _perform(self, call, args, got, left_out, read_pixels):
        ctx = self.ctx
        if call == "select":
            mask, also = args
            counts = ctx.select_tiles(None, 0, ctx.stream) if mask is None else select(ctx, mask, also)
            assert counts == self.sh.counts
        else:
            fn, fn_args = self._call(call, args)
            if got == ACCEPTED:
                fn(*fn_args)
            else:
                snap = snapshot(ctx)
                _refused(ctx, got, fn, *fn_args)
                assert_unchanged(ctx, snap)
        check(ctx, self.sh, left_out, read_pixels)

    def compare(self, other):
        """rt_compare equals the restatement over the two shadows' packed frames (both hold a pass in every tile); then both frames."""
        assert self.sh.left_out() == 0 and other.sh.left_out() == 0
        assert self.ctx.compare(other.ctx) == frame_error_restated(self.sh.pixels(), other.sh.pixels(), W, H)[0]
        check(self.ctx, self.sh)
        check(other.ctx, other.sh)

    def read_pixels_async(self):
        """rt_read_pixels_async on a caller's stream, and that stream alone waited for."""
        stream, out = torch.cuda.Stream(), np.zeros(W * H, np.uint32)
        self.ctx.pin_output(out)
        self.ctx.read_pixels_async(out, stream.cuda_stream)
        stream.synchronize()
        self.ctx.pin_output(None)
        assert self.sh.left_out() == 0 and np.array_equal(out, self.sh.pixels())

    def counters(self, want):
        assert_counters(self.ctx, want)

    def tile_list(self, mask):
        """The list the last subset launch walked (diagnostics library): the restated stable filter, in image order or in the schedule's."""
        ctx, lib, n = self.ctx, self.ctx._lib, self.sh.ty * self.sh.tx
        assert ctx.last_kernel == "rt_trace_parity_w1"
        got = np.zeros(n + self.sh.tx, np.uint32)
        slots, n_launch, by_order = C.c_uint32(), C.c_uint32(), C.c_int()
        ctx._check(lib.rt_debug_read_tile_list(ctx._h, got.ctypes.data, got.size, C.byref(slots), C.byref(n_launch), C.byref(by_order)))
        order = None
        if by_order.value:
            order, cost, m, valid = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32(), C.c_int()
            ctx._check(lib.rt_debug_read_tile_order(ctx._h, order.ctypes.data, cost.ctypes.data, n, C.byref(m), C.byref(valid)))
            order = order[:m.value].tolist()
        want, grid = T.list_restated(W, H, 1, mask, order)
        assert (slots.value, n_launch.value) == (grid[0] * grid[1], n)
        assert np.array_equal(got[:slots.value], want)

    def close(self):
        self.ctx.close()
        if self.tmp:
            self.tmp.cleanup()


@pytest.mark.parametrize("script", SCRIPTS, ids=[s.__name__[7:] for s in SCRIPTS])
def test_sequence(script):
    actors = []

    def cast(key, **kw):
        actors.append(OnDevice(key, **kw))
        return actors[-1]

    try:
        script(cast)
        assert len(actors) <= 7                               # (script G's seven contexts are the most any script opens)
    finally:
        for a in actors:
            a.close()
