"""A shadow of ONE context's progressive frame, for the sequence tests (tests/test_gpu_frame_sequences.py): what include/rt_api.h says every
call does to colours, seeds, tile pass counts, pass number, selection and counters, kept in numpy and advanced with the CPU oracle.  One method
per API call; each returns ACCEPTED with the shadow updated, or the refusal code the header documents with the shadow untouched.  No device is
touched here: rendering is tests/_oracle.py render(first_sample, seeds_in, colors_in) -- pixels are independent, so copying the selected tiles
out of a whole-image oracle render is exact -- selection and merges are the numpy restatements of tests/test_tiles_cpu.py and
tests/test_gpu_state.py, the filter is the host function rt_denoise_planes (held to numpy by tests/test_denoise_cpu.py).  That host filter
is the only code of the library under test the shadow runs; the modules it imports helpers from bind the library lazily and touch no device.
tests/test_frame_shadow_cpu.py holds the shadow itself to csrc/rt_frame_state.h and to the straight oracle."""
import numpy as np

import _oracle as O
import test_tiles_cpu as T
from raytracing_simple_amd import api
from test_gpu_state import bits, camera, merge_restated, oracle, pack, scene
from test_state_cpu import restated_stream

W, H = 41, 23            # 6 x 3 tiles, 2 x 3 groups (tests/test_tiles_cpu.py pins the shape by hand)
ACCEPTED = "accepted"
RT_ERR_ARG, RT_ERR_STATE = -1, -5


def marked_map(mask, also, w=W, h=H):
    """The error map test_gpu_tiles.select hands the device: 1 in the last tile of every group of `mask` and of `also`."""
    ty, tx, gx = T.shape(w, h)
    marked = np.asarray(mask, bool) | (np.zeros((ty, gx), bool) if also is None else np.asarray(also, bool))
    err = np.zeros((ty, tx), np.uint32)
    for y, g in zip(*np.nonzero(marked)):
        err[y, min(4 * g + 3, tx - 1)] = 1
    return err


def per_pixel(tile_values, w=W, h=H):
    """A tile map spread over the pixels, row 0 = bottom as the pixel and seed buffers."""
    return np.repeat(np.repeat(np.asarray(tile_values), 8, axis=0), 8, axis=1)[:h, :w]


class Shadow:
    def __init__(self, name="demo", w=W, h=H):
        self.name, self.w, self.h = name, w, h
        self.ty, self.tx, self.gx = T.shape(w, h)
        self.stream = 0                                      # seed stream id
        self.colors = np.zeros(3 * w * h, np.float32)        # the colour plane as rt_read_colors returns it (y-flipped against the tile map)
        self.seeds = O.seeds(w, h)
        self.passes = np.zeros((self.ty, self.tx), np.int64)
        self.cur = 0
        self.ragged = False                                  # what the header calls ragged: set by subset launches and per-tile merges, cleared by resets
        self.have_selection, self.mask, self.counts = False, None, (0, 0)
        self.launches = self.samples = 0                     # since the last reset or written state
        self.pixel_write = True
        # tiles whose WHOLE history is rendering on self.stream from pass 0: check() also holds them to the cached straight render
        self.pure = np.ones((self.ty, self.tx), bool)

    # ---- views ----------------------------------------------------------------------------------------------------------
    def _plane(self, colors=None):
        """[h, w, 3] with row 0 = bottom, a view of the plane."""
        return (self.colors if colors is None else colors).reshape(self.h, self.w, 3)[::-1]

    def pixels(self):
        return pack(self.colors, self.w, self.h)

    def rendered(self):
        """Pixels inside tiles that hold a pass, bool [h, w]: where the packed frame is specified."""
        return per_pixel(self.passes > 0, self.w, self.h)

    def left_out(self):
        return int((~self.rendered()).sum())

    def tile_map(self):
        return self.passes if self.ragged else np.full((self.ty, self.tx), self.cur, np.int64)

    def facts(self):
        """What tests/test_frame_shadow_cpu.py compares with the compiled record."""
        return (self.cur, int(self.ragged), int(self.have_selection), self.counts[0], self.counts[1], self.launches)

    # ---- the pieces -----------------------------------------------------------------------------------------------------
    def _whole(self, pass_number):
        self.cur, self.ragged = pass_number, False
        self.passes = np.full((self.ty, self.tx), pass_number, np.int64)
        self.have_selection, self.mask = False, None
        self.launches = self.samples = 0

    def _render(self, tiles, n):
        out = O.render(scene(self.name)[0], camera(self.name, self.w, self.h), self.w, self.h, n, first_sample=self.cur,
                       seeds_in=self.seeds, colors_in=self.colors)
        pm = per_pixel(tiles, self.w, self.h)
        self._plane()[pm] = self._plane(out["colors"])[pm]
        self.seeds.reshape(self.h, self.w, 2)[pm] = out["seeds"].reshape(self.h, self.w, 2)[pm]
        self.passes = self.passes + n * np.asarray(tiles, np.int64)
        self.cur += n
        self.launches += 1
        self.samples += n * int(pm.sum())

    # ---- one method per API call ----------------------------------------------------------------------------------------
    def reset(self):
        """rt_reset: pass 0 of the default stream, colour plane and pixels cleared."""
        self._whole(0)
        self.stream, self.seeds, self.colors = 0, O.seeds(self.w, self.h), np.zeros(3 * self.w * self.h, np.float32)
        self.pure[:] = True
        return ACCEPTED

    def reset_async(self):
        """rt_reset_async: the default stream read in place; plane and pixels are NOT cleared."""
        self._whole(0)
        self.stream, self.seeds = 0, O.seeds(self.w, self.h)
        self.pure[:] = True                                  # (pass 0 overwrites the old floats of whatever tile renders next)
        return ACCEPTED

    def seed_stream(self, stream_id):
        self.reset_async()
        if stream_id != 0:
            self.stream, self.seeds = stream_id, restated_stream(stream_id, 2 * self.w * self.h).copy()
        return ACCEPTED

    def write_state(self, colors, seeds, pass_number):
        if pass_number < 0 or (colors is None and pass_number != 0):
            return RT_ERR_ARG
        self._whole(pass_number)
        if colors is not None:
            self.colors = np.array(colors, np.float32).reshape(-1)
        self.seeds = O.seeds(self.w, self.h) if seeds is None else np.array(seeds, np.uint32).reshape(-1)
        self.stream = 0 if seeds is None else None           # (somebody else's seeds: no stream of ours)
        self.pure[:] = pass_number == 0 and seeds is None
        return ACCEPTED

    load_state = write_state                                 # rt_load_state: the same through a file

    def set_pixel_write(self, enable):
        self.pixel_write = bool(enable)
        return ACCEPTED

    def render_async(self, n):
        if self.ragged:
            return RT_ERR_STATE
        if n < 0:
            return RT_ERR_ARG
        if n > 0:
            self._render(np.ones((self.ty, self.tx), bool), n)
        return ACCEPTED

    render_pass = render_async                               # (blocking, and it times the launch: nothing the shadow holds)

    def select(self, err, above):
        """rt_select_tiles from a HOST copy of the map (None: every group at the front)."""
        self.mask, self.counts = T.select_restated(self.w, self.h, self.tile_map(), self.cur, err, above)
        self.have_selection = True
        return ACCEPTED

    def render_tiles_async(self, n):
        if n < 0:
            return RT_ERR_ARG
        if not self.have_selection:
            return RT_ERR_STATE
        if n == 0 or self.counts[0] == 0:
            return ACCEPTED
        every = self.counts[0] == self.ty * self.gx
        if self.cur == 0 and not every:                      # from pass 0 the groups left out hold a 0-pass render: the plane is cleared ahead of the launch
            self.colors = np.zeros(3 * self.w * self.h, np.float32)
        self.passes = self.tile_map().copy()
        self._render(T.tiles_of(self.mask, self.w, self.h), n)
        self.ragged = not every
        return ACCEPTED

    def merge(self, sources):
        """rt_merge_async(self, sources): whole contexts by merge_restated, a ragged one among them by merge_tiles_restated; dst's seeds stay."""
        everyone = [self] + list(sources)
        total = sum(x.cur for x in everyone if x.cur > 0)
        if total == 0:
            return RT_ERR_STATE
        if not any(x.ragged for x in everyone):
            self.colors = merge_restated([x.colors for x in everyone], [x.cur for x in everyone])
            self.passes = np.full((self.ty, self.tx), total, np.int64)
        else:
            self.colors, counts = T.merge_tiles_restated([x.colors for x in everyone], [x.tile_map() for x in everyone], self.w, self.h)
            self.colors = np.ascontiguousarray(self.colors, np.float32)
            self.passes, self.ragged = counts.astype(np.int64), True
        self.cur = total
        self.have_selection = False
        self.pure[:] = False
        return ACCEPTED

    def denoise(self, a, b):
        if a.cur != b.cur or a.cur <= 0 or self.cur != 2 * a.cur:
            return RT_ERR_STATE
        self.colors = api.denoise_planes(self.colors, a.colors, b.colors, self.w, self.h)
        self.pure[:] = False
        return ACCEPTED


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def assert_straight(sh, colors, seeds, pixels=None):
    """Every tile whose whole history is rendering on one stream holds the cached straight render at its count -- oracle(name, w, h, p,
    stream), independent of the shadow's own continuation; at 0 passes, the stream's first seeds."""
    w, h = sh.w, sh.h
    col, sd = bits(colors).reshape(h, w, 3)[::-1], np.asarray(seeds).reshape(h, w, 2)
    tiles = sh.tile_map()
    for p in np.unique(tiles[sh.pure]):
        m = per_pixel(sh.pure & (tiles == p), w, h)
        if p == 0:
            first = O.seeds(w, h) if sh.stream == 0 else restated_stream(sh.stream, 2 * w * h)
            assert np.array_equal(sd[m], first.reshape(h, w, 2)[m])
            continue
        want = oracle(sh.name, w, h, int(p), sh.stream)
        assert np.array_equal(col[m], bits(want["colors"]).reshape(h, w, 3)[::-1][m]), p
        assert np.array_equal(sd[m], want["seeds"].reshape(h, w, 2)[m]), p
        if pixels is not None:
            assert np.array_equal(np.asarray(pixels).reshape(h, w)[m], want["pixels"].reshape(h, w)[m]), p


def check(ctx, sh, left_out=0, read_pixels=True):
    """The context equals its shadow: pass number, tile counts, colour bits, seeds, counters, and the packed frame on every tile that holds a
    pass (`left_out` pixels lie in tiles at 0 passes, where include/rt_api.h leaves the packed frame unspecified).  read_pixels=False skips
    rt_read_pixels, which packs the frame and so changes what a later call finds."""
    assert ctx.current_sample == sh.cur
    assert np.array_equal(ctx.tile_passes(), sh.tile_map().astype(np.uint32))
    colors, seeds = ctx.read_colors(), ctx.read_seeds()
    assert np.array_equal(bits(colors), bits(sh.colors))
    assert np.array_equal(seeds, sh.seeds)
    st = ctx.stats()
    assert (st["launches"], st["samples"]) == (sh.launches, sh.samples)
    assert sh.left_out() == left_out
    pixels = None
    if read_pixels:
        pixels, m = ctx.read_pixels(), sh.rendered()
        assert np.array_equal(pixels.reshape(sh.h, sh.w)[m], sh.pixels().reshape(sh.h, sh.w)[m])
    assert_straight(sh, colors, seeds, pixels)


# ---- a script's cast --------------------------------------------------------------------------------------------------------
class Actor:
    """One context of a script beside its shadow.  A script (tests/test_gpu_frame_sequences.py) is a literal list of calls on actors; every
    call goes to the shadow first -- `expect` is ACCEPTED or the refusal code the header documents -- and then to `_perform`, which the two
    casts fill in: the device (the call on the context, then check()) and the compiled record (tests/test_frame_shadow_cpu.py: the events
    the call is supposed to report).  `left_out`: pixels in tiles at 0 passes after the call, stated by the script, asserted against the
    shadow's own count.  read_pixels=False keeps check() from packing the frame, where a later call has to find it stale: rt_read_pixels packs
    the frame and marks it current, and the stale buffer itself holds nothing to compare, so scripts J and K read the pixels only where the call
    under test is the one that has to pack them (everything else -- pass, counts, colours, seeds, counters -- is still compared at those steps)."""

    def __init__(self, key, name="demo"):
        self.key, self.sh = key, Shadow(name)

    def _step(self, call, sh_args, args, expect=ACCEPTED, left_out=0, read_pixels=True):
        before = self.sh.facts()
        got = getattr(self.sh, call)(*sh_args)
        assert got == expect, (self.key, call, got)
        assert got == ACCEPTED or self.sh.facts() == before
        assert self.sh.left_out() == left_out, (self.key, call, self.sh.left_out())
        self._perform(call, args, got, left_out, read_pixels)

    def _perform(self, call, args, got, left_out, read_pixels):
        raise NotImplementedError

    # state-changing calls
    def reset(self, **kw): self._step("reset", (), (), **kw)
    def reset_async(self, **kw): self._step("reset_async", (), (), **kw)
    def seed_stream(self, stream_id, **kw): self._step("seed_stream", (stream_id,), (stream_id,), **kw)
    def set_pixel_write(self, enable, **kw): self._step("set_pixel_write", (enable,), (enable,), **kw)
    def render_async(self, n, **kw): self._step("render_async", (n,), (n,), **kw)
    def render_pass(self, n, **kw): self._step("render_pass", (n,), (n,), **kw)
    def render_tiles_async(self, n, **kw): self._step("render_tiles_async", (n,), (n,), **kw)
    def write_state(self, colors, seeds, n, **kw): self._step("write_state", (colors, seeds, n), (colors, seeds, n), **kw)
    def merge(self, sources, **kw): self._step("merge", ([s.sh for s in sources],), (sources,), **kw)
    def denoise(self, a, b, **kw): self._step("denoise", (a.sh, b.sh), (a, b), **kw)

    def load_state(self, saved_from, **kw):
        """rt_load_state of a checkpoint rt_save_state wrote from the whole context `saved_from`."""
        assert not saved_from.sh.ragged
        self._step("load_state", (saved_from.sh.colors, saved_from.sh.seeds, saved_from.sh.cur), (saved_from,), **kw)

    def select(self, mask, also=None, counts=None, **kw):
        """test_gpu_tiles.select: above = 0 and a map that marks the groups of `mask` and of `also`; `counts` is what the script expects back."""
        self._step("select", (marked_map(mask, also), 0), (mask, also), **kw)
        assert self.sh.counts == counts, self.sh.counts

    def select_all(self, counts=None, **kw):
        """rt_select_tiles with a NULL map: every group at the front."""
        self._step("select", (None, 0), (None, None), **kw)
        assert self.sh.counts == counts, self.sh.counts

    # calls that read: nothing for the shadow to do, everything for the cast (a cast that leaves one out must not pass a script that makes it)
    def compare(self, other): raise NotImplementedError
    def read_pixels_async(self): raise NotImplementedError
    def counters(self, want): raise NotImplementedError
    def tile_list(self, mask): raise NotImplementedError
