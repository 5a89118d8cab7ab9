"""Adaptive sampling (include/rt_api.h "adaptive sampling", csrc/rt_tiles.hip), the part that needs no device: a numpy restatement of
the selection rule, the subset launch's tile list, the per-tile merge and the driver's threshold -- what tests/test_gpu_tiles.py compares
the device against -- pinned here against cases worked out by hand at 41 x 23 (6 x 3 tiles, 2 x 3 groups; the right group holds two
tiles, one of them 1 pixel wide; the top row is 7 pixels high), and the argument checks that come before any device call."""
import ctypes as C
import math

import numpy as np

from raytracing_simple_amd import api
from test_compare_cpu import frame_error_restated

SYMBOLS = ("rt_tile_passes", "rt_select_tiles", "rt_render_tiles_async", "rt_render_adaptive")


# ---- the restatement -------------------------------------------------------------------------------------------------
def shape(w, rows):
    """(tiles_y, tiles_x, groups_x): 8x8 tiles of the local pixel buffer, and groups of four tiles per tile row."""
    tiles_x = (w + 7) // 8
    return (rows + 7) // 8, tiles_x, (tiles_x + 3) // 4


def tile_pixels(w, rows):
    """pixels(t): image pixels inside every 8x8 tile, int64 [tiles_y, tiles_x]."""
    ty, tx, _ = shape(w, rows)
    pw = np.minimum(8, w - 8 * np.arange(tx))
    ph = np.minimum(8, rows - 8 * np.arange(ty))
    return (ph[:, None] * pw[None, :]).astype(np.int64)


def tiles_of(mask, w, rows):
    """A group mask [tiles_y, groups_x] spread over the 8x8 tiles [tiles_y, tiles_x]."""
    _, tx, _ = shape(w, rows)
    return np.repeat(np.asarray(mask, bool), 4, axis=1)[:, :tx]


def threshold(db):
    """rt_render_adaptive's `above`: the tile's squared error at which the PSNR over its 192 channel values equals db."""
    return min(int(math.floor(255.0 * 255.0 * 192.0 / 10.0 ** (db / 10.0))), 2 ** 32 - 1)


def select_restated(w, rows, passes, cur, err, above):
    """rt_select_tiles: groups at the front (pass count == cur) with a tile whose err * 64 > above * pixels (err None: every front
    group).  Returns (bool [tiles_y, groups_x], (groups, 8x8 tiles covered))."""
    ty, tx, gx = shape(w, rows)
    passes = np.asarray(passes, np.int64).reshape(ty, tx)
    noisy = np.ones((ty, tx), bool) if err is None else np.asarray(err, np.int64).reshape(ty, tx) * 64 > int(above) * tile_pixels(w, rows)
    mask = np.zeros((ty, gx), bool)
    for y in range(ty):
        for g in range(gx):
            mask[y, g] = passes[y, 4 * g] == cur and noisy[y, 4 * g:4 * g + 4].any()
    return mask, (int(mask.sum()), int(tiles_of(mask, w, rows).sum()))


def advance_restated(passes, mask, n, w, rows):
    """Pass counts after a subset launch of n passes on the groups of `mask`."""
    return (np.asarray(passes, np.int64) + n * tiles_of(mask, w, rows)).astype(np.uint32)


def list_restated(w, rows, waves, mask, order=None):
    """The tile list of a subset launch for an instance of `waves` wavefronts per workgroup (tile 8 * waves x 8): the launch tiles whose
    group is selected, in `order` (default: image order), a stable filter; then the sentinel id up to whole grid rows.
    Returns (uint32 list, (grid_x, grid_y))."""
    ty, tx, gx = shape(w, rows)
    launch_x = gx if waves == 4 else tx
    n = launch_x * ty
    mask = np.asarray(mask, bool)
    keep = [t for t in (range(n) if order is None else order) if mask[t // launch_x, (t % launch_x) // (1 if waves == 4 else 4)]]
    grid_y = -(-len(keep) // launch_x)
    return np.array(keep + [n] * (launch_x * grid_y - len(keep)), np.uint32), (launch_x, grid_y)


def pixel_weights(tile_passes, w, h):
    """A tile map spread over the floats of the colour plane: float32 [3 * w * h], the plane y-flipped against the map (.cl:579)."""
    per_pixel = np.repeat(np.repeat(np.asarray(tile_passes, np.int64), 8, axis=0), 8, axis=1)[:h, :w][::-1]
    return np.repeat(per_pixel.reshape(-1), 3)


def merge_tiles_restated(planes, tile_passes, w, h):
    """rt_merge_async with ragged contexts: test_gpu_state.merge_restated with per-pixel weights.  planes[0] is dst's; a context whose tile
    holds no pass is skipped for that tile; where nobody holds one, dst's floats stay.  Returns (plane, tile counts)."""
    acc = np.zeros(3 * w * h, np.float32)
    total = np.zeros(3 * w * h, np.int64)
    for c, tp in zip(planes, tile_passes):
        n = pixel_weights(tp, w, h)
        term = np.asarray(c, np.float32) * n.astype(np.float32)
        acc = np.where(n == 0, acc, np.where(total == 0, term, (acc + term).astype(np.float32))).astype(np.float32)
        total = total + n
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (acc * (np.float32(1.0) / total.astype(np.float32))).astype(np.float32)
    return np.where(total == 0, np.asarray(planes[0], np.float32), out), sum(np.asarray(tp, np.int64) for tp in tile_passes).astype(np.uint32)


def compose(frame_at, tile_passes, w, h):
    """The packed frame of a ragged context: every tile from the uniform render with that tile's pass count.  frame_at(p) -> uint32 [h * w]."""
    per_pixel = np.repeat(np.repeat(np.asarray(tile_passes, np.int64), 8, axis=0), 8, axis=1)[:h, :w]
    out = np.zeros((h, w), np.uint32)
    for p in np.unique(per_pixel):
        out = np.where(per_pixel == p, np.asarray(frame_at(int(p))).reshape(h, w), out)
    return out.reshape(-1)


def adaptive_restated(frame_a, frame_b, w, h, tile_db, min_passes, per_check, max_passes, start=0):
    """rt_render_adaptive from frames alone: frame_a(p) / frame_b(p) give the packed p-pass frames of the two seed streams.
    Returns (reached, checks, tile pass map, pass number)."""
    ty, tx, _ = shape(w, h)
    cur = max(start, min(min_passes, max_passes))
    passes = np.full((ty, tx), cur, np.uint32)
    above, checks = threshold(tile_db), 0
    while True:
        _, err = frame_error_restated(compose(frame_a, passes, w, h), compose(frame_b, passes, w, h), w, h)
        checks += 1
        mask, counts = select_restated(w, h, passes, cur, err, above)
        if counts[0] == 0:
            return True, checks, passes, cur
        if cur == max_passes:
            return False, checks, passes, cur
        n = min(per_check, max_passes - cur)
        passes = advance_restated(passes, mask, n, w, h)
        cur += n


# ---- pinned by hand at 41 x 23 ---------------------------------------------------------------------------------------
W, H = 41, 23


def test_shape_and_edge_pixels_at_41_by_23():
    assert shape(W, H) == (3, 6, 2)
    px = tile_pixels(W, H)
    assert px.tolist() == [[64, 64, 64, 64, 64, 8], [64, 64, 64, 64, 64, 8], [56, 56, 56, 56, 56, 7]]
    assert int(px.sum()) == W * H
    assert tiles_of([[1, 0], [0, 1], [1, 1]], W, H).tolist() == [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1], [1, 1, 1, 1, 1, 1]]


def test_the_selection_rule_by_hand():
    whole = np.full((3, 6), 2)
    # no map: every group at the front -- 6 groups, 18 tiles
    mask, counts = select_restated(W, H, whole, 2, None, 0)
    assert mask.all() and counts == (6, 18)
    # above = 0: a group is selected as soon as one of its tiles differs at all
    err = np.zeros((3, 6), np.uint32)
    err[0, 5] = 1                                            # the 1-pixel-wide tile of the right group, bottom row
    err[2, 1] = 3
    mask, counts = select_restated(W, H, whole, 2, err, 0)
    assert mask.tolist() == [[False, True], [False, False], [True, False]] and counts == (2, 2 + 4)
    # full tiles: err > above.  Edge tiles scale: the 8-pixel tile at above = 80 needs err * 64 > 80 * 8, err > 10
    err = np.zeros((3, 6), np.uint32)
    err[1, 0], err[1, 5], err[2, 5] = 80, 10, 9                # 80 > 80 no; 10 * 64 > 640 no; 7-pixel tile: 9 * 64 = 576 > 560 yes
    mask, _ = select_restated(W, H, whole, 2, err, 80)
    assert mask.tolist() == [[False, False], [False, False], [False, True]]
    err[1, 0], err[1, 5] = 81, 11
    mask, _ = select_restated(W, H, whole, 2, err, 80)
    assert mask.tolist() == [[False, False], [True, True], [False, True]]
    # the front: a group that fell behind is not selected whatever its error
    passes = advance_restated(whole, [[1, 0], [0, 0], [0, 1]], 3, W, H)
    assert passes.tolist() == [[5, 5, 5, 5, 2, 2], [2] * 6, [2, 2, 2, 2, 5, 5]]
    mask, counts = select_restated(W, H, passes, 5, np.full((3, 6), 1000), 0)
    assert mask.tolist() == [[True, False], [False, False], [False, True]] and counts == (2, 6)
    mask, counts = select_restated(W, H, passes, 5, None, 0)
    assert counts == (2, 6)


def test_the_list_by_hand():
    mask = [[1, 0], [0, 1], [0, 1]]
    # four-wavefront instance: 2 x 3 launch tiles, the group IS the tile; grid.x stays 2, the sentinel is 6
    lst, grid = list_restated(W, H, 4, mask)
    assert lst.tolist() == [0, 3, 5, 6] and grid == (2, 2)
    lst, grid = list_restated(W, H, 4, mask, order=[5, 4, 3, 2, 1, 0])
    assert lst.tolist() == [5, 3, 0, 6] and grid == (2, 2)
    # one-wavefront instance: 6 x 3 launch tiles, a group covers up to four of them; the sentinel is 18
    lst, grid = list_restated(W, H, 1, mask)
    assert lst.tolist() == [0, 1, 2, 3, 10, 11, 16, 17, 18, 18, 18, 18] and grid == (6, 2)
    order = [17, 0, 9, 10, 1, 16, 2, 11, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15]
    lst, grid = list_restated(W, H, 1, mask, order=order)
    assert lst.tolist() == [17, 0, 10, 1, 16, 2, 11, 3, 18, 18, 18, 18] and grid == (6, 2)
    lst, grid = list_restated(W, H, 1, np.ones((3, 2), bool))
    assert lst.tolist() == list(range(18)) and grid == (6, 3)   # everything selected: the plain launch's grid, no sentinel
    lst, grid = list_restated(W, H, 4, np.zeros((3, 2), bool))
    assert lst.size == 0 and grid == (2, 0)


def test_the_merge_by_hand():
    """Three contexts over 41 x 23 with constant planes 1, 2, 4: per tile the weights are that tile's counts."""
    planes = [np.full(3 * W * H, v, np.float32) for v in (1.0, 2.0, 4.0)]
    a = np.full((3, 6), 2)
    b = advance_restated(np.zeros((3, 6)), [[1, 0], [0, 0], [0, 0]], 6, W, H)     # holds passes in the bottom-left group only
    c = np.zeros((3, 6), np.int64)
    c[2, 5] = 1                                              # ... and the 1 x 7 pixel corner tile only
    out, counts = merge_tiles_restated(planes, [a, b, c], W, H)
    assert counts.tolist() == [[8, 8, 8, 8, 2, 2], [2] * 6, [2, 2, 2, 2, 2, 3]]
    img = out.reshape(H, W, 3)[::-1]                         # row 0 = bottom, as the tile map
    f = np.float32
    assert np.all(img[:8, :32] == (f(1) * f(2) + f(2) * f(6)) * (f(1) / f(8)))        # 14 / 8
    assert np.all(img[8:16] == f(2) * (f(1) / f(2))) and np.all(img[:8, 32:] == f(1))
    assert np.all(img[16:, 40:] == (f(2) + f(4)) * (f(1) / f(3)))                      # the corner tile: (1 * 2 + 4 * 1) / 3
    assert np.all(img[16:, :40] == f(1))
    # a tile nobody holds a pass of keeps dst's floats; dst at 0 passes elsewhere is skipped, not weighted by zero
    out, counts = merge_tiles_restated([planes[0], planes[2]], [np.zeros((3, 6)), c], W, H)
    img = out.reshape(H, W, 3)[::-1]
    assert np.all(img[16:, 40:] == f(4)) and np.all(img[:16] == f(1)) and np.all(img[16:, :40] == f(1))
    assert counts.tolist() == c.tolist()
    # whole contexts: the per-tile restatement is the whole-frame one
    rng = np.random.default_rng(5)
    planes = [rng.random(3 * W * H, dtype=np.float32) for _ in range(3)]
    out, _ = merge_tiles_restated(planes, [np.full((3, 6), n) for n in (3, 5, 2)], W, H)
    acc = planes[0] * f(3)
    acc = (acc + planes[1] * f(5)).astype(f)
    acc = (acc + planes[2] * f(2)).astype(f)
    assert np.array_equal(out, acc * (f(1) / f(10)))


def test_the_threshold_formula():
    assert threshold(0.0) == 255 * 255 * 192                 # PSNR 0 dB: the largest error a tile can hold (64 * 3 * 255^2)
    assert threshold(10.0) == 1248480 and threshold(20.0) == 124848 and threshold(30.0) == 12484 and threshold(40.0) == 1248
    assert threshold(200.0) == 0 and threshold(-200.0) == 2 ** 32 - 1
    # a full tile exactly at the target is not selected, one unit above is
    whole = np.full((3, 6), 4)
    for err, want in ((1248, 0), (1249, 1)):
        e = np.zeros((3, 6), np.uint32)
        e[1, 1] = err
        assert select_restated(W, H, whole, 4, e, threshold(40.0))[1][0] == want


def test_the_driver_restated_on_made_up_frames():
    """Two 'streams' whose frames differ in the left group of the bottom row until 12 passes and nowhere else: that group renders on, the
    others retire at the first check."""
    def frame(stream):
        def at(p):
            f = np.zeros((H, W), np.uint32)
            if stream == 1 and p < 12:
                f[0, 0] = 200
            return f.reshape(-1)
        return at
    reached, checks, passes, cur = adaptive_restated(frame(0), frame(1), W, H, 40.0, 4, 4, 24)
    assert reached and checks == 3 and cur == 12
    assert passes.tolist() == [[12, 12, 12, 12, 4, 4], [4] * 6, [4] * 6]
    reached, checks, passes, cur = adaptive_restated(frame(0), frame(1), W, H, 40.0, 4, 4, 8)
    assert not reached and checks == 2 and cur == 8 and passes[0, 0] == 8


# ---- the library, without a device ----------------------------------------------------------------------------------------
def test_the_symbols_and_bindings_exist():
    from raytracing_simple_amd import _build
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    lib = api.load_library()
    for name in SYMBOLS:
        assert name in api.SYMBOLS
        assert callable(getattr(lib, name))
    for name in ("tile_passes", "select_tiles", "render_tiles_async", "render_adaptive"):
        assert callable(getattr(api.RtContext, name))


def test_argument_checks_need_no_device():
    lib = api.load_library()
    err, n = api.FrameError(), C.c_int()
    buf, counts = (C.c_uint32 * 4)(), (C.c_uint32 * 2)()
    other = C.c_void_p(8)                                    # never dereferenced: the null context is refused first
    for rc in (lib.rt_tile_passes(None, buf),
               lib.rt_select_tiles(None, None, 0, None, counts),
               lib.rt_render_tiles_async(None, 1, None),
               lib.rt_render_adaptive(None, other, 40.0, 4, 4, 8, C.byref(err), C.byref(n)),
               lib.rt_render_adaptive(other, None, 40.0, 4, 4, 8, C.byref(err), None)):
        assert rc == -1                                      # RT_ERR_ARG
        assert b"null" in lib.rt_last_error()
