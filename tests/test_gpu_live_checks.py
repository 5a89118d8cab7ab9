"""Cross-filtering only the groups still rendering (include/rt_api.h rt_denoise_pair_tiles_async, rt_render_adaptive_filtered_tiles; csrc/rt_denoise.hip,
csrc/rt_compare.hip) on the device.  The reference is rt_denoise_pair_planes on the colour planes read back (tests/test_denoise_pair_cpu.py holds it to
a numpy restatement of the rules): a pixel of a selected group holds its value, every other pixel the bits it held before.  The packed planes cannot be
read back; they are held to the same expectation through rt_compare_filtered's exact integer metric and tile map, as in tests/test_gpu_denoise_pair.py.
Every comparison is of bits or of exact integers."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

import test_tiles_cpu as T
from raytracing_simple_amd import api
from test_denoise_cpu import PARAMS, assert_same_bits
from test_gpu_denoise_pair import metric_of, stale, two_streams
from test_gpu_state import RT_ERR_STATE, _refused, assert_unchanged, bits, make, snapshot
from test_gpu_tiles import dev_map, select

pytestmark = pytest.mark.gpu

DB, MIN_PASSES, PER_CHECK, MAX_PASSES = 28.0, 4, 4, 32      # test 4's arguments (the issue's), shared with test 5


def three_groups(w, h):
    """[tiles_y, groups_x], row 0 = bottom: the top-right group (partial at both edges at the sizes used), a bottom-left group, a middle one."""
    ty, _, gx = T.shape(w, h)
    mask = np.zeros((ty, gx), bool)
    mask[ty - 1, gx - 1] = mask[0, 0] = mask[ty // 2, gx // 2] = True
    assert mask.sum() == 3
    return mask


def pixels_of(mask, w, h):
    """A group mask as a pixel mask of the PLANE's layout [h, w] (row 0 = top: the pixel buffer's rows flipped)."""
    return np.repeat(np.repeat(np.asarray(mask, bool), 8, axis=0), 32, axis=1)[:h, :w][::-1]


def rendered_pair(w, h, passes, modes=None):
    a, b = two_streams(w, h)
    if modes:
        a.set_mode(modes[0])
        b.set_mode(modes[1])
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
    a.render_async(passes, a.stream)
    b.render_async(passes, b.stream)
    return a, b


def expected_planes(a, b, params, before, mask):
    """What the tiles call must leave: rt_denoise_pair_planes of the colour planes as they are now inside the groups of `mask`, `before` elsewhere."""
    w, h = a.w, a.h
    fresh = api.denoise_pair_planes(a.read_colors(), b.read_colors(), w, h, params)
    m = pixels_of(mask, w, h)
    out = []
    for new, old in zip(fresh, before):
        x = old.reshape(h, w, 3).copy()
        x[m] = new.reshape(h, w, 3)[m]
        out.append(x.reshape(-1))
    return out, m


# ---- 1. a refresh equals the host, and touches nothing else ---------------------------------------------------------------------------
CASES = PARAMS + [{"search_radius": 0}]


@pytest.mark.parametrize("w,h", [(41, 23), (70, 19)])
def test_a_refresh_forms_the_selected_groups_from_the_current_colours_and_keeps_every_other_word(w, h):
    mask = three_groups(w, h)
    for params in CASES:
        a, b = rendered_pair(w, h, 3)
        with a, b:
            a.denoise_pair(b, params)
            before = a.read_filtered().copy(), b.read_filtered().copy()
            assert select(a, mask) == select(b, mask) == (3, int(T.tiles_of(mask, w, h).sum()))
            a.render_tiles_async(2, a.stream)
            b.render_tiles_async(2, b.stream)
            stale(a, b)
            snaps = snapshot(a), snapshot(b)
            a.denoise_pair_tiles(b, params)
            want, m = expected_planes(a, b, params, before, mask)
            got = a.read_filtered(), b.read_filtered()
            for g, x, old in zip(got, want, before):
                assert_same_bits(g, x)
                assert np.array_equal(bits(g).reshape(h, w, 3)[~m], bits(old).reshape(h, w, 3)[~m])      # nothing else was touched
                if params["search_radius"] > 0:
                    assert not np.array_equal(bits(g).reshape(h, w, 3)[m], bits(old).reshape(h, w, 3)[m])  # (the two passes moved the selected groups)
            err, tiles = a.compare_filtered(b, tiles=True)
            want_err, want_tiles = metric_of(want[0], want[1], w, h)
            assert err == want_err and np.array_equal(tiles, want_tiles), params
            for c, s in zip((a, b), snaps):                   # colours, seeds and pass numbers stay
                assert_unchanged(c, s)
            assert np.array_equal(a.tile_passes(), b.tile_passes()) and sorted(np.unique(a.tile_passes()).tolist()) == [3, 5]


def test_a_fast_context_packs_its_refreshed_groups_with_fast_modes_to_int():
    """One half in fast mode: the words beside its plane are what the pack kernel of that mode makes of the plane -- the expected planes written into
    two contexts of the same modes and compared as frames give the same sums and the same map."""
    w, h = 41, 23
    mask = three_groups(w, h)
    modes = (api.RT_MODE_FAST, api.RT_MODE_PARITY)
    a, b = rendered_pair(w, h, 3, modes)
    with a, b, make("demo", w, h) as c, make("demo", w, h) as d:
        c.set_mode(modes[0])
        d.set_mode(modes[1])
        a.denoise_pair(b)
        before = a.read_filtered().copy(), b.read_filtered().copy()
        select(a, mask)
        select(b, mask)
        a.render_tiles_async(2, a.stream)
        b.render_tiles_async(2, b.stream)
        a.denoise_pair_tiles(b)
        want, _ = expected_planes(a, b, None, before, mask)
        assert_same_bits(a.read_filtered(), want[0])
        assert_same_bits(b.read_filtered(), want[1])
        c.write_state(want[0], None, 5)
        d.write_state(want[1], None, 5)
        got, got_tiles = a.compare_filtered(b, tiles=True)
        ref, ref_tiles = c.compare(d, tiles=True)
        assert got == ref and np.array_equal(got_tiles, ref_tiles)


def test_a_list_of_groups_longer_than_a_chunk_names_the_groups_either_side_of_the_boundary():
    """523x521: 17 x 66 = 1122 groups, two chunks of the one-workgroup compaction.  Groups (60, 3) and (60, 4) are indices 1023 and 1024 -- the last
    entry of the first chunk and the first of the second, so the second's place in the list is the running base the first chunk leaves -- beside
    (0, 0) and the top-right group (65, 16), which is one pixel high (its origin in the plane is negative) and eleven wide."""
    w, h = 523, 521
    params = PARAMS[2]
    assert params == {"search_radius": 1, "patch_radius": 0}
    ty, _, gx = T.shape(w, h)
    assert (ty, gx) == (66, 17) and 60 * gx + 3 == 1023
    mask = np.zeros((ty, gx), bool)
    mask[60, 3] = mask[60, 4] = mask[0, 0] = mask[65, 16] = True
    a, b = rendered_pair(w, h, 3)
    with a, b:
        a.denoise_pair(b, params)
        before = a.read_filtered().copy(), b.read_filtered().copy()
        assert select(a, mask) == select(b, mask) == (4, int(T.tiles_of(mask, w, h).sum()))
        a.render_tiles_async(2, a.stream)
        b.render_tiles_async(2, b.stream)
        a.denoise_pair_tiles(b, params)
        want, m = expected_planes(a, b, params, before, mask)
        for g, x, old in zip((a.read_filtered(), b.read_filtered()), want, before):
            assert_same_bits(g, x)
            assert np.array_equal(bits(g).reshape(h, w, 3)[~m], bits(old).reshape(h, w, 3)[~m])      # every other word is the one from before
        err, tiles = a.compare_filtered(b, tiles=True)
        want_err, want_tiles = metric_of(want[0], want[1], w, h)
        assert err == want_err and np.array_equal(tiles, want_tiles)


# ---- 2. every group selected equals rt_denoise_pair_async -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(41, 23), (96, 64)])
def test_with_every_group_selected_the_refresh_is_the_whole_frame_call(w, h):
    ty, _, gx = T.shape(w, h)
    a, b = rendered_pair(w, h, 3)
    with a, b:
        a.denoise_pair(b)
        old = bits(a.read_filtered()).copy()
        assert select(a, np.ones((ty, gx), bool))[0] == select(b, np.ones((ty, gx), bool))[0] == ty * gx
        a.render_tiles_async(2, a.stream)
        b.render_tiles_async(2, b.stream)
        a.denoise_pair_tiles(b)
        tiles_call = bits(a.read_filtered()).copy(), bits(b.read_filtered()).copy(), a.compare_filtered(b, tiles=True)
        assert not np.array_equal(tiles_call[0], old)
        a.denoise_pair(b)
        whole = bits(a.read_filtered()), bits(b.read_filtered()), a.compare_filtered(b, tiles=True)
        assert np.array_equal(tiles_call[0], whole[0]) and np.array_equal(tiles_call[1], whole[1])
        assert tiles_call[2][0] == whole[2][0] and np.array_equal(tiles_call[2][1], whole[2][1])      # the packed planes, through the metric and the map


# ---- 3. refusals and state --------------------------------------------------------------------------------------------------------------
def test_what_is_not_one_selection_behind_is_refused_and_nothing_changes():
    w, h = 41, 23
    mask = three_groups(w, h)
    two = mask.copy()
    two[0, 0] = False

    def refused(a, b):
        snaps = snapshot(a), snapshot(b)
        passes = a.tile_passes().copy(), b.tile_passes().copy()
        _refused(a, RT_ERR_STATE, a.denoise_pair_tiles, b)
        for c, s, p in zip((a, b), snaps, passes):
            assert_unchanged(c, s)
            assert np.array_equal(c.tile_passes(), p)

    def readable(a, b):
        return bits(a.read_filtered()).copy(), bits(b.read_filtered()).copy(), a.compare_filtered(b)

    def same(x, y):
        return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]

    def fresh(pair=True):
        a, b = rendered_pair(w, h, 3)
        if pair:
            a.denoise_pair(b)
        return a, b

    def launch(*ctxs):
        for c in ctxs:
            c.render_tiles_async(2, c.stream)

    # no selection: the planes are current and stay so
    a, b = fresh()
    with a, b:
        before = readable(a, b)
        refused(a, b)
        select(a, mask)                                       # ... on one context only
        refused(a, b)
        refused(b, a)
        # selections of different counts
        select(b, two)
        refused(a, b)
        assert same(readable(a, b), before)
        # the planes current and equal selections: RT_OK, nothing launched, nothing changed
        select(b, mask)
        a.denoise_pair_tiles(b)
        assert same(readable(a, b), before)
        # only one context subset-launched (its pass number has moved on): the other's plane is still what it was
        launch(a)
        refused(a, b)
        assert np.array_equal(bits(b.read_filtered()), before[1])
    # planes never made
    a, b = fresh(pair=False)
    with a, b:
        select(a, mask), select(b, mask)
        refused(a, b)
        launch(a, b)
        refused(a, b)
        stale(a, b)
    # a whole-frame launch in between (every group selected keeps the frame whole, so that rt_render_async is accepted)
    a, b = fresh()
    with a, b:
        every = np.ones_like(mask)
        select(a, every), select(b, every)
        launch(a, b)
        a.render_async(1, a.stream)
        b.render_async(1, b.stream)
        refused(a, b)
        stale(a, b)
    # a new selection in between
    a, b = fresh()
    with a, b:
        select(a, mask), select(b, mask)
        launch(a, b)
        select(a, mask), select(b, mask)                      # (the same groups: they are the front)
        refused(a, b)
        stale(a, b)
    # a written state in between (it drops the selection too: a selects again, and is still not refreshable)
    a, b = fresh()
    with a, b:
        select(a, mask), select(b, mask)
        launch(a, b)
        a.write_state(a.read_colors(), a.read_seeds(), a.current_sample)
        refused(a, b)
        assert select(a, mask) == (3, int(T.tiles_of(mask, w, h).sum()))
        refused(a, b)
        stale(a, b)
    # rt_denoise_async into one context in between: a holds 4 + 2 passes and passes for the merge of c and d at 3 each
    a, b = rendered_pair(w, h, 4)
    with a, b, make("demo", w, h) as c, make("demo", w, h) as d:
        a.denoise_pair(b)
        select(a, mask), select(b, mask)
        launch(a, b)
        for x in (c, d):
            x.write_state(np.zeros(3 * w * h, np.float32), None, 3)
        a.denoise(c, d)                                       # accepted, and it moves a's colour plane
        refused(a, b)
        stale(a, b)
        # ... and the whole-frame call brings the planes back
        a.denoise_pair(b)
        assert a.compare_filtered(b)["pixels"] == w * h


def test_two_subset_launches_of_one_selection_are_refreshed_by_one_call():
    w, h = 41, 23
    mask = three_groups(w, h)
    a, b = rendered_pair(w, h, 3)
    with a, b:
        a.denoise_pair(b)
        before = a.read_filtered().copy(), b.read_filtered().copy()
        select(a, mask), select(b, mask)
        for n in (1, 2):
            a.render_tiles_async(n, a.stream)
            b.render_tiles_async(n, b.stream)
        a.denoise_pair_tiles(b)
        want, _ = expected_planes(a, b, None, before, mask)
        assert_same_bits(a.read_filtered(), want[0])
        assert_same_bits(b.read_filtered(), want[1])
        # current again: a second call has nothing to do, and a further launch of the same selection is refreshed in turn
        a.denoise_pair_tiles(b)
        assert_same_bits(a.read_filtered(), want[0])
        a.render_tiles_async(1, a.stream)
        b.render_tiles_async(1, b.stream)
        a.denoise_pair_tiles(b)
        again, _ = expected_planes(a, b, None, want, mask)
        assert_same_bits(a.read_filtered(), again[0])
        assert_same_bits(b.read_filtered(), again[1])


# ---- 4. the two loops agree -------------------------------------------------------------------------------------------------------------
def state_of(c):
    return c.tile_passes().copy(), bits(c.read_colors()).copy(), c.read_seeds().copy(), c.read_pixels().copy(), c.stats()


@pytest.fixture(scope="module")
def whole_loop():
    """rt_render_adaptive_filtered on Demo 96x64: what it returns and leaves, computed once and left unchanged."""
    a, b = two_streams(96, 64)
    with a, b:
        out = a.render_adaptive_filtered(b, DB, MIN_PASSES, PER_CHECK, MAX_PASSES)
        return out, state_of(a), state_of(b)


@pytest.fixture(scope="module")
def live_loop():
    a, b = two_streams(96, 64)
    with a, b:
        out = a.render_adaptive_filtered_tiles(b, DB, MIN_PASSES, PER_CHECK, MAX_PASSES)
        planes_current = a.compare_filtered(b) == out[1]
        return out, state_of(a), state_of(b), planes_current


def assert_same_state(got, want):
    for g, x in zip(got, want):
        assert np.array_equal(g, x) if isinstance(x, np.ndarray) else g == x


def test_the_loop_with_live_checks_renders_what_the_whole_frame_loop_renders(whole_loop, live_loop):
    """Demo 96x64, seed streams 1 and 2, the defaults, 28 dB per tile, 4 passes at least, 4 per check, 32 at most.  The test shows something only if a
    group had retired before the last check and one was selected at the second: by the pass map, tiles hold fewer passes than the front (retired
    early) and tiles hold more than 8 (selected at the second check or later).  The CPU prototype has 12 of 24 groups live at the first check and 6 at
    32 passes; the device has 12, 10, 8, 7, 6, 5, 5, 5 live groups at its eight checks, so the issue's target stands."""
    (reached, last, checks), sa, sb = whole_loop
    (reached_l, last_l, checks_l), la, lb, planes_current = live_loop
    passes = sa[0]
    assert np.array_equal(passes, sb[0])
    assert (passes < passes.max()).any()                      # some group had retired before the last check
    assert (passes > MIN_PASSES + PER_CHECK).any() and checks >= 3             # ... and some group was selected at the second check
    assert (reached_l, checks_l) == (reached, checks)
    assert_same_state(la, sa)
    assert_same_state(lb, sb)
    assert planes_current                                     # the last check's planes are current, as after the whole-frame loop
    assert last_l["pixels"] == last["pixels"] == 96 * 64


# ---- 5. the loop is its public calls ----------------------------------------------------------------------------------------------------
def test_the_loop_is_its_public_calls(live_loop):
    (reached, last, checks), la, _, _ = live_loop
    above = T.threshold(DB)
    a, b = two_streams(96, 64)
    with a, b:
        a.render_async(MIN_PASSES, a.stream)
        b.render_async(MIN_PASSES, b.stream)
        a.denoise_pair(b, None, a.stream)
        done, live = 0, []
        while True:
            err, tiles = a.compare_filtered(b, tiles=True)
            d = dev_map(tiles)
            ca, cb = a.select_tiles(d.ptr, above, a.stream), b.select_tiles(d.ptr, above, b.stream)
            d.close()
            done += 1
            assert ca == cb
            live.append(ca[0])
            if ca[0] == 0:
                got = True
                break
            n = min(PER_CHECK, MAX_PASSES - a.current_sample)
            if n == 0:
                got = False
                break
            a.render_tiles_async(n, a.stream)
            b.render_tiles_async(n, b.stream)
            a.denoise_pair_tiles(b, None, a.stream)
        print("\n[live checks] Demo 96x64, %g dB: live groups per check %s of 24" % (DB, live))
        assert (got, done) == (reached, checks)
        assert err == last                                    # every field of the 48 bytes
        assert np.array_equal(a.tile_passes(), la[0]) and np.array_equal(b.tile_passes(), la[0])
        assert live[0] > live[-1] and live[1] > 0
