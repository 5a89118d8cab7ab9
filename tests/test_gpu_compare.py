"""Frame error on the device (include/rt_api.h "frame error on the device", csrc/rt_compare.hip).  The metric is exact integer arithmetic,
so every comparison is `==` against test_compare_cpu.frame_error_restated: first over synthetic buffers (torch tensors the contexts are
pointed at with set_pixel_buffer; nothing is rendered), then over frames whose pixels the CPU oracle gives (tests/_oracle.py render)."""
import math

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api
from test_compare_cpu import frame_error_restated, random_frames
from test_gpu_state import H, RT_ERR_ARG, RT_ERR_STATE, W, _refused, assert_counters, assert_state, assert_unchanged, make, oracle, snapshot

pytestmark = pytest.mark.gpu


def on_device(words, rows, w):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).reshape(rows, w).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


class Pair:
    """Two pass-0 contexts of one size whose pixel buffers are caller-owned torch tensors of exactly rows * w words."""

    def __init__(self, w, h, **kw):
        self.w, self.h = w, h
        self.a, self.b = api.RtContext(w, h, **kw), api.RtContext(w, h, **kw)
        self.keep = []

    def point_at(self, a_words, b_words):
        rows = self.a.local_rows
        ta, tb = on_device(a_words, rows, self.w), on_device(b_words, rows, self.w)
        self.a.set_pixel_buffer(ta.data_ptr(), ta.numel())
        self.b.set_pixel_buffer(tb.data_ptr(), tb.numel())
        self.keep = [ta, tb]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.a.close()
        self.b.close()


def assert_compare_equals(a, b, want_err, want_tiles):
    err, tiles = a.compare(b, tiles=True)
    assert err == want_err
    assert tiles.shape == want_tiles.shape == a.compare_tiles() and np.array_equal(tiles, want_tiles)
    assert a.compare(b) == want_err                          # without the map; and a second call equals the first
    again, tiles2 = a.compare(b, tiles=True)
    assert again == want_err and np.array_equal(tiles2, want_tiles)
    assert api.error_psnr(err) == api.error_psnr(want_err)


# ---- 1. synthetic buffers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (41, 23), (523, 9)],
                         ids=["one-pixel", "one-full-tile", "partial-tiles-unaligned-rows", "wider-than-a-workgroups-run"])
def test_synthetic_frames_equal_the_restatement(w, h):
    with Pair(w, h) as p:
        a, b = random_frames(w, h, 1000 * w + h)
        p.point_at(a, b)
        assert_compare_equals(p.a, p.b, *frame_error_restated(a, b, w, h))
        swapped, _ = p.b.compare(p.a, tiles=True)             # the metric is symmetric
        assert swapped == frame_error_restated(a, b, w, h)[0]
        # the extremes of every field: all channels 255 apart, and frames that differ in the ignored top byte only
        lo, hi = np.full(w * h, 0xFF000000, np.uint32), np.full(w * h, 0x00FFFFFF, np.uint32)
        p.point_at(hi, lo)
        want, tiles = frame_error_restated(hi, lo, w, h)
        assert want["sq_err"] == [w * h * 255 * 255] * 3 and want["differing"] == w * h and want["max_abs"] == 255
        assert_compare_equals(p.a, p.b, want, tiles)
        p.point_at(a, a | np.uint32(0xAB000000))
        assert_compare_equals(p.a, p.b, {"sq_err": [0, 0, 0], "differing": 0, "pixels": w * h, "max_abs": 0, "reserved": 0},
                              np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32))
        # one pixel differs, in one channel, by one: the last pixel of the last (partial) row
        c = a.copy()
        c[-1] ^= np.uint32(0x00000100)
        p.point_at(a, c)
        want, tiles = frame_error_restated(a, c, w, h)
        assert want["sq_err"] == [0, 1, 0] and want["differing"] == 1 and want["max_abs"] == 1 and tiles[-1, -1] == 1 and tiles.sum() == 1
        assert_compare_equals(p.a, p.b, want, tiles)


def test_a_full_size_frame_needs_the_64_bit_sums():
    w, h = 1920, 1080
    with Pair(w, h) as p:
        hi, lo = np.full(w * h, 0x00FFFFFF, np.uint32), np.full(w * h, 0xFF000000, np.uint32)
        p.point_at(hi, lo)
        err, tiles = p.a.compare(p.b, tiles=True)
        assert 134_835_840_000 == w * h * 255 * 255 > 2 ** 32
        assert err == {"sq_err": [134_835_840_000] * 3, "differing": w * h, "pixels": w * h, "max_abs": 255, "reserved": 0}
        assert tiles.shape == (135, 240) and np.all(tiles == 12_484_800)          # every tile is a full one at this size
        assert p.a.compare(p.b) == err                        # a second call equals the first
        assert api.error_psnr(err) == 0.0
        words, _ = random_frames(w, h, 5)
        p.point_at(words, words | np.uint32(0xAB000000))
        err, tiles = p.a.compare(p.b, tiles=True)
        assert err == {"sq_err": [0, 0, 0], "differing": 0, "pixels": w * h, "max_abs": 0, "reserved": 0} and not tiles.any()
        assert api.error_psnr(err) == math.inf
        other, _ = random_frames(w, h, 6)                     # ... and random words: several strips per workgroup (the grid is capped)
        p.point_at(words, other)
        assert_compare_equals(p.a, p.b, *frame_error_restated(words, other, w, h))


# ---- 2. asynchronous, into the caller's device memory, on the caller's stream -------------------------------------
def test_compare_async_writes_the_callers_tensors_on_the_callers_stream():
    import torch
    w, h = 523, 9
    with Pair(w, h) as p:
        a, b = random_frames(w, h, 77)
        p.point_at(a, b)
        want, want_tiles = p.a.compare(p.b, tiles=True)
        assert (want, want_tiles.tolist()) == (frame_error_restated(a, b, w, h)[0], frame_error_restated(a, b, w, h)[1].tolist())
        stream = torch.cuda.Stream()
        for with_tiles in (True, False, True):
            res = torch.full((12,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")       # the call clears its accumulators itself
            tiles = torch.full(want_tiles.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            p.a.compare_async(p.b, res.data_ptr(), tiles.data_ptr() if with_tiles else None, stream.cuda_stream)
            p.a.compare_async(p.b, res.data_ptr(), tiles.data_ptr() if with_tiles else None, stream.cuda_stream)     # twice in a row: the same answer
            stream.synchronize()
            got = api.FrameError.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
            assert got == want
            got_tiles = tiles.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_tiles, want_tiles) if with_tiles else np.all(got_tiles == 0x5A5A5A5A)
        p.a.compare_async(p.b, res.data_ptr())                # the null stream
        torch.cuda.synchronize()
        assert api.FrameError.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict() == want


# ---- 3. rendered frames: the oracle's pixels, and nothing else of the contexts changes ---------------------------
def two_streams(n, **kw):
    a, b = make("demo", **kw), make("demo", **kw)
    a.seed_stream(1, a.stream)
    b.seed_stream(2, b.stream)
    if n:
        a.render_async(n, a.stream)
        b.render_async(n, b.stream)
    return a, b


def oracle_error(n_a, stream_a, n_b, stream_b, rows=None):
    pa, pb = oracle("demo", W, H, n_a, stream_a)["pixels"].reshape(H, W), oracle("demo", W, H, n_b, stream_b)["pixels"].reshape(H, W)
    rows = np.arange(H) if rows is None else rows
    return frame_error_restated(pa[rows], pb[rows], W, len(rows))


def test_rendered_frames_equal_the_oracles_and_the_contexts_stay_as_they_were():
    a, b = make("demo"), make("demo")
    with a, b:
        a.seed_stream(1, a.stream)
        b.seed_stream(2, b.stream)
        b.set_pixel_write(0)                                 # b's frame exists in the colour plane only: the pack kernel runs
        a.render_async(3, a.stream)
        b.render_async(3, b.stream)
        kernels = (a.last_kernel, b.last_kernel)
        want, want_tiles = oracle_error(3, 1, 3, 2)
        assert want["differing"] > 0                         # two streams, two frames
        err, tiles = a.compare(b, tiles=True)
        assert err == want and np.array_equal(tiles, want_tiles)
        assert a.compare(b) == want and b.compare(a) == want
        assert (a.last_kernel, b.last_kernel) == kernels and a.current_sample == b.current_sample == 3
        for ctx, k in ((a, 1), (b, 2)):
            assert_state(ctx, oracle("demo", W, H, 3, k))
            assert_counters(ctx, oracle("demo", W, H, 3, k))
            assert ctx.stats()["launches"] == 1
        b.set_pixel_write(1)
        for ctx, k in ((a, 1), (b, 2)):                      # one more pass continues bit for bit
            px = ctx.render_pass(1)
            assert ctx.current_sample == 4
            assert_state(ctx, oracle("demo", W, H, 4, k), px)
        assert a.compare(b) == oracle_error(4, 1, 4, 2)[0]
        a.render_pass(2)                                     # pass numbers may differ
        assert a.compare(b) == oracle_error(6, 1, 4, 2)[0]


# ---- 4. fast against parity: the gate's use ----------------------------------------------------------------------
def test_fast_mode_against_parity_mode_equals_the_restatement_over_read_pixels():
    with make("demo") as a, make("demo") as b:
        b.set_mode(api.RT_MODE_FAST)
        a.render_async(3, a.stream)
        b.render_async(3, b.stream)
        err, tiles = a.compare(b, tiles=True)
        pa, pb = a.read_pixels(), b.read_pixels()
        assert np.array_equal(pa, oracle("demo", W, H, 3)["pixels"])
        want, want_tiles = frame_error_restated(pa, pb, W, H)
        assert err == want and np.array_equal(tiles, want_tiles)
        assert abs(api.error_psnr(err) - O.psnr(pa, pb)) <= 1e-9


# ---- 5. sharded pairs --------------------------------------------------------------------------------------------
def test_sharded_pairs_compare_their_rows_and_add_up_to_the_whole():
    total = {"sq_err": [0, 0, 0], "differing": 0, "pixels": 0, "max_abs": 0, "reserved": 0}
    for rank in range(3):
        a, b = two_streams(3, rank=rank, nranks=3, tile_rows=8)
        with a, b:
            rows = a.local_row_map()
            assert len(rows) == (8, 8, 7)[rank]
            want, want_tiles = oracle_error(3, 1, 3, 2, rows)
            err, tiles = a.compare(b, tiles=True)
            assert err == want and np.array_equal(tiles, want_tiles)
        for k in range(3):
            total["sq_err"][k] += err["sq_err"][k]
        total["differing"] += err["differing"]
        total["pixels"] += err["pixels"]
        total["max_abs"] = max(total["max_abs"], err["max_abs"])
    assert total == oracle_error(3, 1, 3, 2)[0]
    a, b = two_streams(3)
    with a, b:
        assert a.compare(b) == total


def test_a_rank_without_rows_yields_zeros():
    a, b = two_streams(2, rank=3, nranks=4, tile_rows=8)      # three row tiles, four ranks
    with a, b:
        assert a.local_rows == 0 and a.compare_tiles() == (0, 6)
        err, tiles = a.compare(b, tiles=True)
        assert err == {"sq_err": [0, 0, 0], "differing": 0, "pixels": 0, "max_abs": 0, "reserved": 0} and tiles.size == 0
        assert api.error_psnr(err) == math.inf


# ---- 6. refusals -------------------------------------------------------------------------------------------------
def test_refused_pairs_leave_the_contexts_as_they_were():
    import torch
    a, b = two_streams(3)
    with a, b, make("demo", W + 1, H) as wider, make("demo", rank=1, nranks=3) as shard, make("demo", devices=[0, 0]) as multi:
        multi.render_pass(2)
        snaps = [snapshot(c) for c in (a, b, multi)]
        lib = api.load_library()
        res = torch.zeros(12, dtype=torch.int32, device="cuda")
        for x, y in ((a, wider), (wider, a), (a, shard), (shard, a), (a, multi), (multi, a), (a, a)):
            _refused(x, RT_ERR_ARG, x.compare, y)
            _refused(x, RT_ERR_ARG, x.compare_async, y, res.data_ptr())
            _refused(x, RT_ERR_ARG, x.render_converged, y, 30.0, 1, 8)
        assert "multi-device" in _refused(a, RT_ERR_ARG, a.compare, multi) and "multi-device" in _refused(multi, RT_ERR_ARG, multi.compare, a)
        assert "itself" in _refused(a, RT_ERR_ARG, a.compare, a)
        assert "null" in _refused(a, RT_ERR_ARG, a.compare_async, b, None)                         # a null result
        assert lib.rt_compare(a._h, b._h, None, None) == RT_ERR_ARG and b"null" in lib.rt_last_error()
        assert lib.rt_render_converged(a._h, b._h, 30.0, 1, 8, None, None) == RT_ERR_ARG and b"null" in lib.rt_last_error()
        assert "null" in _refused(a, RT_ERR_ARG, a.compare, None)
        _refused(multi, RT_ERR_ARG, multi.compare_tiles)
        if torch.cuda.device_count() >= 2:                    # (a one-GPU machine cannot make this case)
            with make("demo", device=1) as elsewhere:
                assert "device" in _refused(a, RT_ERR_ARG, a.compare, elsewhere)
        torch.cuda.synchronize()
        assert not res.cpu().numpy().any()                    # nothing was written
        for c, s in zip((a, b, multi), snaps):
            assert_unchanged(c, s)
        assert a.stats()["launches"] == 1 and b.stats()["launches"] == 1
        for ctx, k in ((a, 1), (b, 2)):                       # what was refused left nothing half done
            assert_state(ctx, oracle("demo", W, H, 4, k), ctx.render_pass(1))


# ---- 7. rt_render_converged --------------------------------------------------------------------------------------
def test_render_converged_stops_at_the_first_check_that_reaches_the_target():
    # the pair's PSNR after 2, 4, 6, 8 passes, from the oracle's pixels alone (rt_error_psnr is host arithmetic on the restated sums; it is held
    # to host.psnr by test_compare_cpu) -- the very double the library compares with the target, so a target taken from it is met exactly
    passes = (2, 4, 6, 8)
    errs = [oracle_error(n, 1, n, 2)[0] for n in passes]
    psnr = [api.error_psnr(e) for e in errs]
    target = psnr[2]
    assert psnr[0] < target and math.isfinite(target), psnr   # the test's own precondition: the first check must not already pass
    stop = next(k for k, v in enumerate(psnr) if v >= target)
    a, b = two_streams(0)
    with a, b:
        reached, last, checks = a.render_converged(b, target, 2, 8)
        assert reached is True and checks == stop + 1 and last == errs[stop]
        assert a.current_sample == b.current_sample == passes[stop]
        for ctx, k in ((a, 1), (b, 2)):
            assert_state(ctx, oracle("demo", W, H, passes[stop], k))
            assert_counters(ctx, oracle("demo", W, H, passes[stop], k))
        # no pass left to render: one check of the frames as they are
        assert a.render_converged(b, target, 2, passes[stop]) == (True, errs[stop], 1)
        assert a.render_converged(b, math.inf, 5, passes[stop]) == (False, errs[stop], 1)
        assert a.current_sample == b.current_sample == passes[stop]
    a, b = two_streams(0)
    with a, b:                                               # a target nothing reaches: max_passes ends it
        assert a.render_converged(b, math.inf, 2, 4) == (False, errs[1], 2)
        assert a.current_sample == b.current_sample == 4
        for ctx, k in ((a, 1), (b, 2)):
            assert_state(ctx, oracle("demo", W, H, 4, k))
        # 3 passes per check up to 8: checks at 7 and 8 (the last step is shorter)
        assert a.render_converged(b, math.inf, 3, 8) == (False, errs[3], 2)
        assert a.current_sample == b.current_sample == 8


def test_render_converged_refusals():
    a, b = two_streams(2)
    with a, b, make("demo") as c, make("demo") as d:
        snaps = [snapshot(x) for x in (a, b, c, d)]
        _refused(a, RT_ERR_ARG, a.render_converged, b, 30.0, 0, 8)                 # passes_per_check < 1
        _refused(a, RT_ERR_ARG, a.render_converged, b, 30.0, 1, 1)                 # max_passes below the pass number
        _refused(a, RT_ERR_ARG, a.render_converged, b, math.nan, 1, 8)
        assert "default" in _refused(c, RT_ERR_STATE, c.render_converged, d, 30.0, 1, 8)          # both fresh: the default stream twice
        _refused(a, RT_ERR_STATE, a.render_converged, c, 30.0, 1, 8)               # 2 passes against 0
        for x, s in zip((a, b, c, d), snaps):
            assert_unchanged(x, s)
        c.render_pass(1)
        d.render_pass(1)
        c.reset_async(c.stream)                              # pass 0 again, by either reset: still the default stream twice
        d.reset()
        _refused(c, RT_ERR_STATE, c.render_converged, d, 30.0, 1, 8)
        c.seed_stream(0, c.stream)
        _refused(c, RT_ERR_STATE, c.render_converged, d, 30.0, 1, 8)
        c.seed_stream(3, c.stream)                           # one of them on a stream of its own: accepted
        reached, last, checks = c.render_converged(d, math.inf, 1, 1)
        assert (reached, checks) == (False, 1) and c.current_sample == d.current_sample == 1
        assert last == frame_error_restated(oracle("demo", W, H, 1, 3)["pixels"], oracle("demo", W, H, 1)["pixels"], W, H)[0]
