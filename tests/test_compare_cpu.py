"""Frame error (include/rt_api.h "frame error on the device", csrc/rt_compare.hip), the part that needs no device: the numpy restatement
of the metric that the GPU tests compare against, rt_error_psnr against host.psnr, the struct's layout and the argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

from raytracing_simple_amd import api, host

SYMBOLS = ("rt_compare_tiles", "rt_compare_async", "rt_compare", "rt_error_psnr", "rt_render_converged")


def frame_error_restated(a_pix, b_pix, w, rows):
    """include/rt_api.h rt_frame_error and its tile map, restated: exact integers over the low three bytes of the packed words.
    Returns (dict as FrameError.as_dict gives it, uint32 [ceil(rows / 8), ceil(w / 8)])."""
    a = np.ascontiguousarray(a_pix).view(np.uint32).reshape(rows, w)
    b = np.ascontiguousarray(b_pix).view(np.uint32).reshape(rows, w)
    d = np.stack([((a >> (8 * c)) & 255).astype(np.int64) - ((b >> (8 * c)) & 255).astype(np.int64) for c in range(3)])     # [3, rows, w]
    sq = d * d
    tiles_y, tiles_x = (rows + 7) // 8, (w + 7) // 8
    padded = np.zeros((tiles_y * 8, tiles_x * 8), np.int64)
    padded[:rows, :w] = sq.sum(axis=0)
    tiles = padded.reshape(tiles_y, 8, tiles_x, 8).sum(axis=(1, 3))
    assert tiles.size == 0 or tiles.max() <= 64 * 3 * 255 * 255
    err = {"sq_err": [int(sq[c].sum()) for c in range(3)], "differing": int(np.count_nonzero((a ^ b) & 0x00FFFFFF)), "pixels": rows * w,
           "max_abs": int(np.abs(d).max()) if d.size else 0, "reserved": 0}
    return err, tiles.astype(np.uint32)


def random_frames(w, rows, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2 ** 32, w * rows, dtype=np.uint64).astype(np.uint32) for _ in range(2))


def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    for name in SYMBOLS:
        assert name in api.SYMBOLS
        assert callable(getattr(lib, name))
    for name in ("compare", "compare_async", "render_converged", "compare_tiles"):
        assert callable(getattr(api.RtContext, name))
    assert callable(api.error_psnr) and callable(api.FrameError.as_dict)


def test_the_struct_is_48_bytes_in_the_documented_order():
    assert C.sizeof(api.FrameError) == 48
    offsets = {name: getattr(api.FrameError, name).offset for name, _ in api.FrameError._fields_}
    assert offsets == {"sq_err": 0, "differing": 24, "pixels": 32, "max_abs": 40, "reserved": 44}
    e = api.FrameError.from_dict({"sq_err": [1, 2 ** 40, 3], "differing": 4, "pixels": 5, "max_abs": 6})
    assert e.as_dict() == {"sq_err": [1, 2 ** 40, 3], "differing": 4, "pixels": 5, "max_abs": 6, "reserved": 0}


def test_every_entry_point_refuses_a_null_context():
    lib = api.load_library()
    err, n = api.FrameError(), C.c_int()
    other = C.c_void_p(8)                                    # never dereferenced: the null context is refused first
    for rc in (lib.rt_compare_tiles(None, None, None),
               lib.rt_compare_async(None, other, C.c_void_p(16), None, None),
               lib.rt_compare_async(other, None, C.c_void_p(16), None, None),
               lib.rt_compare(None, other, C.byref(err), None),
               lib.rt_compare(other, None, C.byref(err), None),
               lib.rt_render_converged(None, other, 40.0, 1, 8, C.byref(err), C.byref(n)),
               lib.rt_render_converged(other, None, 40.0, 1, 8, C.byref(err), None)):
        assert rc == -1                                      # RT_ERR_ARG
        assert b"null" in lib.rt_last_error()
    assert math.isnan(lib.rt_error_psnr(None)) and b"null" in lib.rt_last_error()


@pytest.mark.parametrize("w,rows", [(41, 23), (200, 120)])
def test_error_psnr_is_host_psnr_on_the_same_pixels(w, rows):
    a, b = random_frames(w, rows, 7 * w + rows)
    err, _ = frame_error_restated(a, b, w, rows)
    got, want = api.error_psnr(err), host.psnr(a, b)
    assert math.isfinite(got) and abs(got - want) <= 1e-9    # two binary64 evaluations of one formula
    # a frame of small differences: a PSNR of the size the project quotes
    c = a ^ (np.random.default_rng(3).integers(0, 2, a.size, dtype=np.uint32) << np.uint32(8))
    err, _ = frame_error_restated(a, c, w, rows)
    assert abs(api.error_psnr(err) - host.psnr(a, c)) <= 1e-9
    assert api.error_psnr(api.FrameError.from_dict(err)) == api.error_psnr(err)


def test_error_psnr_of_equal_frames_is_infinite_and_the_top_byte_is_ignored():
    a, _ = random_frames(41, 23, 11)
    b = a ^ np.uint32(0xAB000000)
    err, tiles = frame_error_restated(a, b, 41, 23)
    assert err == {"sq_err": [0, 0, 0], "differing": 0, "pixels": 41 * 23, "max_abs": 0, "reserved": 0} and not tiles.any()
    assert api.error_psnr(err) == math.inf and host.psnr(a, b) == math.inf
    assert api.error_psnr({"sq_err": [0, 0, 0], "differing": 0, "pixels": 0, "max_abs": 0}) == math.inf      # a rank without rows


def test_the_restatement_on_a_frame_worked_out_by_hand():
    """3 x 2 pixels, one tile: differences of (1, 2, 3) and (255, 0, 16) in two pixels, a top-byte difference in a third."""
    a = np.array([0x00030201, 0x11000000, 0x000010FF, 5, 6, 7], np.uint32)
    b = np.array([0x00000000, 0x22000000, 0x00100000, 5, 6, 7], np.uint32)
    err, tiles = frame_error_restated(a, b, 3, 2)
    assert err == {"sq_err": [1 + 255 * 255, 4 + 16 * 16, 9 + 16 * 16], "differing": 2, "pixels": 6, "max_abs": 255, "reserved": 0}
    assert tiles.tolist() == [[1 + 4 + 9 + 255 * 255 + 2 * 16 * 16]]
