"""Render state in and out, the part that needs no device: the seed streams of rt_stream_seeds against a numpy restatement of the
formula in include/rt_api.h, and the argument checks of the entry points that write a context's state."""
import ctypes as C

import numpy as np
import pytest

from raytracing_simple_amd import api, host


def restated_stream(stream_id, count):
    """include/rt_api.h, rt_stream_seeds: the splitmix64 finaliser of (stream_id, i) in wrapping uint64, clamped to >= 2."""
    n_pairs = (count + 1) // 2
    golden = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = np.uint64(stream_id) * golden + np.arange(n_pairs, dtype=np.uint64) + golden
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    out = np.empty(2 * n_pairs, np.uint32)
    out[0::2] = np.maximum((z & np.uint64(0xFFFFFFFF)).astype(np.uint32), 2)
    out[1::2] = np.maximum((z >> np.uint64(32)).astype(np.uint32), 2)
    return out[:count]


@pytest.mark.parametrize("stream_id", [1, 2, 2 ** 40 + 3])
@pytest.mark.parametrize("count", [2 * 41 * 23, 2 * 41 * 23 - 1, 1, 0])
def test_stream_seeds_equal_the_restated_formula(stream_id, count):
    got = api.stream_seeds(stream_id, count)
    assert got.dtype == np.uint32 and got.size == count
    assert np.array_equal(got, restated_stream(stream_id, count))
    assert count == 0 or got.min() >= 2                      # the reference's clamp (a seed word of 0 or 1 degenerates its generator)


def test_the_clamp_is_applied_to_either_half():
    """No pair of the streams above needs the clamp (a word below 2 has probability 2^-31), so the clamp itself is checked on the
    restatement's terms: the library's words are never below 2 over a million pairs, and equal the restatement there too."""
    got = api.stream_seeds(7, 2 * (1 << 20))
    assert got.min() >= 2 and np.array_equal(got, restated_stream(7, 2 * (1 << 20)))


def test_stream_zero_is_the_default_stream():
    for count in (2 * 41 * 23, 2 * 41 * 23 - 1):
        assert np.array_equal(api.stream_seeds(0, count), host.default_seeds(count))


def test_two_streams_differ_in_every_pair_of_an_image():
    n = 2 * 41 * 23
    a, b, d = (api.stream_seeds(k, n).reshape(-1, 2) for k in (1, 2, 0))
    for x, y in ((a, b), (a, d), (b, d)):
        assert np.all((x != y).any(axis=1))


def test_a_null_buffer_is_ignored():
    api.load_library().rt_stream_seeds(3, None, 16)


def test_every_state_entry_point_refuses_a_null_context():
    lib = api.load_library()
    buf = np.zeros(16, np.float32)
    one = (C.c_void_p * 1)(None)
    for rc in (lib.rt_seed_stream_async(None, 1, None),
               lib.rt_write_state(None, api._ptr(buf), None, 0),
               lib.rt_save_state(None, b"/nonexistent/state.bin"),
               lib.rt_load_state(None, b"/nonexistent/state.bin"),
               lib.rt_merge_async(None, one, 1, None)):
        assert rc == -1                                      # RT_ERR_ARG
        assert b"null" in lib.rt_last_error()


def test_the_bindings_exist():
    for name in ("seed_stream", "write_state", "save_state", "load_state", "merge"):
        assert callable(getattr(api.RtContext, name))
    for name in ("rt_stream_seeds", "rt_seed_stream_async", "rt_write_state", "rt_save_state", "rt_load_state", "rt_merge_async"):
        assert name in api.SYMBOLS
