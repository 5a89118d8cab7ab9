"""Render state in and out (include/rt_api.h "render state", csrc/rt_state.hip) against the CPU oracle: resumed renders, seed
streams, merged frames, checkpoint files.  Every comparison is of bits -- colour-plane words, seeds, packed pixels.  The oracle
is tests/_oracle.py render(first_sample, seeds_in, colors_in), never the library; the seed formula is restated in numpy uint64
(test_state_cpu.restated_stream), the merge formula in numpy float32 with separate multiply and add (merge_restated)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host, scenes
from test_state_cpu import restated_stream

pytestmark = pytest.mark.gpu

W, H = 41, 23            # no multiple of the 8x8 tile; 3 * W * H = 2829 is odd: the merge kernel's scalar tail runs
RT_ERR_ARG, RT_ERR_STATE = -1, -5


@functools.lru_cache(maxsize=None)
def scene(name):
    sph, orig, target = (host.demo_scene(), host.DEMO_ORIG, host.DEMO_TARGET) if name == "demo" else scenes.demo_plus(16)
    return sph, orig, target


def camera(name, w, h):
    _, orig, target = scene(name)
    return host.compute_camera(orig, target, w, h)


@functools.lru_cache(maxsize=None)
def oracle(name, w, h, spp, stream_id=0):
    """`spp` straight passes of the oracle on seed stream `stream_id`; computed once, handed out read-only."""
    seeds = None if stream_id == 0 else restated_stream(stream_id, 2 * w * h)
    out = O.render(scene(name)[0], camera(name, w, h), w, h, spp, seeds_in=seeds)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def merge_restated(planes, passes):
    """include/rt_api.h rt_merge_async, restated: contexts at pass 0 skipped; multiply, then add, then one multiply by the reciprocal."""
    acc, total = None, 0
    for c, n in zip(planes, passes):
        if n <= 0:
            continue
        term = np.asarray(c, np.float32) * np.float32(n)
        acc = term if acc is None else (acc + term).astype(np.float32)
        total += n
    return (acc * (np.float32(1.0) / np.float32(total))).astype(np.float32)


def pack(colors, w, h):
    """The oracle's toInt over a colour plane, in the pixel buffer's layout: row 0 = bottom, the plane y-flipped (.cl:579,594-596)."""
    lib = O.oracle()
    ch = np.array([lib.orc_to_int(float(v)) for v in colors], np.uint32).reshape(h, w, 3)[::-1]
    return (ch[:, :, 0] | (ch[:, :, 1] << 8) | (ch[:, :, 2] << 16)).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(name, w=W, h=H, **kw):
    ctx = api.RtContext(w, h, **kw)
    ctx.set_scene(scene(name)[0])
    ctx.set_camera(camera(name, w, h))
    return ctx


def own_rows(ctx):
    """Rows of the pixel / seed buffers this context renders, and the same rows of the y-flipped colour plane."""
    rows = ctx.local_row_map()
    return rows, ctx.h - 1 - rows


def assert_state(ctx, want, pixels=None):
    """Colours, seeds, pass number (and packed pixels) of `ctx` equal the oracle's `want` on the rows the context renders."""
    rows, crows = own_rows(ctx)
    w, h = ctx.w, ctx.h
    assert np.array_equal(bits(ctx.read_colors()).reshape(h, 3 * w)[crows], bits(want["colors"]).reshape(h, 3 * w)[crows])
    assert np.array_equal(ctx.read_seeds().reshape(h, 2 * w)[rows], want["seeds"].reshape(h, 2 * w)[rows])
    px = ctx.read_pixels() if pixels is None else pixels
    assert np.array_equal(px.reshape(-1, w), want["pixels"].reshape(h, w)[rows])


def assert_counters(ctx, want):
    g, o = ctx.stats(), want["stats"]
    assert (g["samples"], g["closest_rays"], g["shadow_rays"], g["sphere_tests"], g["rng_draws"]) == \
           (o["samples"], o["closest_calls"], o["shadow_calls"], o["sphere_tests"], o["rng_draws"])


def snapshot(ctx):
    return bits(ctx.read_colors()).copy(), ctx.read_seeds().copy(), ctx.current_sample


def assert_unchanged(ctx, snap):
    now = snapshot(ctx)
    assert np.array_equal(now[0], snap[0]) and np.array_equal(now[1], snap[1]) and now[2] == snap[2]


# ---- 1. resume ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("demo", {}), ("coop16", {}), ("demo", {"rank": 1, "nranks": 3}), ("demo", {"devices": [0, 0]})],
                         ids=["demo", "cooperative-16-spheres", "rank-1-of-3", "two-shards"])
def test_a_render_written_into_a_fresh_context_continues_bit_for_bit(name, kw):
    with make(name) as a, make(name, **kw) as b:
        frame = a.render_pass(3)
        assert np.array_equal(frame, oracle(name, W, H, 3)["pixels"])
        b.write_state(a.read_colors(), a.read_seeds(), 3)
        assert b.current_sample == 3 and b.stats()["launches"] == 0 and b.stats()["samples"] == 0
        rows, _ = own_rows(b)
        assert np.array_equal(b.read_pixels().reshape(-1, W), frame.reshape(H, W)[rows])      # toInt of the restored plane
        px = b.render_pass(4)
        assert b.current_sample == 7
        assert_state(b, oracle(name, W, H, 7), px)
        assert_state(b, oracle(name, W, H, 7))                                                # ... and through rt_read_pixels
        if name == "coop16":
            assert "coop" in b.last_kernel


# ---- 2. streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"devices": [0, 0]}], ids=["one-context", "two-shards"])
def test_seed_streams_are_generated_on_the_device_and_render_the_oracles_frames(kw):
    with make("demo", **kw) as ctx:
        ctx.render_pass(2)                                  # something to go back from
        ctx.seed_stream(5, None if kw else ctx.stream)
        assert ctx.current_sample == 0
        assert np.array_equal(ctx.read_seeds(), restated_stream(5, 2 * W * H))
        px = ctx.render_pass(4)
        want = oracle("demo", W, H, 4, 5)
        assert ctx.current_sample == 4
        assert_state(ctx, want, px)
        assert_counters(ctx, want)
        assert not np.array_equal(px, oracle("demo", W, H, 4)["pixels"])     # another stream, another frame
        # stream 0 is the default stream, read in place: rt_reset_async
        default = oracle("demo", W, H, 4)
        ctx.seed_stream(0, None if kw else ctx.stream)
        assert ctx.current_sample == 0 and np.array_equal(ctx.read_seeds(), host.default_seeds(2 * W * H))
        assert_state(ctx, default, ctx.render_pass(4))
        assert_counters(ctx, default)
        ctx.seed_stream(5)
        ctx.render_pass(1)
        ctx.write_state(None, None, 0)                      # ... and so is a state without seeds
        assert ctx.current_sample == 0 and np.array_equal(ctx.read_seeds(), host.default_seeds(2 * W * H))
        assert_state(ctx, default, ctx.render_pass(4))
        assert_counters(ctx, default)
        with make("demo") as fresh:
            assert np.array_equal(fresh.render_pass(4), default["pixels"])


def test_seed_stream_kernel_across_several_workgroups():
    w, h = 200, 120
    with api.RtContext(w, h) as ctx:
        ctx.seed_stream(2 ** 40 + 3, ctx.stream)
        assert np.array_equal(ctx.read_seeds(), restated_stream(2 ** 40 + 3, 2 * w * h))


# ---- 3. merge ----------------------------------------------------------------------------------------------------
PASSES = (3, 5, 2)


def _three(w, h):
    ctxs = [make("demo", w, h) for _ in PASSES]
    for k, (c, n) in enumerate(zip(ctxs, PASSES)):
        c.seed_stream(k + 1, c.stream)
        c.render_async(n, c.stream)
    return ctxs


def test_merge_is_the_sample_weighted_average_and_the_render_goes_on_from_it():
    ctxs = _three(W, H)
    try:
        dst = ctxs[0]
        dst.merge(ctxs[1:], dst.stream)
        want = merge_restated([oracle("demo", W, H, n, k + 1)["colors"] for k, n in enumerate(PASSES)], PASSES)
        assert dst.current_sample == 10
        assert np.array_equal(bits(dst.read_colors()), bits(want))
        assert np.array_equal(dst.read_pixels(), pack(want, W, H))
        seeds = oracle("demo", W, H, PASSES[0], 1)["seeds"]
        assert np.array_equal(dst.read_seeds(), seeds)                        # dst's seeds stay
        for k in (1, 2):                                                      # the sources are only read
            src = oracle("demo", W, H, PASSES[k], k + 1)
            assert ctxs[k].current_sample == PASSES[k]
            assert_state(ctxs[k], src)
        nxt = O.render(scene("demo")[0], camera("demo", W, H), W, H, 1, first_sample=10, seeds_in=seeds, colors_in=want)
        px = dst.render_pass(1)
        assert dst.current_sample == 11
        assert_state(dst, nxt, px)
    finally:
        for c in ctxs:
            c.close()


def test_merge_kernel_across_several_workgroups():
    w, h = 200, 120
    ctxs = _three(w, h)
    try:
        ctxs[0].merge(ctxs[1:])                              # (the null stream: ordered behind the contexts' own streams all the same)
        want = merge_restated([oracle("demo", w, h, n, k + 1)["colors"] for k, n in enumerate(PASSES)], PASSES)
        assert ctxs[0].current_sample == 10
        assert np.array_equal(bits(ctxs[0].read_colors()), bits(want))
    finally:
        for c in ctxs:
            c.close()


# ---- 4. a context at pass 0 is skipped ---------------------------------------------------------------------------
def test_merge_skips_a_destination_at_pass_zero_whose_plane_holds_an_old_frame():
    with make("demo") as dst, make("demo") as s1, make("demo") as s2:
        dst.render_pass(2)
        dst.reset_async(dst.stream)                          # pass 0; the plane still holds the two-pass frame
        assert dst.current_sample == 0 and np.any(dst.read_colors() != 0)
        s1.seed_stream(2, s1.stream)
        s1.render_pass(5)
        s2.seed_stream(3, s2.stream)
        s2.render_pass(2)
        dst.merge([s1, s2], dst.stream)
        want = merge_restated([oracle("demo", W, H, 5, 2)["colors"], oracle("demo", W, H, 2, 3)["colors"]], (5, 2))
        assert dst.current_sample == 7
        assert np.array_equal(bits(dst.read_colors()), bits(want))
        assert np.array_equal(dst.read_pixels(), pack(want, W, H))
        # ... and a source at pass 0 likewise
        s2.reset_async(s2.stream)
        before = bits(dst.read_colors()).copy()
        dst.merge([s2])
        assert dst.current_sample == 7
        assert np.array_equal(bits(dst.read_colors()), bits(merge_restated([before.view(np.float32)], (7,))))


# ---- 5. refusals -------------------------------------------------------------------------------------------------
def _refused(ctx, code, call, *args):
    with pytest.raises(api.RtError) as e:
        call(*args)
    assert e.value.code == code, e.value
    return str(e.value)


def test_refused_calls_leave_the_context_as_it_was(tmp_path):
    def device_count():
        import torch
        return torch.cuda.device_count()

    with make("demo") as dst, make("demo") as src, make("demo", W + 1, H) as wider, make("demo", rank=1, nranks=3) as shard, \
            make("demo", devices=[0, 0]) as multi:
        dst.seed_stream(1)
        dst.render_pass(3)
        src.render_pass(2)
        multi.render_pass(2)
        col, sd = dst.read_colors(), dst.read_seeds()
        snap, snap_src, snap_multi = snapshot(dst), snapshot(src), snapshot(multi)
        lib = api.load_library()
        # rt_write_state
        assert "current_sample" in _refused(dst, RT_ERR_ARG, dst.write_state, col, sd, -1)
        assert "colors_host" in _refused(dst, RT_ERR_ARG, dst.write_state, None, sd, 2)
        _refused(multi, RT_ERR_ARG, multi.write_state, None, None, 1)
        assert_unchanged(dst, snap)
        assert_unchanged(multi, snap_multi)
        # rt_save_state / rt_load_state: null and unusable paths
        assert lib.rt_save_state(dst._h, None) == RT_ERR_ARG and lib.rt_load_state(dst._h, None) == RT_ERR_ARG
        _refused(dst, RT_ERR_ARG, dst.save_state, tmp_path / "no_such_dir" / "s.bin")
        _refused(dst, RT_ERR_ARG, dst.load_state, tmp_path / "missing.bin")
        assert_unchanged(dst, snap)
        # rt_merge_async
        assert lib.rt_merge_async(dst._h, None, 1, None) == RT_ERR_ARG
        _refused(dst, RT_ERR_ARG, dst.merge, [])
        with make("demo") as extra:
            _refused(dst, RT_ERR_ARG, dst.merge, [src] + [extra] * 15)         # 16 sources
            assert "repeats" in _refused(dst, RT_ERR_ARG, dst.merge, [src, extra, src])
        assert "null" in _refused(dst, RT_ERR_ARG, dst.merge, [src, None])
        assert "destination" in _refused(dst, RT_ERR_ARG, dst.merge, [src, dst])
        _refused(dst, RT_ERR_ARG, dst.merge, [wider])                           # another image size
        _refused(dst, RT_ERR_ARG, dst.merge, [shard])                           # another sharding
        _refused(shard, RT_ERR_ARG, shard.merge, [src])
        assert "multi-device" in _refused(dst, RT_ERR_ARG, dst.merge, [multi])
        assert "multi-device" in _refused(multi, RT_ERR_ARG, multi.merge, [src])
        if device_count() >= 2:                              # (a one-GPU machine cannot make this case)
            with make("demo", device=1) as elsewhere:
                elsewhere.render_pass(1)
                assert "device" in _refused(dst, RT_ERR_ARG, dst.merge, [elsewhere])
        with make("demo") as e1, make("demo") as e2:                            # nothing rendered anywhere: N == 0
            s1 = snapshot(e1)
            _refused(e1, RT_ERR_STATE, e1.merge, [e2])
            assert_unchanged(e1, s1)
        assert_unchanged(dst, snap)
        assert_unchanged(src, snap_src)
        assert_unchanged(multi, snap_multi)
        # the contexts still work: what was refused left nothing half done
        assert_state(dst, oracle("demo", W, H, 4, 1), dst.render_pass(1))


# ---- 6. files ----------------------------------------------------------------------------------------------------
def test_a_checkpoint_file_resumes_the_render_and_bad_files_are_refused(tmp_path):
    path = tmp_path / "state.bin"
    with make("demo") as a:
        a.render_pass(3)
        a.save_state(path)
        assert a.current_sample == 3
    raw = path.read_bytes()
    assert len(raw) == 24 + 20 * W * H and raw[:8] == b"RTSTATE\0"                # the documented layout
    assert np.array_equal(np.frombuffer(raw[8:24], "<i4"), [1, W, H, 3])
    assert np.array_equal(np.frombuffer(raw[24:24 + 12 * W * H], "<u4"), bits(oracle("demo", W, H, 3)["colors"]))
    assert np.array_equal(np.frombuffer(raw[24 + 12 * W * H:], "<u4"), oracle("demo", W, H, 3)["seeds"])
    with make("demo") as b:
        b.load_state(path)
        assert b.current_sample == 3
        assert np.array_equal(b.read_pixels(), oracle("demo", W, H, 3)["pixels"])
        px = b.render_pass(4)
        assert b.current_sample == 7
        assert_state(b, oracle("demo", W, H, 7), px)
        snap = snapshot(b)
        bad = tmp_path / "bad.bin"
        for data, word in ((raw[:-5], "short"), (raw[:10], "short"), (b"", "short"), (b"RTSTATF\0" + raw[8:], "magic"),
                           (raw[:12] + np.array([W + 1], "<i4").tobytes() + raw[16:], "image size"),
                           (raw[:8] + np.array([2], "<u4").tobytes() + raw[12:], "version"),
                           (raw[:20] + np.array([-1], "<i4").tobytes() + raw[24:], "pass number")):
            bad.write_bytes(data)
            assert word in _refused(b, RT_ERR_ARG, b.load_state, bad)
            assert_unchanged(b, snap)
        with make("demo", W + 1, H) as other:                # the same file, another context size
            s2 = snapshot(other)
            assert "image size" in _refused(other, RT_ERR_ARG, other.load_state, path)
            assert_unchanged(other, s2)


# ---- what a context acquires, its teardown gives back (csrc/rt_owned.h) -------------------------------------------------------------------
def _every_resource_once(w, h):
    """Two halves and a destination of w x h on device 0, driven through every call that acquires something on first use; returns what must stay
    alive until they are closed: the contexts, and the buffers the first one has had registered."""
    cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
    many = scenes.random_spheres(200)[0].copy()
    many[199] = many[198]                                   # one record repeats another bit for bit: the duplicate flags and their staging exist
    a, b, dst = (api.RtContext(w, h) for _ in range(3))
    for k, c in enumerate((a, b, dst)):
        c.set_scene(host.demo_scene())                      # tables and staging ring for 64 records ...
        c.set_camera(cam)
        c.set_scene(many)                                   # ... grown to 256; the hierarchy, the host's tree and its staging
        c.update_spheres(3, many[3:9])
        if k < 2:
            c.seed_stream(k + 1)
            c.render_async(2)
    dst.merge([a, b])
    a.compare(b, tiles=True)
    for c in (a, b):
        c.set_denoise_guide(api.guide_defaults())
        c.features_async()
    dst.denoise(a, b)
    a.denoise_pair(b)
    assert a.select_tiles(None, 0, a.stream) == b.select_tiles(None, 0, b.stream)
    a.render_tiles_async(1, a.stream)
    b.render_tiles_async(1, b.stream)
    a.denoise_pair_tiles(b)
    outs = [np.zeros(w * h, np.uint32) for _ in range(2)]
    for c in (a, b, dst):
        c.throttle(4)
        c.throttle(0)
    for out in outs:
        a.pin_output(out)                                   # the second call gives the first registration back
    return [a, b, dst], outs


def test_contexts_give_back_every_resource_they_acquired():
    """Free device memory after two halves and a destination that have acquired everything a context can -- regrown scene tables and staging, the
    hierarchy's blob and staging, duplicate flags, the tile arrays, compare scratch, feature, filter and variance planes, throttle events, a registered
    output buffer -- and were closed is what it was before them, within the megabyte tests/test_gpu_features.py allows a broken multi-device
    context; and again after a second such cycle against the SAME baseline, so that one plane lost per cycle shows even where the first loss fits
    the margin.  While they are held, at least the bytes the planes acquired on first use ask for are gone (the sum below, from w and h alone)."""
    import torch
    w, h = 512, 256
    px = w * h
    on_first_use = (2 * 8 * px * 4          # feature planes of the two halves
                    + 2 * 3 * px * 4        # their cross-filtered planes ...
                    + 2 * px * 4            # ... packed
                    + 2 * 3 * px * 4        # variance planes: the first half's, the destination's
                    + 3 * px * 4)           # the plane the destination's filter writes
    ctxs, outs = _every_resource_once(w, h)                 # (a first cycle pays the process-wide allocations: not part of the baseline)
    for c in ctxs:
        c.close()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    for cycle in range(2):
        ctxs, outs = _every_resource_once(w, h)
        torch.cuda.synchronize()
        held = free_before - torch.cuda.mem_get_info(0)[0]
        print("cycle %d: %d bytes held, %d acquired on first use" % (cycle, held, on_first_use))
        assert held >= on_first_use, (cycle, held, on_first_use)
        for c in ctxs:
            c.close()
        torch.cuda.synchronize()
        free_after = torch.cuda.mem_get_info(0)[0]
        print("cycle %d: free %d before, %d after" % (cycle, free_before, free_after))
        assert free_after >= free_before - (1 << 20), (cycle, free_before, free_after)
        del outs


def test_a_multi_device_context_gives_back_what_it_acquired():
    """The same bound for rt_multi's own record (the assembled frame, the two receive slots, events, the gather stream) and its shards: one device
    listed twice, created, rendered, closed."""
    import torch
    w, h = 96, 64
    sph, orig, target = scene("plus")
    cam = host.compute_camera(orig, target, w, h)

    def cycle():
        ctx = api.RtContext(w, h, devices=[0, 0])
        ctx.set_scene(sph)
        ctx.set_camera(cam)
        ctx.render_pass(1)
        return ctx

    cycle().close()                                         # (process-wide allocations)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    for _ in range(2):
        ctx = cycle()
        assert torch.cuda.mem_get_info(0)[0] < free_before  # (the context holds device memory now)
        ctx.close()
        torch.cuda.synchronize()
        free_after = torch.cuda.mem_get_info(0)[0]
        print("multi: free %d before, %d after" % (free_before, free_after))
        assert free_after >= free_before - (1 << 20), (free_before, free_after)
