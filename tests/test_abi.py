"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/rt_api.h
declares, validates arguments, fails loudly without a GPU, and its host helpers agree with the
oracle and with the reference-generated pins.  No device compute here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
from raytracing_simple_amd import api, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_present():
    return os.path.exists("/dev/kfd")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_library_exports_exactly_the_declared_symbols():
    """librt_hip.so exports what include/rt_api.h declares and NOTHING else (no rt_debug_*, no kernel
    stubs, no C++ runtime instantiations); librt_hip_diag.so adds exactly include/rt_debug.h."""
    from raytracing_simple_amd import _build
    declared = _build.declared_symbols("rt_api.h")
    assert declared == sorted(api.SYMBOLS)
    lib = api.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert _exports(api.lib_path()) == declared
    debug = sorted(set(_build.declared_symbols("rt_debug.h")) - set(declared))
    assert debug == sorted(api.DEBUG_SYMBOLS)
    assert _exports(api.lib_path(diag=True)) == sorted(declared + debug)
    assert not any(n.startswith("rt_debug") for n in _exports(api.lib_path()))


SHIPPED_PARITY = ["rt_trace_parity" + k for k in ("_w1", "_coop", "_coop_w1", "_pairs", "_pairs_m", "_pairs_g", "_g")]
SHIPPED_FAST = [k.replace("parity", "fast") for k in SHIPPED_PARITY]


def test_shipped_kernels_have_no_private_segment_and_fit_their_occupancy():
    """no kernel of the product library uses scratch (no register spills, no private arrays), the
    sweep instances fit 80 vector registers (6 wavefronts per SIMD), the instances that walk the hierarchy 96 (5 per SIMD).
    Read from the code objects inside librt_hip.so (rt_trace_parity_coop had a 12-byte private segment,
    rt_trace_parity_pairs_g 98 registers)."""
    from raytracing_simple_amd import _build
    meta = _build.kernel_metadata()
    trace = {k: v for k, v in meta.items() if k.startswith("rt_trace_")}
    assert sorted(trace) == sorted(SHIPPED_PARITY + SHIPPED_FAST), sorted(trace)        # the instances that ship, by name (rt_kernel_parity.hip / rt_kernel_fast.hip)
    assert len(meta) >= 23, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        # (rt_trace_parity_g holds two groups of four records in 32 scalar registers through its sweeps, round 6; twelve scalar values the prologue
        # forms for the epilogue -- masks of `tid < 5`, the tile number -- are parked in lanes of ONE vector register meanwhile: v_writelane before the
        # loop, v_readlane after it, none inside a sweep, no scratch)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] <= (12 if name == "rt_trace_parity_g" else 0), (name, m)
        assert "agpr_count" in m and m["agpr_count"] == 0, (name, m)
    for name, m in trace.items():
        assert m["vgpr_count"] <= (96 if "_pairs" in name else 80), (name, m["vgpr_count"])


def test_every_shipped_parity_instance_has_a_profile_of_this_library():
    """"every shipped parity instance has a stamped profile"  -- held here: the kernels that ship are read
    from the product library's code objects, and each parity instance (and the fast-mode headline instance) must have a profiles/*.json whose `kernel`
    is its symbol and whose `build_id` is the id of the sources this library is built from (tools/profile_gpu.sh + tools/collect.py write them)."""
    import glob
    import json
    from raytracing_simple_amd import _build
    lib_id = _build.source_hash()
    have = {}
    for f in glob.glob(os.path.join(ROOT, "profiles", "*.json")):
        try:
            d = json.load(open(f))
        except ValueError:
            continue
        if isinstance(d, dict) and isinstance(d.get("kernel"), str) and d.get("build_id"):
            have.setdefault(d["kernel"], {})[d["build_id"]] = os.path.basename(f)
    shipped = sorted(k for k in _build.kernel_metadata() if k.startswith("rt_trace_parity"))
    assert shipped == sorted(SHIPPED_PARITY)
    missing = [k for k in shipped + ["rt_trace_fast_w1"] if lib_id not in have.get(k, {})]
    assert not missing, "no profile of library %s for: %s (run tools/session.sh P through gpurun, then tools/collect.py)" % (lib_id, missing)
    for k in shipped:                       # ... and the record is a real one: launches, counters
        d = json.load(open(os.path.join(ROOT, "profiles", have[k][lib_id])))
        assert d.get("timed_launches", 0) >= 5 and d["pmc_per_launch_avg"].get("SQ_INSTS_VALU", 0) > 0 and "launch" in d, have[k][lib_id]


def test_no_built_binaries_are_tracked():
    """Built artefacts stay out of history (.gitignore policy): no ELF file in the index."""
    files = subprocess.run(["git", "ls-files"], cwd=ROOT, capture_output=True, text=True)
    if files.returncode != 0:
        pytest.skip("not a git checkout (GPU box snapshot)")
    elf = []
    for f in files.stdout.split():
        p = os.path.join(ROOT, f)
        if os.path.isfile(p) and open(p, "rb").read(4) == b"\x7fELF":
            elf.append(f)
    assert elf == []


def test_struct_layouts_match_reference_sizes():
    assert api.SPHERE_DT.itemsize == 44          # Sphere.hpp:11-15
    assert api.CAMERA_FLOATS * 4 == 60           # Camera.hpp:7-14
    assert C.sizeof(api.Stats) == 7 * 8


@pytest.mark.skipif(_gpu_present(), reason="checks the no-device failure path")
def test_fails_loudly_without_device():
    with pytest.raises(api.RtError) as e:
        api.RtContext(64, 64)
    assert e.value.code == -2
    with pytest.raises(api.RtError):
        api.render(host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, 8, 8), 8, 8, 1)
    with pytest.raises(api.RtError):
        api.debug_eval(0, np.zeros(4, np.float32))


def test_argument_validation_needs_no_device():
    lib = api.load_library()
    h = C.c_void_p()
    assert lib.rt_create(C.byref(h), 0, 10) == -1
    assert lib.rt_create_sharded(C.byref(h), 16, 16, 0, 2, 2, 8) == -1       # rank >= nranks
    assert lib.rt_create_sharded(C.byref(h), 16, 16, 0, 0, 2, 12) == -1      # tile_rows % 8
    assert b"tile_rows" in lib.rt_last_error()
    assert lib.rt_render(None, None, None, 4, 4, 1) == -1
    assert lib.rt_set_scene(None, None, 0) == -1
    assert lib.rt_local_rows(None) == -1
    # the round-2 entry points: argument checks come before any device call
    assert lib.rt_create_multi(C.byref(h), 16, 16, 0) == -1 and b"ngpus" in lib.rt_last_error()
    assert lib.rt_create_multi(C.byref(h), 16, 16, 65) == -1
    assert lib.rt_create_multi_on(C.byref(h), 0, 16, (C.c_int * 1)(0), 1, 8) == -1
    assert lib.rt_create_multi_on(C.byref(h), 16, 16, None, 1, 8) == -1
    # the device list of a multi-device context: all different, or one device n times (the rehearsal) -- never mixed
    assert lib.rt_create_multi_on(C.byref(h), 16, 16, (C.c_int * 3)(0, 1, 0), 3, 8) == -1 and b"mixed" in lib.rt_last_error()
    assert lib.rt_create_multi_on(C.byref(h), 16, 16, (C.c_int * 4)(2, 2, 3, 3), 4, 8) == -1
    assert lib.rt_create_multi_on(C.byref(h), 16, 16, (C.c_int * 2)(0, -1), 2, 8) == -1
    assert lib.rt_create_multi_on(C.byref(h), 16, 16, (C.c_int * 2)(0, 0), 2, 12) == -1 and b"tile_rows" in lib.rt_last_error()
    assert lib.rt_throttle(None, 0, None) == -1 and lib.rt_read_pixels_async(None, None, None) == -1
    assert lib.rt_shard_count(None) == -1
    assert lib.rt_update_spheres_async(None, 0, 0, None, None) == -1
    assert lib.rt_read_pixels(None, None) == -1
    assert lib.rt_deinterleave_rows(None, None, 16, 16, 1, 8, 16, 0, None) == -1
    buf = (C.c_uint32 * 4)()
    assert lib.rt_deinterleave_rows(buf, buf, 0, 16, 1, 8, 16, 0, None) == -1
    assert lib.rt_deinterleave_rows(buf, buf, 16, 16, 2, 8, 4, 0, None) == -1 and b"pad_rows" in lib.rt_last_error()
    lib.rt_release_cache()                                            # nothing cached: a no-op, no device needed


def test_default_seeds_equal_oracle_and_pins(golden_dir):
    pins = np.load(os.path.join(golden_dir, "host_pins.npz"))
    mine = host.default_seeds(2 * 64 * 64)
    assert np.array_equal(mine, pins["seeds_first_8192"])
    assert np.array_equal(host.default_seeds(2 * 800 * 600), O.seeds(800, 600))
    # the library keeps the head of the stream per process (2^23 words): shorter requests, repeated
    # requests and requests that run past the kept head all return the same stream
    assert O.fnv(host.default_seeds(2 * 1920 * 1080)) == str(pins["fnv_seeds_1920x1080"])
    long = host.default_seeds((1 << 23) + 4096)
    want = O.seeds(2100, 2000)[: (1 << 23) + 4096]              # the oracle's own generator, 8.4 M words
    assert np.array_equal(long, want)
    assert np.array_equal(host.default_seeds(1000), want[:1000])
    assert np.array_equal(host.default_seeds((1 << 23) + 4096), want)


def test_compute_camera_equals_oracle_and_pins(golden_dir):
    pins = np.load(os.path.join(golden_dir, "host_pins.npz"))
    for (w, h) in [(256, 256), (800, 600), (1920, 1080), (3840, 2160)]:
        cam = host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h)
        assert np.array_equal(cam.view(np.uint32), pins[f"camera_{w}x{h}"].view(np.uint32))
    rng = np.random.default_rng(5)
    for _ in range(200):
        o, t = rng.normal(size=3) * 50, rng.normal(size=3) * 50
        w, h = int(rng.integers(1, 4000)), int(rng.integers(1, 3000))
        a = host.compute_camera(o, t, w, h)
        b = O.camera(o.astype(np.float32), t.astype(np.float32), w, h)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_demo_scene_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "c1_demo_256x256_1spp.npz"))
    assert host.demo_scene().tobytes() == z["spheres"].tobytes()


def test_scene_reader_roundtrip_and_doubling(tmp_path):
    sph = O.demo_spheres()
    p = tmp_path / "t.scn"
    host.write_scene(p, sph, (1.5, 2, 3), (4, 5, 6.25))
    got, o, t = host.read_scene(p, reference_doubling=False)
    assert got.tobytes() == sph.view(api.SPHERE_DT).tobytes() and o == (1.5, 2.0, 3.0) and t == (4.0, 5.0, 6.25)
    dbl, _, _ = host.read_scene(p, reference_doubling=True)
    assert len(dbl) == 12 and dbl[:6].tobytes() == bytes(6 * 44) and dbl[6:].tobytes() == got.tobytes()


def test_scene_reader_errors(tmp_path):
    with pytest.raises(api.RtError, match="Failed to open"):
        host.read_scene(tmp_path / "missing.scn")
    p = tmp_path / "bad.scn"
    p.write_text("camera 1 2 3 4 5\nsize 1\n")
    with pytest.raises(api.RtError, match="camera"):
        host.read_scene(p)
    p.write_text("camera 1 2 3 4 5 6\nsize 1\nsphere 1  0 0 0  0 0 0  1 1 1  7\n")
    with pytest.raises(api.RtError, match="material"):
        host.read_scene(p)
    p.write_text("camera 1 2 3 4 5 6\nsize 2\nsphere 1  0 0 0  0 0 0  1 1 1  0\n")
    with pytest.raises(api.RtError, match="sphere #1"):
        host.read_scene(p)
    p.write_text("camera 1 2 3 4 5 6\nsize 0\n")
    got, _, _ = host.read_scene(p)
    assert len(got) == 0


@pytest.mark.skipif(not O.ref_tree_available(), reason="reference loader exists only in the build container")
def test_scene_reader_equals_reference_loader_on_shipped_scenes():
    d = os.path.join(O.REF_ROOT, "SimpleRT", "Scene")
    for name in sorted(os.listdir(d)):
        want, wo, wt = O.ref_read_scene(os.path.join(d, name), cap=16384)
        got, go, gt = host.read_scene(os.path.join(d, name), reference_doubling=True)
        assert got.tobytes() == want.tobytes(), name
        assert go == wo and gt == wt


def test_png_writer_equals_ppm_writer(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    px = (np.arange(7 * 5, dtype=np.uint32) * 2654435761 % (1 << 24)).astype(np.uint32)
    host.write_png(str(tmp_path / "a.png"), px, 7, 5)
    host.write_ppm(str(tmp_path / "a.ppm"), px, 7, 5)
    png = np.asarray(PIL.open(str(tmp_path / "a.png")).convert("RGB"))
    ppm = np.frombuffer(open(tmp_path / "a.ppm", "rb").read()[len(b"P6\n7 5\n255\n"):], np.uint8).reshape(5, 7, 3)
    assert np.array_equal(png, ppm)


def test_ppm_writer_flips_rows(tmp_path):
    px = np.arange(6, dtype=np.uint32).reshape(3, 2)      # row 0 = bottom
    host.write_ppm(tmp_path / "a.ppm", px, 2, 3)
    raw = (tmp_path / "a.ppm").read_bytes()
    assert raw.startswith(b"P6\n2 3\n255\n")
    body = np.frombuffer(raw[len(b"P6\n2 3\n255\n"):], np.uint8).reshape(3, 2, 3)
    assert body[0, 0, 0] == 4 and body[2, 1, 0] == 1       # top row of the file = buffer row 2


def test_committed_scn_files_equal_the_generators():
    """the synthetic BASELINE configurations exist as committed .scn files (the reference's wire
    format, Utility.cpp:90-160) so that the C++ hosts -- tools/rt_bench, the reference's own Main.cpp
    through the adapter -- can run all five configurations; they must be the generators' bytes."""
    from raytracing_simple_amd import scenes
    d = os.path.join(ROOT, "raytracing_simple_amd", "scenes_scn")
    for name, maker in (("c3_random_1024.scn", lambda: scenes.random_spheres(1024)),
                        ("c5_mirror_box_64.scn", lambda: scenes.mirror_box(64)),
                        ("c16_demo_plus_10.scn", lambda: scenes.demo_plus(16))):
        sph, orig, target = maker()
        got, o2, t2 = host.read_scene(os.path.join(d, name), reference_doubling=False)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(sph).view(np.uint8)), name
        assert np.array_equal(np.float32(orig), np.float32(o2)) and np.array_equal(np.float32(target), np.float32(t2))
        doubled, _, _ = host.read_scene(os.path.join(d, name), reference_doubling=True)     # what the reference's loader hands over
        assert len(doubled) == 2 * len(sph) and not doubled[: len(sph)].view(np.uint8).any()
        assert np.array_equal(doubled[len(sph):].view(np.uint8), got.view(np.uint8))


@pytest.mark.skipif(_gpu_present(), reason="checks the no-device paths of bench.py")
def test_bench_refuses_to_measure_without_the_gpus_it_was_asked_for():
    """`python bench.py --gpus N` without a launcher starts its ranks itself -- but never on fewer devices than asked
    for, and never on a CPU fallback."""
    import sys
    for argv, text in ((["--gpus", "2"], "nothing is measured on fewer"), ([], "no HIP device visible")):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=300,
                             env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
        assert res.returncode != 0 and text in (res.stderr + res.stdout), (argv, res.stderr[-500:])


def test_profile_counters_are_bound_to_the_code_they_describe(tmp_path, monkeypatch):
    """`roofline.executed` / `roofline.traffic` are constants of a committed profile.  They carry the build id
    of the library they were measured on (rt_build_id(): a hash of csrc/, the public headers and the compiler flags), and
    bench.py prints them only beside that library.  A touched kernel changes the id, and the line then drops both figures
    and says why."""
    import json
    import shutil
    sys.path.insert(0, ROOT)
    import bench
    from raytracing_simple_amd import _build
    # (1) the library knows its id, and the id is what the build recipe computes from the sources it compiled
    lib_id = api.build_id()
    assert len(lib_id) == 16 and lib_id == _build.source_hash() == api.build_id(diag=True)
    # (2) one character of one kernel source changes it
    copy = tmp_path / "csrc"
    shutil.copytree(_build.CSRC, copy, ignore=shutil.ignore_patterns("_obj"))
    monkeypatch.setattr(_build, "CSRC", str(copy))
    assert _build.source_hash() == lib_id
    with open(copy / "rt_trace.inc.h", "a") as f:
        f.write("// touched\n")
    assert _build.source_hash() != lib_id
    # (3) bench.py: counters beside the library they were measured on, withheld beside any other
    rec = {"kernel": "rt_trace_parity_w1", "build_id": lib_id, "valu_insts_per_launch": 2.4e9, "active_lane_frac": 0.64,
           "profiled_kernel_ms": 2.6, "valu_busy_frac_single_stream": 0.83, "hbm_bytes_per_launch": 77000000, "source": "test"}
    pmc = tmp_path / "pmc.json"
    pmc.write_text(json.dumps({"c2": {"parity": rec}}))
    monkeypatch.setattr(bench, "PMC_FILE", str(pmc))
    same = bench.roofline_block("rt_trace_parity_w1", 2.6, 1788296212, 1920 * 1080, 6, "c2", "parity")
    assert same["traffic"] == 77000000 and same["executed"]["valu_insts_per_launch"] == 2.4e9 and "counters_withheld" not in same
    assert same["frac_unfused"] == pytest.approx(2 * same["frac"], rel=1e-3) and same["peak_unfused"] < same["peak"]
    monkeypatch.setattr(bench, "library_build_id", lambda: "0123456789abcdef")          # the library has changed since the profile
    stale = bench.roofline_block("rt_trace_parity_w1", 2.6, 1788296212, 1920 * 1080, 6, "c2", "parity")
    assert stale["traffic"] is None and "executed" not in stale and lib_id in stale["counters_withheld"]
    monkeypatch.setattr(bench, "library_build_id", lambda: lib_id)                       # same library, another kernel instance
    other = bench.roofline_block("rt_trace_parity_coop_w1", 2.6, 1788296212, 1920 * 1080, 6, "c2", "parity")
    assert other["traffic"] is None and "executed" not in other


def _listing(*insns):
    """A synthetic kernel listing in llvm-objdump's layout, four bytes per instruction from address 0x100; a branch's operand is written
    as `@k`, the index of its target, and turned into the dword offset the disassembler prints."""
    lines = ["0000000000000100 <k>:"]
    for k, text in enumerate(insns):
        m = re.search(r"@(\d+)", text)
        if m:
            text = text.replace(m.group(0), str((int(m.group(1)) - k - 1) & 0xFFFF))
        lines.append("\t%-58s // %012X: 00000000" % (text, 0x100 + 4 * k))
    return lines


_CLEAN = ["s_mov_b32 s5, 0",
          "s_load_dwordx16 s[16:31], s[2:3], 0x0",
          "s_add_u32 s2, s66, s2",                      # other scalar registers are free
          "v_writelane_b32 v40, s32, 3",
          "s_cbranch_vccz @6",
          "s_mov_b32 s4, s15",
          "s_waitcnt lgkmcnt(0)",
          "s_mov_b32 s4, s16",                          # after the wait: the records are there
          "s_cbranch_scc1 @1",                          # a loop back to the load, behind the wait
          "s_endpgm"]


def test_scalar_load_path_checker_on_synthetic_listings():
    """tools/scalar_load_paths.py: a clean listing passes; each way of touching the sixteen registers of an s_load_dwordx16 before the
    s_waitcnt lgkmcnt(0) that makes them valid -- on ANY path: fall-through, taken branch, backward branch -- is flagged."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scalar_load_paths as S
    assert S.check_kernel(_listing(*_CLEAN)) == (1, [])
    assert S.check_kernel(_listing("s_mov_b32 s4, 0", "s_endpgm")) == (0, [])

    def flagged(*insns):
        n, bad = S.check_kernel(_listing(*insns))
        return n >= 1 and len(bad) >= 1

    load, wait = "s_load_dwordx16 s[16:31], s[2:3], 0x0", "s_waitcnt lgkmcnt(0)"
    assert flagged(load, "s_mov_b32 s4, s20", wait, "s_endpgm")                          # a destination register read before the wait
    assert flagged(load, "s_mov_b32 s31, 0", wait, "s_endpgm")                           # ... written (reused) before it
    assert flagged(load, "s_add_u32 s2, s[30:31], 1", wait, "s_endpgm")                  # ... named within a range
    assert flagged(load, "v_writelane_b32 v40, s17, 0", wait, "s_endpgm")                # copied into a lane
    assert flagged(load, "s_cbranch_vccz @4", wait, "s_endpgm", "s_mov_b32 s4, s16", "s_endpgm")     # a branch past the wait
    assert flagged(load, "s_cbranch_scc0 @3", wait, "s_endpgm")                          # ... to the end of the program
    assert flagged(load, "s_waitcnt lgkmcnt(1)", "s_mov_b32 s4, s16", wait, "s_endpgm")  # a wait that leaves one access outstanding
    assert flagged(load, "s_waitcnt vmcnt(0)", "s_mov_b32 s4, s16", "s_endpgm")          # a wait for vector memory only
    assert flagged("s_mov_b32 s5, 0", load, "s_add_u32 s5, s5, 1", "s_cbranch_scc1 @1", wait, "s_endpgm")   # the load again, no wait between
    assert flagged(load, "s_branch @3", wait, "s_mov_b32 s4, s18", "s_endpgm")           # an unconditional branch over the wait
    assert flagged(load, "s_mov_b32 s4, 0", "s_endpgm")                                  # the program ends, never waited for
    # a backward branch to before the load that reads the registers there
    assert flagged("s_mov_b32 s4, s16", load, "s_cbranch_scc1 @0", wait, "s_endpgm")
    # and a conditional branch whose fall-through is clean but whose target is not (both sides are followed)
    assert flagged(load, "s_cbranch_execz @5", wait, "s_nop 0", "s_endpgm", "v_mov_b32_e32 v1, s16", "s_endpgm")
    assert not flagged(load, "s_cbranch_execz @5", wait, "s_nop 0", "s_endpgm", wait, "v_mov_b32_e32 v1, s16", "s_endpgm")
    assert S.branch_offset("65432") == -104 and S.branch_offset("33") == 33
    assert S.waits_for_scalar_loads("s_waitcnt", "vmcnt(0) lgkmcnt(0)") and S.waits_for_scalar_loads("s_waitcnt", "0")
    assert S.waits_for_scalar_loads("s_waitcnt", "0xc07f") and not S.waits_for_scalar_loads("s_waitcnt", "0xc17f")     # (raw: lgkmcnt in bits 11:8)


def test_scalar_loads_of_the_shipped_sweeps_are_waited_for_on_every_path():
    """rt_trace_{parity,fast}_g request four records with s_load_dwordx16 in one asm statement and wait for them in another
    (rt_trace.inc.h request_four_uniform / arrived): the compiler sees the sixteen registers as defined at the request.  On every
    path from each such load -- fall-through, both sides of each branch, backward too -- an s_waitcnt lgkmcnt(0) must come before any
    instruction that names one of them, before the program ends and before the load is reached again.  Read from the product library's
    gfx950 code objects; each kernel holds at least one such load (four today: two pipelined pairs), so the test is not vacuous."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scalar_load_paths as S
    kernels = S.disassemble(api.lib_path())
    for name in ("rt_trace_parity_g", "rt_trace_fast_g"):
        n, bad = S.check_kernel(kernels[name])
        assert n >= 1, name
        assert bad == [], (name, bad[:5])
