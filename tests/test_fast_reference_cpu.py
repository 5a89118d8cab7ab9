"""The references, envelopes and input families of the fast-mode tests, proved without a GPU: the same families and the same
assertions as tests/test_gpu_fast_blocks.py / test_gpu_fast_rays.py, with the ORACLE's binary32 results (orc_sphere_intersect,
orc_to_int, om_sinf / om_cosf) and the binary32 restatements of tests/_fast_reference.py in the device's place.  That shows that
the binary64 references are right, that the envelopes hold for correctly rounded binary32, and that the families stay inside the
exclusion rule's cap.  Both arms of the probe are also cross-compiled for gfx950 and must come out without scratch; and the bias
gate's preconditions (tests/test_gpu_fast_bias.py) are run on the oracle at a reduced pass count.  Run with -s for the figures."""
import ctypes as C

import numpy as np
import pytest

import _fast_reference as R
import _oracle as O
from raytracing_simple_amd import _build, api, host

F, D = np.float32, np.float64


# ---- the probe builds, both arms, without scratch ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_builds(tmp_path_factory):
    out = tmp_path_factory.mktemp("fast_probe")
    return {arm: R.build_probe(out, fast=(arm == "fast")) for arm in ("fast", "control")}


@pytest.mark.parametrize("arm", ["fast", "control"])
def test_probe_cross_compiles_for_gfx950_without_scratch(probe_builds, arm):
    meta = _build.kernel_metadata(probe_builds[arm])
    assert sorted(meta) == ["probe_eval_kernel", "probe_pairs_kernel", "probe_scene_kernel", "probe_shade_kernel"]
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


# ---- (ray, sphere) pairs -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ray_scenes():
    return R.scenes_of_the_rays()


def test_binary32_restatement_is_the_tile_test_s_discriminant_and_the_oracle_s_intersection(ray_scenes):
    from test_tile_candidates import discriminants
    lib = O.oracle()
    rng = np.random.default_rng(3)
    for name, sph, orig, target in ray_scenes[:5]:
        tab = R.table_of(sph)
        rays = R.family("camera", sph, orig, target, 1)[:512]
        got = R.pairs32(rays, tab)
        with np.errstate(all="ignore"):
            for i in range(len(sph)):
                assert R.bits_equal(got["det"][:, i], discriminants(rays[:, 0:3], rays[:, 3:6], tab[i, 0:3], tab[i, 3])).all(), (name, i)
        rec = O._as_spheres(sph)
        for r, s in zip(rng.integers(0, len(rays), 400), rng.integers(0, len(sph), 400)):
            o3, d3 = (C.c_float * 3)(*rays[r, 0:3]), (C.c_float * 3)(*rays[r, 3:6])
            want = F(lib.orc_sphere_intersect(C.c_void_p(rec[s:s + 1].ctypes.data), o3, d3))
            assert R.bits_equal(np.array([want]), got["t_post"][r:r + 1, s]).all(), (name, r, s, want, got["t_post"][r, s])


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_ray_family_against_binary64_with_correctly_rounded_binary32(ray_scenes, fam):
    """what tests/test_gpu_fast_rays.py asserts of the device, asserted of the binary32 restatement; the cap of the exclusion rule"""
    k = R.K.exact()
    tot = {"pairs": 0, "skipped": 0, "hits": 0, "misses": 0, "rays": 0, "id_skipped": 0, "first_skipped": 0}
    for n_scene, (name, sph, orig, target) in enumerate(ray_scenes):
        tab = R.table_of(sph)
        rays = R.family(fam, sph, orig, target, 100 * n_scene + R.FAMILIES.index(fam))
        p = R.pairs64(rays, tab, k)
        got = R.pairs32(rays, tab)
        res = R.check_pairs(name + "/" + fam, got, p)
        unit_d = np.abs(np.linalg.norm(rays[:, 3:6].astype(D), axis=1) - 1.0) < 1e-6
        fin = p["finite"] & unit_d[:, None]
        assert (p["det"].e[fin] <= R.closed_det_bound(p, tab)[fin] * (1 + 1e-5) + 1e-30).all(), name       # the running bound never exceeds the closed form
        sc = R.check_scene(name + "/" + fam, R.scene_from_pairs(got["t"], got["hit"], rays[:, 6]), p, rays[:, 6], tie=(fam == "shadow"))
        for key in tot:
            tot[key] += res.get(key, 0) + sc.get(key, 0)
    R.cap(fam + " pairs", tot["skipped"], tot["pairs"])
    assert tot["hits"] > 0 and tot["misses"] > 0
    if fam not in ("grazing", "shadow"):       # (those two are BUILT at ties -- of det and of max_t: see check_ray_totals)
        R.cap(fam + " closest hits", tot["id_skipped"], tot["rays"])
        R.cap(fam + " first blockers", tot["first_skipped"], tot["rays"])
    R.check_ray_totals(fam, tot)


# ---- scalar blocks ------------------------------------------------------------------------------------------------------------------
def test_to_int_reference_and_inputs():
    """parity's to_int against the binary64 one.  Parity's distance from a rounding boundary inside which the two may differ, derived:
    powf's result within 1 ulp of g <= 1 (2^-24 * 255 = 1.5e-5 after the scaling), the product and the sum round at half an ulp of 256
    (2 * 2^-17 = 1.5e-5), and the exponent 1/2.2f is 1.4e-8 from 1/2.2, which moves g by at most 1.4e-8 / (e * 0.4545) (0.3e-5 scaled):
    below 4e-5."""
    near, grid, edges = R.to_int_inputs()
    lib = O.oracle()
    assert len(near) > 255 * 100
    for name, v in (("near", near[::7]), ("grid", grid[::16]), ("edges", edges)):
        got = np.array([lib.orc_to_int(C.c_float(float(x))) for x in v], np.int64)
        want, dist = R.to_int64(v)
        assert (np.abs(got - want) <= 1).all(), name
        clear = dist > 4e-5
        assert np.array_equal(got[clear], want[clear]), name
        assert clear.mean() > 0.5, (name, clear.mean())
    want, _ = R.to_int64(edges)
    assert want.tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 255, 0, 0, 0, 255, 0, 0]


def test_sine_and_cosine_reference():
    u = (np.arange(0, 1 << 23, 64) / F(1 << 23)).astype(F)
    sn, cs = R.sincos32(u)
    es, ec = R.e_sincos(u, R.K.exact())
    worst = max(float(np.abs(sn.astype(D) - es.v).max()), float(np.abs(cs.astype(D) - ec.v).max()))
    print("parity sine / cosine of a draw: largest error %.3g, bound %.3g" % (worst, R.K.exact().sin_abs))
    assert worst <= R.K.exact().sin_abs


def test_square_roots_reciprocals_and_unit_vectors_in_binary32():
    rng = np.random.default_rng(11)
    k = R.K.exact()
    x = R.log_uniform(rng, -96, 127, 1 << 16)
    with np.errstate(all="ignore"):
        assert R.ulp_error(np.sqrt(x), np.sqrt(x.astype(D))).max() <= 0.5
        assert R.ulp_error(F(1) / x, 1.0 / x.astype(D)).max() <= 0.5
    a = (R.log_uniform(rng, np.log2(1e-6), np.log2(1e4), 3 * 4096).reshape(-1, 3) * rng.choice([-1, 1], (4096, 3))).astype(F)
    want = R.e_unit(R.e_vec(a), k)
    got = R.unit32(a)
    ratio = max(float((np.abs(got[:, c].astype(D) - want[c].v) / want[c].e).max()) for c in range(3))
    length_bound = np.sqrt(sum((np.abs(want[c].v) + want[c].e) ** 2 for c in range(3))) - 1.0
    off = np.abs(np.linalg.norm(got.astype(D), axis=1) - 1.0)
    print("unit(): observed / bound %.3f, largest | |unit(a)| - 1 | %.3g of %.3g allowed" % (ratio, off.max(), length_bound.max()))
    assert ratio <= 1.0 and (off <= length_bound).all() and length_bound.max() < 8 * R.U


@pytest.mark.parametrize("what", [0, 1, 2, 3, 4], ids=["camera", "bounce", "hit-record", "glass", "light"])
def test_shading_steps_against_binary64_with_correctly_rounded_binary32(what):
    rec, cam, extra = R.shade_inputs(what, np.random.default_rng(40 + what))
    got = R.shade32(what, rec, extra)
    R.check_shade(what, got, rec, extra, R.K.exact())
    if what == 1:
        assert ((got[:, 6:9].astype(D) * rec[:, 0:3].astype(D)).sum(1) >= 0).all()


# ---- the bias gate can see a bias (preconditions, on the oracle at a reduced pass count) -------------------------------------------
CPU_PASSES = 1024


@pytest.fixture(scope="module")
def oracle_frames():
    """glass_and_mirror at 41x23 on the oracle: the parity frames of the four streams and a maker of frames on the fast frame's stream"""
    name, maker, w, h = R.bias_scenes()[2]
    sph, orig, target = maker()
    cam = host.compute_camera(orig, target, w, h)

    def frame(spheres, stream=R.FAST_STREAM):
        return O.render(spheres, cam, w, h, CPU_PASSES, seeds_in=api.stream_seeds(stream, 2 * w * h))["pixels"]
    parity = [frame(sph, s) for s in R.PARITY_STREAMS]
    among = [O.psnr(parity[i], parity[j]) for i in range(4) for j in range(i + 1, 4)]
    return {"spheres": sph, "parity": parity, "among": among, "frame": frame}


def _gate(frames, spheres, label):
    against = [O.psnr(frames["frame"](spheres), f) for f in frames["parity"]]
    ok, thr = R.bias_gate(frames["among"], against)
    print("%s: D %.2f .. %.2f dB, threshold %.2f, F %s -> %s" % (
        label, min(frames["among"]), max(frames["among"]), thr, ["%.2f" % v for v in against], "passes" if ok else "FAILS"))
    return ok


def test_bias_gate_passes_an_honest_frame_on_the_oracle(oracle_frames):
    assert _gate(oracle_frames, oracle_frames["spheres"], "an independent stream")


@pytest.mark.parametrize("bias", ["glass-turned-diffuse", "emission-x1.10"])
def test_bias_gate_fails_a_biased_frame_on_the_oracle(oracle_frames, bias):
    """The preconditions of tests/test_gpu_fast_bias.py.  The 2 % brighter light the gate was asked to see it does not see at a pass count
    a test can afford (that module's docstring; printed below): 1.10 is what it resolves at 1024 and at 4096 passes."""
    sph = oracle_frames["spheres"]
    biased = R.glass_turned_diffuse(sph) if bias == "glass-turned-diffuse" else R.brighter_light(sph, 1.10)
    assert not _gate(oracle_frames, biased, bias)
    if bias != "glass-turned-diffuse":
        _gate(oracle_frames, R.brighter_light(sph, 1.02), "emission x 1.02 (below the gate's resolution)")
