"""The ray sets and the checks of tests/test_gpu_fast_walk.py, proved without a GPU (tests/_walk_probe.py): both arms of
tests/walk_probe.hip cross-compile for gfx950 with the rays kernel free of scratch; the binary32 restatement of the two sweeps
(pairs32, scene_from_pairs) passes the checks the fast walk and the fast sweep face, under K.exact(), on every scene and ray set, inside
the caps and not vacuously; and a ray with a NaN or infinite component hits nothing in binary32.  Run with -s for the figures."""
import numpy as np
import pytest

import _fast_reference as R
import _walk_probe as WP
from raytracing_simple_amd import _build

F = np.float32
SCENES = WP.walk_scenes()


@pytest.fixture(scope="module")
def probe_builds(tmp_path_factory):
    out = tmp_path_factory.mktemp("walk_probe")
    return {arm: R.build_probe(out, fast=(arm == "fast"), source="walk_probe") for arm in ("fast", "control")}


@pytest.mark.parametrize("arm", ["fast", "control"])
def test_walk_probe_cross_compiles_for_gfx950_without_scratch(probe_builds, arm):
    meta = _build.kernel_metadata(probe_builds[arm])
    assert sorted(meta) == ["rt_trace_walk_probe", "rt_walk_rays_probe"]
    m = meta["rt_walk_rays_probe"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m


def _sweeps32(rays7, table):
    """both sweeps of every ray in correctly rounded binary32, 1024 rays at a time"""
    parts = []
    for a in range(0, len(rays7), 1024):
        p = R.pairs32(rays7[a:a + 1024], table)
        parts.append(R.scene_from_pairs(p["t"], p["hit"], rays7[a:a + 1024, 6]))
    return {key: np.concatenate([q[key] for q in parts]) for key in ("t", "id", "first")}


CASES = [(scene, set_name) for scene in SCENES for set_name in WP.set_names(scene)]


@pytest.mark.parametrize("scene,set_name", CASES, ids=["%s-%s" % c for c in CASES])
def test_ray_set_against_binary64_with_correctly_rounded_binary32(scene, set_name):
    sph = SCENES[scene][0]
    table = R.table_of(sph)
    rays7 = WP.ray_sets(scene)[set_name]
    got = _sweeps32(rays7, table)
    tot = WP.check_judged(scene + "/" + set_name, {"binary32": got}, rays7, table, R.K.exact(), tie=(set_name == "shadow"))["binary32"]
    WP.check_caps(scene + "/" + set_name, set_name, tot)
    assert tot["hits"] > 1000 and tot["blocked"] > 1000, (scene, set_name, tot)
    # what binary64 cannot judge: nothing with a NaN or an infinite component hits anything
    odd = WP.not_a_number_or_infinite(rays7)
    assert (got["t"][odd] == R.T_NONE).all() and (got["first"][odd] == len(table)).all(), (scene, set_name)
    if set_name == "adversarial":
        assert odd.sum() > 500 and (~WP.judged(rays7) & ~odd).sum() > 300, (int(odd.sum()), int((~WP.judged(rays7) & ~odd).sum()))


@pytest.mark.parametrize("what", ["a dropped leaf", "a lost blocker"])
def test_a_walk_that_loses_one_decided_ray_in_a_thousand_fails(what):
    """what the PSNR gates let through: four of 4096 camera rays on random_spheres(256) answered as a walk would that skipped the leaf of
    the winner (the next sphere behind it, or a miss) or of the first blocker -- the checks the fast walk faces must refuse it"""
    scene, set_name = "random256", "camera"
    table = R.table_of(SCENES[scene][0])
    rays7 = WP.ray_sets(scene)[set_name]
    p = R.pairs32(rays7, table)
    got = R.scene_from_pairs(p["t"], p["hit"], rays7[:, 6])
    s = R.scene64(R.pairs64(rays7, table, R.K.exact()), rays7[:, 6])
    rows = np.arange(len(rays7))
    if what == "a dropped leaf":
        pick = np.nonzero(s["id_decided"] & s["any_hit"])[0][::800][:4]
        hit = p["hit"].copy()
        hit[pick, got["id"][pick]] = False
        bad = R.scene_from_pairs(p["t"], hit, rays7[:, 6])
        got = {"t": np.where(np.isin(rows, pick), bad["t"], got["t"]), "id": np.where(np.isin(rows, pick), bad["id"], got["id"]), "first": got["first"]}
    else:
        pick = np.nonzero(s["first_decided"] & (s["first"] < len(table)))[0][::800][:4]
        got = dict(got, first=np.where(np.isin(rows, pick), len(table), got["first"]))
    assert len(pick) == 4
    with pytest.raises(AssertionError, match="away from a tie"):
        WP.check_judged("tampered", {"binary32": got}, rays7, table, R.K.exact(), tie=False, verbose=False)
