"""Feature planes through the hierarchy (include/rt_api.h "feature planes", csrc/rt_instance.h features_form), the part that needs no device: the
symbols and bindings; the rule that says which kernel a call gets, compiled with the host compiler and run under the sanitizers as a program of its
own (tools/sanitize/features_main.cpp); and the scenes of tests/test_gpu_features_walk.py, each shown to contain what it is there for -- on the
hierarchy's host work (rt_bvh_host.cpp: which records repeat an earlier one, which stay outside the tree) and on rt_features_planes."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _features_walk as W
from raytracing_simple_amd import _build, api
from test_features_cpu import MISS, distances_restated, rays_restated

ROOT = W.ROOT
CASES = ["no_hierarchy_is_swept", "count_either_side_of_the_threshold", "placements_either_side_of_the_lds_limits", "render_knobs_change_nothing", "forced_forms"]


def test_the_symbols_and_bindings_exist():
    lib = api.load_library()
    assert "rt_last_features_kernel" in api.SYMBOLS and callable(lib.rt_last_features_kernel)
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    assert lib.rt_last_features_kernel(None) == b""
    assert callable(api.RtContext.last_features_kernel)
    assert "rt_debug_set_features_form" in api.DEBUG_SYMBOLS and "rt_debug_set_features_form" not in api.SYMBOLS
    assert not hasattr(lib, "rt_debug_set_features_form")                 # the product library does not export it ...
    assert callable(api.load_library(diag=True).rt_debug_set_features_form)      # ... the diagnostics library does
    assert api.load_library(diag=True).rt_last_features_kernel(None) == b""


@functools.lru_cache(maxsize=None)
def program(tmp):
    exe = os.path.join(tmp, "features_san")
    # (the sanitizers' runtimes linked INTO the program, as tests/test_instance_cpu.py builds its own)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), os.path.join(ROOT, "tools", "sanitize", "features_main.cpp"),
                    os.path.join(ROOT, "raytracing_simple_amd", "csrc", "rt_bvh_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return program(str(tmp_path_factory.mktemp("features_walk")))


def test_the_rule_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, r.stdout
    assert "features: clean" in lines, r.stdout


def host_plan(exe, sph, tmp_path):
    """What rt_bvh_host.cpp makes of the records: counts, the records that repeat an earlier one, the records outside the tree."""
    path = str(tmp_path / "records.bin")
    api.as_spheres(sph).tofile(path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.split("\n")
    head = lines[0].split()
    plan = {head[k]: float(head[k + 1]) if head[k] == "r_cut" else int(head[k + 1]) for k in range(0, len(head), 2)}
    plan["repeat"] = [int(ln.split()[1]) for ln in lines if ln.startswith("repeat ")]
    plan["outside"] = [int(ln.split()[1]) for ln in lines if ln.startswith("outside ")]
    assert plan["records"] == len(sph) and len(plan["repeat"]) == plan["repeats"] and len(plan["outside"]) == plan["always"]
    return plan


def nearest_two(sph, cam, w, h):
    """Per pixel (image rows): the two smallest non-zero distances of rule 11 and the records they belong to, lowest index first among equals."""
    o, d = rays_restated(cam, w, h)
    with np.errstate(all="ignore"):
        dist = distances_restated(api.as_spheres(sph), o, d).astype(np.float64)
    dist[~(dist > 0)] = np.inf                                # misses and NaNs
    order = np.argsort(dist, axis=0, kind="stable")[:2]
    return np.take_along_axis(dist, order, 0), order


@pytest.mark.parametrize("name", W.SCENES)
def test_every_scene_contains_what_it_is_there_for(name, exe, tmp_path):
    w, h = 41, 23
    sph, cam = W.scene(name, w, h)
    plan = host_plan(exe, sph, tmp_path)
    assert plan["tree"] >= W.BVH_MIN                          # the scene gets a hierarchy
    feat = api.features_planes(sph, cam, w, h)
    ids = feat[..., 7].view(np.uint32)
    in_tree = lambda k: k not in plan["outside"] and k not in plan["repeat"]      # noqa: E731
    if name in ("two_sizes", "doubled", "nonfinite"):
        assert plan["always"] >= 3 and all(k in plan["outside"] for k in (64, 65, 66))     # a non-empty always-list: the three large spheres
        seen = set(int(v) for v in np.unique(ids))
        assert seen & set(plan["outside"]) and any(in_tree(k) for k in seen - {MISS}) and MISS in seen    # always-list, tree and sky are all seen
    if name == "doubled":
        assert plan["repeats"] == 8 and plan["repeat"] == list(range(67, 75))
        near, who = nearest_two(sph, cam, w, h)
        tie = np.isfinite(near[0]) & (near[0] == near[1])
        assert tie.sum() > 20                                  # pixels whose two nearest records tie exactly ...
        assert (who[0][tie] < 67).all() and (who[1][tie] >= 67).all()
        assert np.array_equal(ids[::-1][tie], who[0][tie].astype(np.uint32))     # ... and rule 11 picks the lower index
        assert ((who[0] == 64) & tie).any() and (who[0][tie] < 64).any()          # ties on the always-list and in the tree
    if name == "smallest":
        assert plan == {**plan, "records": W.BVH_MIN, "tree": W.BVH_MIN, "always": 0, "repeats": 0}
        assert (ids == MISS).any() and len(np.unique(ids)) > 20
    if name == "inside":
        k = int(np.argmax(sph["rad"][:64]))
        assert in_tree(k) and np.allclose(cam[0:3], sph["p"][k]) and sph["rad"][k] > 0.2     # the camera, and every ray's origin 0.1 further, inside a tree sphere
        assert (ids == k).all() and (feat[..., 6] < 2 * sph["rad"][k]).all()
    if name == "away":
        assert (ids == MISS).all()                            # pixels that miss everything: all of them
    if name == "nonfinite":
        assert 10 in plan["outside"] and in_tree(20) and plan["always"] == 4
        assert not (ids == 10).any()
    if name == "camera_nonfinite":
        with np.errstate(all="ignore"):
            o, d = rays_restated(cam, w, h)
        assert not np.isfinite(d).all(axis=-1).any()          # no ray has a finite direction


def test_the_large_scenes_reach_both_builders(exe, tmp_path):
    for n in (1600, 8200):
        sph, _, _ = W.many(n)
        plan = host_plan(exe, sph, tmp_path)
        assert plan["always"] >= 1 and plan["tree"] + plan["always"] == n
        assert (128 <= plan["tree"] <= 8192) == (n == 1600)   # tools/bvh_check.py builder_reached: shaped on the device by area / halved on the host


def test_lds_of_restates_features_lds(exe):
    """The helper the GPU tests force placements with, against csrc/rt_instance.h features_lds itself."""
    for tree in ((129, 1033, 9), (7, 56, 4), (9, 75, 5), (1, 8, 1), (1025, 8201, 22), (32768, 262145, 40)):
        r = subprocess.run([exe, "lds"] + [str(v) for v in tree], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert tuple(int(v) for v in r.stdout.split()) == W.lds_of(*tree), tree
