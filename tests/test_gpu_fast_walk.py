"""The hierarchy walk's SOURCE under the fast flags, ray by ray against binary64, for closest-hit and shadow rays (tests/_walk_probe.py,
tests/walk_probe.hip: csrc/rt_walk.inc.h's rays kernel -- the walk, then the plain sweep, one lane per ray -- built with
rt_kernel_fast.hip's flags, and with parity's as the control arm).  The derivation of the walk's pad (rt_walk.inc.h, "walking the
hierarchy") is written for binary32 rounded after every operation and a correctly rounded root; fast mode fuses and uses v_sqrt_f32.
This is what checks that the pad's slack covers it.

  1. CONTROL ARM: on every ray set its four words equal rt_debug_walk_rays of the diagnostics library on the same context bit for bit,
     and its walk equals its sweep in all four words.  Otherwise the probe is wired wrong and the fast arm means nothing.
  2. FAST ARM, rays binary64 can judge: the walk's answer AND the sweep's each go through R.check_scene against
     pairs64(..., K.measured()) -- closest hits by index and by t within t_env, shadow rays by first blocker (the shadow family with
     tie=True); the 2 % cap except for the sets built at ties (_walk_probe.check_caps).
  3. FAST ARM, rays binary64 cannot judge (a non-finite component, or a direction further than 1e-3 from unit length: the walk gives them
     an infinite pad and must visit everything): the walk's hit / miss and index words equal the sweep's (the t bits are not compared:
     the two inline sites may fuse differently); a ray with a NaN or an infinite component hits nothing in either.
  4. NOT VACUOUS: per ray set more than a thousand decided hits and decided blocked shadow rays.
Ray sets: the six R.FAMILIES (4096 rays each) on random_spheres(256) and (1024); 12 000 adversarial rays (tests/_adversarial_rays.py) on
random_spheres(1024), mirror_box(120) and _adversarial(3).  Trees: the default build and rt_debug_set_tree_shape(ctx, 0).  The same checks
on correctly rounded binary32 without a GPU: tests/test_fast_walk_cpu.py.  Run with -s for the figures (profiles/r26_fast_first_hit.jsonl),
among them how many rays the fast walk and the fast sweep answer with different t bits (informational)."""

import numpy as np
import pytest

import _fast_reference as R
import _walk_probe as WP
from raytracing_simple_amd import api

pytestmark = pytest.mark.gpu

SCENES = WP.walk_scenes()
CASES = [(scene, set_name) for scene in SCENES for set_name in WP.set_names(scene)]
IDS = ["%s-%s" % c for c in CASES]
TREES = {"default tree": None, "halved tree": 0}
_RUNS = {}


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    out = tmp_path_factory.mktemp("walk_probe")
    return {arm: WP.WalkProbe(R.build_probe(out, fast=(arm == "fast"), source="walk_probe")) for arm in ("fast", "control")}


@pytest.fixture(scope="module")
def measured():
    k = R.K.measured()
    if k is None:
        pytest.skip("not measured yet: profiles/r20_fast_blocks.jsonl has no record (tools/measure_fast_blocks.py writes it)")
    return k


def runs(probes, scene):
    """{(tree, set): {"library", "control", "fast": out4}} of one scene: one context per tree, every ray set through the library's own kernel
    and through both arms of the probe on that context's tables"""
    if scene in _RUNS:
        return _RUNS[scene]
    assert probes["fast"].fast and not probes["control"].fast
    sph = api.as_spheres(SCENES[scene][0])
    table = R.table_of(sph)
    out = {}
    for tree, shape in TREES.items():
        with api.RtContext(32, 32, diag=True) as ctx:
            if shape is not None:
                ctx._check(ctx._lib.rt_debug_set_tree_shape(ctx._h, shape))
            ctx._check(ctx._lib.rt_debug_set_bvh(ctx._h, 1, 152 * 1024))
            ctx.set_scene(sph)
            tr = WP.tree_of(ctx)
            for set_name, rays7 in WP.ray_sets(scene).items():
                rays8 = WP.both_kinds(rays7)
                with np.errstate(all="ignore"):
                    out[tree, set_name] = {"library": WP.library_answers(ctx, rays8), "control": probes["control"].rays(table, tr, rays8),
                                           "fast": probes["fast"].rays(table, tr, rays8)}
    _RUNS[scene] = out
    return out


def _control(probes, scene, set_name):
    for tree in TREES:
        r = runs(probes, scene)[tree, set_name]
        if not np.array_equal(r["control"], r["library"]):
            differ = np.nonzero((r["control"] != r["library"]).any(1))[0]
            return "%s/%s, %s: %d records differ from rt_debug_walk_rays, first %s" % (scene, set_name, tree, len(differ), differ[:4].tolist())
        c = r["control"]
        differ = np.nonzero((c[:, 0] != c[:, 2]) | (c[:, 1] != c[:, 3]))[0]
        if len(differ):
            return "%s/%s, %s: the control arm's walk differs from its sweep at %s" % (scene, set_name, tree, differ[:4].tolist())
    return None


@pytest.mark.parametrize("scene,set_name", CASES, ids=IDS)
def test_control_arm_is_the_library_s_own_rays_kernel_bit_for_bit(probes, scene, set_name):
    assert _control(probes, scene, set_name) is None


@pytest.mark.parametrize("scene,set_name", CASES, ids=IDS)
def test_fast_walk_and_fast_sweep_against_binary64(probes, measured, scene, set_name):
    bad = _control(probes, scene, set_name)
    if bad:
        pytest.fail("the control arm of the walk probe does not reproduce the library's kernel (%s): the probe is wired wrong, the fast arm's results mean nothing" % bad)
    rays7 = WP.ray_sets(scene)[set_name]
    table = R.table_of(SCENES[scene][0])
    gots = {}
    for tree in TREES:
        out4 = runs(probes, scene)[tree, set_name]["fast"]
        gots[tree + ", walk"], gots[tree + ", sweep"] = WP.answers(out4, 0), WP.answers(out4, 2)
    name = scene + "/" + set_name
    for label, tot in WP.check_judged(name, gots, rays7, table, measured, tie=(set_name == "shadow")).items():
        WP.check_caps(name + " " + label, set_name, tot)
        assert tot["hits"] > 1000 and tot["blocked"] > 1000, (name, label, tot)
    # the rays binary64 cannot judge: the walk visits everything, so it answers as the sweep does
    cannot, odd = ~WP.judged(rays7), WP.not_a_number_or_infinite(rays7)
    for tree in TREES:
        walk, sweep = gots[tree + ", walk"], gots[tree + ", sweep"]
        differ = cannot & ((walk["hit"] != sweep["hit"]) | (walk["id"] != sweep["id"]) | (walk["first"] != sweep["first"]))
        assert not differ.any(), (name, tree, "the walk differs from the sweep on rays with an infinite pad", np.nonzero(differ)[0][:4].tolist())
        for which, got in (("walk", walk), ("sweep", sweep)):
            assert not got["hit"][odd].any() and (got["first"][odd] == len(table)).all(), (name, tree, which, "a ray with a NaN or infinite component hit something")
        both = WP.judged(rays7) & walk["hit"] & sweep["hit"]
        print("%-40s %-14s cannot be judged %5d (not a number / infinite %4d)   walk and sweep hit with different t bits: %d of %d judged" % (
            name, tree, int(cannot.sum()), int(odd.sum()), int((walk["t_bits"] != sweep["t_bits"])[both].sum()), int(both.sum())))
    if set_name == "adversarial":
        assert odd.sum() > 500 and (cannot & ~odd).sum() > 300
