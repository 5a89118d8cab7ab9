"""(ray, sphere) pairs and the two sweeps of fast mode on the device against binary64: tests/fast_probe.hip's probe_pairs (hit_pre,
hit_roots, hit_post) and probe_scene (sweep_closest, sweep_any over a table staged in LDS), on the Demo scene (its radius-1000 ground
is the cancellation case of b^2 - op.op + r^2), the mirror box, 256 random spheres and the eight adversarial fixtures, six seeded ray
families of 4096 rays each.  References, envelopes, the exclusion rule and its cap: tests/_fast_reference.py; the same assertions run
on correctly rounded binary32 without a GPU in tests/test_fast_reference_cpu.py.  The control arm of the probe (parity flags) must
equal the binary32 restatement bit for bit first.  Run with -s for observed / bound per family."""
import functools

import numpy as np
import pytest

import _fast_reference as R

pytestmark = pytest.mark.gpu
CONTROL = {}


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    out = tmp_path_factory.mktemp("fast_probe")
    return {arm: R.Probe(R.build_probe(out, fast=(arm == "fast"))) for arm in ("fast", "control")}


@pytest.fixture(scope="module")
def measured():
    k = R.K.measured()
    if k is None:
        pytest.skip("not measured yet: profiles/r20_fast_blocks.jsonl has no record (tools/measure_fast_blocks.py writes it)")
    return k


@functools.lru_cache(maxsize=None)
def family_rays(fam):
    """[(scene name, table, rays)] of one family over every scene"""
    return [(name, R.table_of(sph), R.family(fam, sph, orig, target, 100 * n + R.FAMILIES.index(fam)))
            for n, (name, sph, orig, target) in enumerate(R.scenes_of_the_rays())]


def _control(probes, fam):
    if fam in CONTROL:
        return CONTROL[fam]
    bad = None
    for name, tab, rays in family_rays(fam):
        got, want = probes["control"].pairs(rays, tab), R.pairs32(rays, tab)
        checks = [("b", R.bits_equal(got["b"], want["b"])), ("det", R.bits_equal(got["det"], want["det"])), ("hit", got["hit"] == want["hit"]),
                  ("t", R.bits_equal(got["t"], want["t"]) | ~want["hit"]), ("hit_post", R.bits_equal(got["t_post"], want["t_post"]))]
        sc, ws = probes["control"].scene(rays, tab), R.scene_from_pairs(want["t"], want["hit"], rays[:, 6])
        checks += [("closest t", R.bits_equal(sc["t"], ws["t"])), ("closest index", sc["id"] == ws["id"]), ("first blocker", sc["first"] == ws["first"])]
        for what, same in checks:
            if not same.all():
                bad = bad or "%s/%s %s: %d of %d differ" % (name, fam, what, int((~same).sum()), same.size)
    CONTROL[fam] = bad
    return bad


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_control_arm_is_the_binary32_restatement_bit_for_bit(probes, fam):
    assert _control(probes, fam) is None


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_fast_rays_against_binary64(probes, measured, fam):
    bad = _control(probes, fam)
    if bad:
        pytest.fail("the control arm of the probe does not reproduce parity arithmetic (%s): the probe is wired wrong, the fast arm's results mean nothing" % bad)
    tot = {"pairs": 0, "skipped": 0, "hits": 0, "misses": 0, "rays": 0, "id_skipped": 0, "first_skipped": 0}
    for name, tab, rays in family_rays(fam):
        p = R.pairs64(rays, tab, measured)
        res = R.check_pairs(name + "/" + fam, probes["fast"].pairs(rays, tab), p)
        sc = R.check_scene(name + "/" + fam, probes["fast"].scene(rays, tab), p, rays[:, 6], tie=(fam == "shadow"))
        for key in tot:
            tot[key] += res.get(key, 0) + sc.get(key, 0)
    R.cap(fam + " pairs", tot["skipped"], tot["pairs"])
    if fam not in ("grazing", "shadow"):       # (those two are built AT ties: _fast_reference.check_ray_totals)
        R.cap(fam + " closest hits", tot["id_skipped"], tot["rays"])
        R.cap(fam + " first blockers", tot["first_skipped"], tot["rays"])
    R.check_ray_totals(fam, tot)
