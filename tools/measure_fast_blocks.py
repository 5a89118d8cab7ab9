#!/usr/bin/env python3
"""Measure what the fast-mode tests cannot derive, on the device, against binary64 (tests/_fast_reference.py observe_blocks): the ulp
accuracy of v_rcp_f32 / v_rsq_f32 / v_sqrt_f32, the absolute error of v_sin_f32 / v_cos_f32 over the 2^23 arguments the renderer forms
and |sin^2 + cos^2 - 1|, and to_int's delta.  One record per op, stamped with the library's build id; then the observed / bound ratios of
the derived envelopes (rays, sweeps, shading steps) with twice those maxima in them, the largest first.

    python tools/measure_fast_blocks.py [--out profiles/r20_fast_blocks.jsonl]

The tests assert twice the observed maximum: room for another stepping of the same instruction, not for another algorithm."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_fast_blocks.jsonl"))
    args = ap.parse_args()
    import _fast_reference as R
    from raytracing_simple_amd import api
    with tempfile.TemporaryDirectory() as tmp:
        probe = R.Probe(R.build_probe(tmp, fast=True))
        control = R.Probe(R.build_probe(tmp, fast=False))
        rays = R.family("camera", *R.scenes_of_the_rays()[0][1:], 1)
        tab = R.table_of(R.scenes_of_the_rays()[0][1])
        same = R.bits_equal(control.pairs(rays, tab)["det"], R.pairs32(rays, tab)["det"]).all()
        if not same:
            raise SystemExit("the control arm does not reproduce the binary32 restatement: the probe is wired wrong, nothing measured")
        records = R.observe_blocks(probe)
        by = {r["op"]: r["observed_max"] for r in records}
        k = R.K(True, 2 * by["v_sqrt_f32"], 2 * by["v_rcp_f32"], 2 * by["v_rsq_f32"], 2 * max(by["v_sin_f32"], by["v_cos_f32"]))
        ratios = {}
        for n_scene, (name, sph, orig, target) in enumerate(R.scenes_of_the_rays()):
            t = R.table_of(sph)
            for fam in R.FAMILIES:
                r = R.family(fam, sph, orig, target, 100 * n_scene + R.FAMILIES.index(fam))
                res = R.check_pairs(name + "/" + fam, probe.pairs(r, t), R.pairs64(r, t, k), verbose=False)
                for q in ("b", "det", "t"):
                    ratios[q + " " + fam] = max(ratios.get(q + " " + fam, 0.0), res[q])
        for what in range(5):
            rec, cam, extra = R.shade_inputs(what, np.random.default_rng(40 + what))
            ratios["shade step %d" % what] = R.check_shade(what, probe.shade(what, rec, cam), rec, extra, k, verbose=False)
        worst = max(ratios, key=ratios.get)
        records.append({"op": "envelopes", "observed_max": ratios[worst], "unit": "observed / bound, the bound with twice the measured maxima above in it",
                        "input": worst, "inputs": {q: round(v, 4) for q, v in sorted(ratios.items(), key=lambda kv: -kv[1])}})
    bid = api.build_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in records:
            f.write(json.dumps(dict(r, build_id=bid)) + "\n")
            print(r["op"], r["observed_max"], r["input"] if r["op"] != "envelopes" else r["input"])


if __name__ == "__main__":
    main()
