"""Writes profiles/r26_fast_first_hit.jsonl on a machine with the device: what tests/test_gpu_fast_first_hit.py and
tests/test_gpu_fast_walk.py print with -s, as records stamped with the build id -- per scene and instance of the first-hit frames the
decided / excluded counts and the largest observed / bound of |n.d|; per scene, ray set, tree and arm of the walk probe the counts, the
largest observed / bound of t, and how many judged rays the fast walk and the fast sweep answer with different t bits.  Informational:
no test reads the file.    python tools/record_fast_first_hit.py [out.jsonl]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import _fast_reference as R  # noqa: E402
import _first_hit as FH  # noqa: E402
import _walk_probe as WP  # noqa: E402
import test_gpu_fast_first_hit as A  # noqa: E402
import test_gpu_fast_walk as B  # noqa: E402
from raytracing_simple_amd import api  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FH.RECORDS
    k = R.K.measured()
    assert k is not None, "profiles/r20_fast_blocks.jsonl first (tools/measure_fast_blocks.py)"
    recs = []
    for name, knobs, kernel in A.CASES:
        colors, rendered_by = FH.render(name, knobs=knobs)
        assert rendered_by == kernel
        res = FH.check_frame("%s / %s" % (kernel, name), colors, FH.reference(name, True))
        recs.append(dict(res, what="first_hit", scene=name, instance=kernel, library="diagnostics" if knobs else "product",
                         knobs=[s for s, _ in knobs], build_id=api.build_id(bool(knobs))))
    with tempfile.TemporaryDirectory() as tmp:
        probes = {arm: WP.WalkProbe(R.build_probe(tmp, fast=(arm == "fast"), source="walk_probe")) for arm in ("fast", "control")}
        for scene, set_name in B.CASES:
            assert B._control(probes, scene, set_name) is None
            rays7, table = WP.ray_sets(scene)[set_name], R.table_of(B.SCENES[scene][0])
            for tree in B.TREES:
                out4 = B.runs(probes, scene)[tree, set_name]["fast"]
                walk, sweep = WP.answers(out4, 0), WP.answers(out4, 2)
                tots = WP.check_judged(scene + "/" + set_name, {"walk": walk, "sweep": sweep}, rays7, table, k, tie=(set_name == "shadow"))
                both = WP.judged(rays7) & walk["hit"] & sweep["hit"]
                recs.append({"what": "fast_walk_rays", "scene": scene, "rays": set_name, "tree": tree, "walk": tots["walk"], "sweep": tots["sweep"],
                             "cannot_be_judged": int((~WP.judged(rays7)).sum()), "both_hit": int(both.sum()),
                             "different_t_bits": int((walk["t_bits"] != sweep["t_bits"])[both].sum()), "build_id": api.build_id(True)})
    with open(out_path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    print("%d records -> %s" % (len(recs), out_path))


if __name__ == "__main__":
    main()
