"""Writes profiles/r28_shadow_frames.jsonl: what tests/test_gpu_fast_shadow.py prints with -s, as records stamped with the build id --
per case the instance, the library, the population, the decided, lit and dark-by-blocker counts, the share of answers the exclusion rule
leaves out under K.exact() and under K.measured(), and the largest observed / bound of 8 k.  Informational: no test reads the file.
    python tools/record_shadow_frames.py [out.jsonl]                  on a machine with the device
    python tools/record_shadow_frames.py --save DIR                   on the device: only render, keep the colour planes (DIR/<case>.npy) and kernel names
    python tools/record_shadow_frames.py [out.jsonl] --frames DIR     anywhere: the figures of the planes kept that way"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import _fast_reference as R  # noqa: E402
import _shadow_frames as SF  # noqa: E402
import test_gpu_fast_shadow as A  # noqa: E402
from raytracing_simple_amd import api  # noqa: E402


def main():
    args = sys.argv[1:]
    save = frames = None
    if "--save" in args:
        save = args.pop(args.index("--save") + 1)
        args.remove("--save")
    if "--frames" in args:
        frames = args.pop(args.index("--frames") + 1)
        args.remove("--frames")
    out_path = args[0] if args else SF.RECORDS
    if save:
        os.makedirs(save, exist_ok=True)
        names = {}
        for case in A.CASES:
            colors, names[A._case_id(case)], _, _ = SF.render(case[0], knobs=case[1])
            np.save(os.path.join(save, A._case_id(case) + ".npy"), colors)
        json.dump({"kernels": names, "build_id": {"product": api.build_id(False), "diagnostics": api.build_id(True)}}, open(os.path.join(save, "kernels.json"), "w"))
        print("%d frames -> %s" % (len(names), save))
        return
    assert R.K.measured() is not None, "profiles/r20_fast_blocks.jsonl first (tools/measure_fast_blocks.py)"
    kept = json.load(open(os.path.join(frames, "kernels.json"))) if frames else None
    recs = []
    for case in A.CASES:
        name, knobs, kernel = case
        if frames:
            colors, rendered_by = np.load(os.path.join(frames, A._case_id(case) + ".npy")), kept["kernels"][A._case_id(case)]
            build = kept["build_id"]["diagnostics" if knobs else "product"]
        else:
            colors, rendered_by, _, _ = SF.render(name, knobs=knobs)
            build = api.build_id(bool(knobs))
        assert rendered_by == kernel, (case, rendered_by)
        res = SF.check_frame("%s / %s" % (kernel, name), colors, SF.reference(name, True))
        exact = SF.figures(SF.reference(name, False))
        recs.append({"what": "shadow_frame", "scene": name, "instance": kernel, "library": "diagnostics" if knobs else "product", "knobs": [s for s, _ in knobs],
                     "population": res["population"], "answers": res["answers"], "decided": res["decided"], "lit": res["lit"],
                     "dark_by_blocker": res["dark_by_blocker"], "blockers": len(res["blockers"]),
                     "excluded_share_measured": res["excluded"] / max(res["answers"], 1), "excluded_share_exact": exact["excluded"] / max(exact["answers"], 1),
                     "ratio_8k": res["ratio"], "build_id": build})
    with open(out_path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    print("%d records -> %s" % (len(recs), out_path))


if __name__ == "__main__":
    main()
