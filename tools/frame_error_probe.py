#!/usr/bin/env python3
"""Measurements of the frame-error calls (include/rt_api.h "frame error on the device"), one JSON record each, stamped with rt_build_id():

    python tools/frame_error_probe.py [--repeats 20] [--bench NEW.jsonl PARENT.jsonl [--bench-only]] >> profiles/rNN_frame_error.jsonl

  compare_time   device time of rt_compare_async between two HIP events on the caller's stream, at 800x600 and 1920x1080, with and
                 without the tile map (median of the repeats after three warm-up calls), beside the wall time of the host route it
                 replaces: two rt_read_pixels and host.psnr.  The frames are two 8-pass renders of the Demo scene on seed streams 1 and 2.
  pair_offset    the Demo scene at 800x600, N = 8, 16, 32, 64 passes per half on seed streams 1 and 2: the PSNR BETWEEN the halves (what
                 rt_render_converged stops on) and the PSNR of the merged 2N-pass frame against a 1024-pass frame of the default
                 stream.  Their difference is what a host may add to the pair figure.
  bench          with --bench: the flagship figure of bench.py (its JSON result lines, one per run, kept in two files) of this library
                 beside the parent commit's, measured in the same visit -- no render kernel differs, so they should agree within
                 run-to-run noise."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_simple_amd import api, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--bench", nargs=2, metavar=("NEW", "PARENT"), default=None)
ap.add_argument("--bench-only", action="store_true", help="with --bench: that record alone (needs no device)")
args = ap.parse_args()
WARM = 3
sph = host.demo_scene()


def context(w, h, stream_id=0):
    c = api.RtContext(w, h)
    c.set_scene(sph)
    c.set_camera(host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h))
    if stream_id:
        c.seed_stream(stream_id, c.stream)
    return c


def spread(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def compare_time():
    import torch
    rec = {"record": "compare_time", "scene": "demo", "passes_per_frame": 8, "repeats": args.repeats, "sizes": {}, "build_id": api.build_id()}
    stream = torch.cuda.Stream()
    for w, h in ((800, 600), (1920, 1080)):
        with context(w, h, 1) as a, context(w, h, 2) as b:
            a.render_pass(8)
            b.render_pass(8)
            ty, tx = a.compare_tiles()
            res = torch.zeros(12, dtype=torch.int32, device="cuda")
            tiles = torch.zeros((ty, tx), dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            size = {"bytes_read": 8 * w * h, "tiles": ty * tx}
            for name, tptr in (("device_ms", None), ("device_ms_with_tile_map", tiles.data_ptr())):
                ms = []
                for r in range(WARM + args.repeats):
                    e0.record(stream)
                    a.compare_async(b, res.data_ptr(), tptr, stream.cuda_stream)
                    e1.record(stream)
                    stream.synchronize()
                    if r >= WARM:
                        ms.append(e0.elapsed_time(e1))
                size[name] = spread(ms)
            err = api.FrameError.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
            ms = []
            for r in range(WARM + args.repeats):
                t0 = time.perf_counter()
                psnr = host.psnr(a.read_pixels(), b.read_pixels())
                if r >= WARM:
                    ms.append((time.perf_counter() - t0) * 1e3)
            size["host_route_wall_ms"] = spread(ms)
            ms = []
            for r in range(WARM + args.repeats):                # the blocking call as a host sees it: queue, kernel, 48 bytes back
                t0 = time.perf_counter()
                blocking = a.compare(b)
                if r >= WARM:
                    ms.append((time.perf_counter() - t0) * 1e3)
            size["rt_compare_wall_ms"] = spread(ms)
            assert blocking == err and abs(api.error_psnr(err) - psnr) <= 1e-9, (blocking, err, psnr)
            size["pair_psnr_db"] = round(psnr, 3)
            size["GB_per_s"] = round(8 * w * h / (size["device_ms"]["median"] * 1e6), 1)
            rec["sizes"]["%dx%d" % (w, h)] = size
    return rec


def pair_offset():
    w, h = 800, 600
    rec = {"record": "pair_offset", "scene": "demo", "w": w, "h": h, "reference_frame": "1024 passes, default stream", "rows": [],
           "build_id": api.build_id()}
    with context(w, h) as truth:
        truth.render_pass(1024)
        for n in (8, 16, 32, 64):
            with context(w, h, 1) as a, context(w, h, 2) as b:
                a.render_async(n, a.stream)
                b.render_async(n, b.stream)
                pair = a.compare(b)
                half = [x.compare(truth) for x in (a, b)]
                a.merge([b], a.stream)
                merged = a.compare(truth)
                assert a.current_sample == 2 * n
                assert abs(api.error_psnr(merged) - host.psnr(a.read_pixels(), truth.read_pixels())) <= 1e-9
                row = {"passes_per_half": n, "pair_psnr_db": round(api.error_psnr(pair), 3),
                       "half_vs_reference_db": [round(api.error_psnr(e), 3) for e in half],
                       "merged_vs_reference_db": round(api.error_psnr(merged), 3)}
                row["merged_minus_pair_db"] = round(row["merged_vs_reference_db"] - row["pair_psnr_db"], 3)
                rec["rows"].append(row)
    return rec


def bench(new_path, parent_path):
    """The result lines bench.py printed for this library and for the parent's, runs alternating in one visit, one line per run."""
    def runs(path):
        lines = [json.loads(line) for line in open(path) if line.lstrip().startswith("{")]
        ms = [d["ms_per_step"] for d in lines]
        return {"ms_per_step": ms, "median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "value": [d["value"] for d in lines]}
    new, parent = runs(new_path), runs(parent_path)
    return {"record": "bench", "command": "python bench.py --gpus 1 --steps 20 --warmup 5", "workload": "C2: Demo scene, 1920x1080, 64 spp, parity",
            "protocol": "both libraries in one visit to one MI355X, alternating (this, parent)", "this": new, "parent": parent,
            "median_difference_ms": round(new["median_ms"] - parent["median_ms"], 4), "build_id": api.build_id()}


for make in (() if args.bench_only else (compare_time, pair_offset)):
    print(json.dumps(make()), flush=True)
if args.bench:
    print(json.dumps(bench(*args.bench)), flush=True)
