"""Which kernel instance a launch gets (csrc/rt_instance.h: Knobs, SceneFacts, pick_shape, instance_lds) on the host alone:
tools/sanitize/instance_main.cpp -- the thresholds at which a scene changes instance, workgroup shape or what it stages, each from one side and from the
other, the LDS of every table kind and its refusals, the mode's meaning, the filling of Choice::Facts, and the real scenes of
profiles/r29_instance_facts.jsonl with the kernels the library picked for them -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a
program of its own.  No device: the rule holds no HIP.  The expectations are literals in the program, the arithmetic beside them."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["small_scene_plain_w1",
         "coop_from_twelve",
         "w1_boundary_moves_with_the_pass_count",
         "materials_leave_lds_at_24k",
         "sweep_leaves_lds_at_40k",
         "hierarchy_roles",
         "recorded_scenes_get_their_kernels",
         "lds_per_table_kind",
         "mode_said_once",
         "choice_facts_from_knobs"]


def test_instance_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "instance_san")
    # (the sanitizers' runtimes linked INTO the program: it then starts whatever else its environment loads into a process ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sanitize", "instance_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr                     # no report of either sanitizer
    lines = r.stdout.split("\n")
    for case in CASES:                                  # every case ran and held
        assert "ok " + case in lines, r.stdout
    assert "instance: clean" in lines, r.stdout


def test_the_program_carries_the_recorded_rows():
    """The rows of recorded_scenes_get_their_kernels are the rows of profiles/r29_instance_facts.jsonl, number for number."""
    src = open(os.path.join(ROOT, "tools", "sanitize", "instance_main.cpp")).read()
    rows = [json.loads(line) for line in open(os.path.join(ROOT, "profiles", "r29_instance_facts.jsonl"))]
    assert len(rows) == 8
    for r in rows:
        facts = ("tree(%d, %d, %d, %d, %d)" % (r["n_spheres"], r["n_lights"], r["n_leaves"], r["n_slots"], r["stack_depth"]) if r["has_hierarchy"]
                 else "flat(%d, %d)" % (r["n_spheres"], r["n_lights"]))
        want = '{ "%s", %s, %d, Form::%s, "%s", ' % (r["scene"], facts, r["passes"], r["form"], r["kernel"])
        assert want in src, want
        assert r["n_top"] == 0 and r["packed_at"] == 0          # (the product's layout: what tree() and flat() leave)
    assert len(re.findall(r'^        \{ "', src, flags=re.M)) == len(rows)
