"""What a context holds of its scene (csrc/rt_scene_state.h SceneState) on the host alone: tools/sanitize/scene_main.cpp -- which drives the record
through the transitions in the order the API's calls report them -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a
program of its own.  No device: the record holds no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["renderable_needs_scene_and_camera",
         "identical_set_scene_ends_the_features_only",
         "failed_upload_leaves_no_scene_and_refuses_updates",
         "updates_leave_tables_stale_until_a_rebuild_succeeds",
         "replaced_capacity_voids_hierarchy_and_flags_not_the_scene",
         "empty_flags_are_uploaded_once_after_a_scene_with_duplicates",
         "features_end_with_three_calls_and_nothing_else",
         "hierarchy_adopted_after_voided_reports_n_tree"]


def test_scene_state_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scene_san")
    # (the sanitizers' runtimes linked INTO the program: it then starts whatever else its environment loads into a process ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sanitize", "scene_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr                     # no report of either sanitizer
    lines = r.stdout.split("\n")
    for case in CASES:                                  # every case ran and held
        assert "ok " + case in lines, r.stdout
    assert "scene: clean" in lines, r.stdout
