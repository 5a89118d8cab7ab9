"""Which form renders a scene (csrc/rt_choice.h Choice) on the host alone: tools/sanitize/choice_main.cpp -- a host that does what rt_launch.hip
launch() does with the record's answers, a launch a line in a log, the elapsed times handed in by the case -- built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a program of its own.  No device: the record holds no HIP.  The expectations are literals in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["whole_frames_small_scene_4",
         "whole_frames_small_scene_9",
         "whole_frames_small_scene_11",
         "a_pass_per_call_small_scene",
         "subset_launch_restarts_the_timed_step",
         "coop_dead_band",
         "coop_knob_opens_nothing",
         "blocking_call_splits_1_2_1_2",
         "one_step_per_non_blocking_launch",
         "walk_dead_band",
         "estimate_decides_outside_its_band",
         "nothing_asked_where_the_answer_is_known",
         "updates_keep_the_verdict_until_the_tree_moved",
         "new_scene_and_knobs_clear_the_verdicts_only",
         "a_follower_follows",
         "frame_ended_counts_launched_frames",
         "diagnostics_and_empty_calls_measure_nothing"]


def test_choice_record_under_sanitizers(tmp_path):
    exe = str(tmp_path / "choice_san")
    # (the sanitizers' runtimes linked INTO the program: it then starts whatever else its environment loads into a process ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sanitize", "choice_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr                     # no report of either sanitizer
    lines = r.stdout.split("\n")
    for case in CASES:                                  # every case ran and held
        assert "ok " + case in lines, r.stdout
    assert "choice: clean" in lines, r.stdout
