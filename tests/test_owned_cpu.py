"""The record of what a context owns (csrc/rt_owned.h Owned) on the host alone: tools/sanitize/owned_main.cpp -- which defines owned_free as a
recorder over made-up handles -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own.  No device: the
record holds no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["recorder_reports_a_double_free",
         "release_frees_each_once_in_reverse_with_its_kind",
         "drop_frees_now_and_release_not_again",
         "forget_frees_nothing_nor_the_destructor",
         "destructor_releases",
         "exchanged_handles_are_each_freed_once"]


def test_owned_record_under_sanitizers(tmp_path):
    exe = str(tmp_path / "owned_san")
    # (the sanitizers' runtimes linked INTO the program: it then starts whatever else its environment loads into a process ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sanitize", "owned_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr                     # no report of either sanitizer
    lines = r.stdout.split("\n")
    for case in CASES:                                  # every case ran and held, the recorder's own check among them
        assert "ok " + case in lines, r.stdout
    assert "owned: clean" in lines, r.stdout
