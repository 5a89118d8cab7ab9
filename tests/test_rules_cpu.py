"""The rules' arithmetic (csrc/rt_rules.h) is plain C++: a translation unit that includes nothing else compiles under g++ -std=c++17 -Wall with no HIP
header on the include path and no warning -- so the host statements (rt_host.cpp), the sanitizer programs and the kernels can all call the one copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_header_is_plain_cxx(tmp_path):
    unit = tmp_path / "rules_alone.cpp"
    unit.write_text('#include "rt_rules.h"\nint main() { return rt::falloff(0.0f) == 1.0f ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr                     # no warning either
