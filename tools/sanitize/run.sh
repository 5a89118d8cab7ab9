#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the CPU-side code (GPU sanitizers are not
# available on this pool): the oracle's renderer, the product's host helpers (scene reader with
# good, truncated and missing files, seed stream, camera basis), the hierarchy's host builders,
# the record of a context's resources (rt_owned.h, with a recorder in owned_free's place), the
# record of which form renders a scene (rt_choice.h, with a log in the launches' place), the
# rule that says which kernel instance a launch gets and which kernel forms the feature plane
# (rt_instance.h) and the record of what a context holds of its scene (rt_scene_state.h).
# Run from the repository root.
set -eu
R=$(cd "$(dirname "$0")/../.." && pwd)
T=/tmp/rt_san; mkdir -p $T
python3 - <<PY
import sys; sys.path.insert(0, "$R")
from raytracing_simple_amd import host, scenes
sph, o, t = scenes.demo_plus(16)
host.write_scene("$T/a.scn", sph, o, t)
open("$T/bad1.scn", "w").write("camera 1 2 3\n")
open("$T/bad2.scn", "w").write(open("$T/a.scn").read()[:200])
PY
gcc -std=c11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -mfma -ffp-contract=off -I$R/oracle \
    $R/tools/sanitize/oracle_main.c $R/oracle/rt_oracle.c -o $T/oracle_san -lm -lpthread
$T/oracle_san
# (rt_host.cpp finds csrc/rt_rules.h beside itself: the host statements of the filters, and through them every rule, run in host_san)
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I$R/include \
    $R/tools/sanitize/host_main.cpp $R/raytracing_simple_amd/csrc/rt_host.cpp -o $T/host_san
# the hierarchy's host builders (rt_bvh_host.cpp alone: plain C++), both shapes, on generated record sets
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -I$R/include \
    $R/tools/sanitize/bvh_main.cpp $R/raytracing_simple_amd/csrc/rt_bvh_host.cpp -o $T/bvh_san
$T/bvh_san
$T/host_san
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I$R/raytracing_simple_amd/csrc $R/tools/sanitize/owned_main.cpp -o $T/owned_san
$T/owned_san
# which form renders a scene (rt_choice.h alone), driven as rt_launch.hip drives it
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I$R/raytracing_simple_amd/csrc $R/tools/sanitize/choice_main.cpp -o $T/choice_san
$T/choice_san
# which kernel instance a launch gets (rt_instance.h alone): the thresholds from either side, the LDS of every table kind, recorded real scenes
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I$R/raytracing_simple_amd/csrc $R/tools/sanitize/instance_main.cpp -o $T/instance_san
$T/instance_san
# which kernel forms the feature plane (rt_instance.h features_form, features_lds): no hierarchy, the count and the LDS limits from either side
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I$R/raytracing_simple_amd/csrc $R/tools/sanitize/features_main.cpp \
    $R/raytracing_simple_amd/csrc/rt_bvh_host.cpp -o $T/features_san
$T/features_san
# what a context holds of its scene (rt_scene_state.h alone), driven in the order the API's calls report to it
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I$R/raytracing_simple_amd/csrc $R/tools/sanitize/scene_main.cpp -o $T/scene_san
$T/scene_san
# the .scn reader on 1000 mutated files (deletions, junk tokens, non-finite numbers, truncation)
mkdir -p $T/fz
python3 - <<PY
import random
base = open("$T/a.scn", "rb").read()
random.seed(1)
toks = [b"nan", b"inf", b"-inf", b"1e999", b"-1e999", b"0x10", b"", b" ", b"\n", b"\x00", b"size", b"sphere", b"camera",
        b"99999999999999999999", b"-1", b"1.5e-45", b"\t\t", b"9" * 400]
for i in range(1000):
    b = bytearray(base)
    for _ in range(random.randint(1, 6)):
        k, pos = random.random(), random.randrange(len(b) + 1)
        if k < 0.3 and b: del b[pos:pos + random.randint(1, 40)]
        elif k < 0.6: b[pos:pos] = random.choice(toks)
        elif k < 0.8 and b: b[min(pos, len(b) - 1)] = random.randrange(256)
        else: b = b[:pos]
    open("$T/fz/f%d.scn" % i, "wb").write(bytes(b))
PY
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I$R/include \
    $R/tools/sanitize/reader_fuzz.cpp $R/raytracing_simple_amd/csrc/rt_host.cpp -o $T/reader_fuzz
$T/reader_fuzz
echo "sanitizers: clean"
