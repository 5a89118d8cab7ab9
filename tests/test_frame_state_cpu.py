"""The host record of a progressive frame (csrc/rt_frame_state.h FrameState) on the host alone: a small C++ program reports the things that
happen to a frame -- launches, resets, seed streams, selections, merges, written states -- and checks EVERY field after every step against
literal values.  The literals are DESIGN.md section 5.10's table, read off the call sites as they stood before the record existed.  No
device: the record holds no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include "rt_frame_state.h"

using rt::FrameState;
static int bad = 0;

// every field as one line: pass | seeds_default seeds_custom | pixels_current | launches last_ms | ragged have_selection | counts serial |
// list_valid list_by_order list_serial list_tiles list_slots
static void expect(const char *what, const FrameState &f, const char *want) {
    char got[160];
    snprintf(got, sizeof got, "p%d sd%d sc%d px%d L%llu ms%g rg%d sel%d c%u,%u s%llu lv%d lo%d ls%llu lt%u ln%u", f.current_sample, (int)f.seeds_default,
             (int)f.seeds_custom, (int)f.pixels_current, (unsigned long long)f.launches, f.last_ms, (int)f.ragged, (int)f.have_selection, f.counts[0],
             f.counts[1], (unsigned long long)f.selection_serial, (int)f.list_valid, (int)f.list_by_order, (unsigned long long)f.list_serial, f.list_tiles,
             f.list_slots);
    if (strcmp(got, want) != 0) { printf("%s:\n  got      %s\n  expected %s\n", what, got, want); bad = 1; }
}
static void check(const char *what, bool ok) { if (!ok) { printf("%s\n", what); bad = 1; } }

int main() {
    {   // A: render, pack, reset, seed
        FrameState f;
        expect("fresh", f, "p0 sd0 sc0 px1 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        check("a fresh record is on the default stream", f.on_default_stream());
        f.launched(4, true);
        expect("4 passes, store on", f, "p4 sd0 sc0 px1 L1 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.launched(2, false);
        expect("2 passes, store off", f, "p6 sd0 sc0 px0 L2 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.timed(1.5);
        expect("a blocking launch's time", f, "p6 sd0 sc0 px0 L2 ms1.5 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.pixels_packed();
        expect("packed", f, "p6 sd0 sc0 px1 L2 ms1.5 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.launched(1, false);
        f.reset_in_place();
        expect("in-place reset: seeds_custom and pixels_current stay", f, "p0 sd1 sc0 px0 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.custom_seeds_written();
        expect("custom stream", f, "p0 sd0 sc1 px0 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        check("a custom stream is not the default stream", !f.on_default_stream());
        f.reset_in_place();
        expect("in-place reset again: seeds_custom still set", f, "p0 sd1 sc1 px0 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        check("... and the default stream is read all the same", f.on_default_stream());
        f.launched(3, true);
        f.reset_blocking();
        expect("blocking reset", f, "p0 sd0 sc0 px1 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
    }
    {   // B: subset launches
        FrameState f;
        f.reset_in_place();
        f.selection_started();
        expect("selection started", f, "p0 sd1 sc0 px1 L0 ms0 rg0 sel0 c0,0 s0 lv0 lo0 ls0 lt0 ln0");
        f.selection_landed(3, 10);
        expect("selection landed", f, "p0 sd1 sc0 px1 L0 ms0 rg0 sel1 c3,10 s1 lv0 lo0 ls0 lt0 ln0");
        check("no list yet", f.list_is_stale(true, 40));
        f.list_built(true, 40, 16);
        expect("list built", f, "p0 sd1 sc0 px1 L0 ms0 rg0 sel1 c3,10 s1 lv1 lo1 ls1 lt40 ln16");
        check("the list serves this launch", !f.list_is_stale(true, 40));
        check("another tile shape wants another list", f.list_is_stale(true, 160));
        check("image order wants another list", f.list_is_stale(false, 40));
        f.default_seeds_copied();
        expect("default stream copied for the tiles left out", f, "p0 sd0 sc0 px1 L0 ms0 rg0 sel1 c3,10 s1 lv1 lo1 ls1 lt40 ln16");
        f.launched_subset(3, true, false);
        expect("subset launch, pixels current before", f, "p3 sd0 sc0 px1 L1 ms0 rg1 sel1 c3,10 s1 lv1 lo1 ls1 lt40 ln16");
        f.colours_replaced();
        f.launched_subset(3, true, false);
        expect("subset launch, pixels stale before: they stay stale", f, "p6 sd0 sc0 px0 L2 ms0 rg1 sel1 c3,10 s1 lv1 lo1 ls1 lt40 ln16");
        f.launched_subset(1, false, true);
        expect("subset launch, store off", f, "p7 sd0 sc0 px0 L3 ms0 rg0 sel1 c3,10 s1 lv1 lo1 ls1 lt40 ln16");
        f.selection_started();
        f.selection_landed(5, 20);
        expect("second selection", f, "p7 sd0 sc0 px0 L3 ms0 rg0 sel1 c5,20 s2 lv0 lo1 ls1 lt40 ln16");
        f.list_built(true, 40, 24);
        f.selection_landed(5, 20);
        check("a newer selection makes the list stale by its serial alone", f.list_valid && f.list_is_stale(true, 40));
        f.list_built(false, 40, 24);
        check("rebuilt", !f.list_is_stale(false, 40));
        f.order_resorted();
        expect("order re-sorted", f, "p7 sd0 sc0 px0 L3 ms0 rg0 sel1 c5,20 s3 lv0 lo0 ls3 lt40 ln24");
        check("a re-sort makes the list stale", f.list_is_stale(false, 40));
        f.launched_subset(2, true, false);
        check("ragged after a launch that left groups out", f.ragged);
        f.launched_subset(2, true, true);
        expect("every group selected: whole again, pixels current again", f, "p11 sd0 sc0 px1 L5 ms0 rg0 sel1 c5,20 s3 lv0 lo0 ls3 lt40 ln24");
    }
    {   // C: merges and written state
        FrameState f;
        f.launched(4, true);
        f.selection_started();
        f.selection_landed(2, 8);
        f.list_built(false, 12, 12);
        f.merged(12);
        expect("whole-frame merge: list_valid stays", f, "p12 sd0 sc0 px0 L1 ms0 rg0 sel0 c2,8 s1 lv1 lo0 ls1 lt12 ln12");
        f.pixels_packed();
        f.selection_landed(2, 8);
        f.merged_by_tile(20);
        expect("per-tile merge", f, "p20 sd0 sc0 px0 L1 ms0 rg1 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
        f.timed(2.0);
        f.state_written(5, true);
        expect("state written at pass 5 with seeds", f, "p5 sd0 sc1 px0 L0 ms0 rg0 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
        f.state_written(0, false);
        expect("state written at pass 0 without seeds", f, "p0 sd1 sc0 px0 L0 ms0 rg0 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
        f.launched(2, true);
        expect("a launch after it", f, "p2 sd0 sc0 px1 L1 ms0 rg0 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
        f.colours_replaced();
        expect("colour plane replaced: pixels_current alone", f, "p2 sd0 sc0 px0 L1 ms0 rg0 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
        f.front_follows(9);
        expect("a multi-device front follows its shards: the pass alone", f, "p9 sd0 sc0 px0 L1 ms0 rg0 sel0 c2,8 s2 lv0 lo0 ls1 lt12 ln12");
    }
    {   // D: the diagnostics reset by copy touches pass and seed flags, nothing else
        FrameState f;
        f.reset_in_place();
        f.custom_seeds_written();
        f.reset_in_place();
        f.selection_landed(1, 4);
        f.list_built(true, 8, 8);
        f.launched_subset(3, false, false);
        f.timed(0.25);
        expect("before", f, "p3 sd0 sc1 px0 L1 ms0.25 rg1 sel1 c1,4 s1 lv1 lo1 ls1 lt8 ln8");
        f.debug_reset_by_copy();
        expect("reset by copy", f, "p0 sd0 sc0 px0 L1 ms0.25 rg1 sel1 c1,4 s1 lv1 lo1 ls1 lt8 ln8");
        f.reset_in_place();
        f.debug_reset_by_copy();
        expect("reset by copy after an in-place reset", f, "p0 sd0 sc0 px0 L0 ms0 rg0 sel0 c1,4 s1 lv0 lo1 ls1 lt8 ln8");
    }
    return bad;
}
'''


def test_frame_state_holds_the_table_of_transitions_field_by_field(tmp_path):
    """csrc/rt_frame_state.h: sequence A (launches with the pixel store on and off, the pack, the in-place reset that keeps seeds_custom and
    pixels_current, a custom seed stream, the blocking reset), B (selection, list, subset launches that keep stale pixels stale, a list made
    stale by a newer selection, by another shape and by a re-sorted order, the launch of every group that makes the frame whole), C (the
    whole-frame merge that keeps list_valid, the per-tile merge, written states with and without seeds, a replaced colour plane, a
    multi-device front) and D (the diagnostics reset by copy: pass and seed flags, nothing else) -- every field after every step."""
    src = tmp_path / "frame_state.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "frame_state"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
