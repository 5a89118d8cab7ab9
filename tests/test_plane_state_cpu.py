"""The frame record's row for the moments plane (csrc/rt_frame_state.h: `moments_formed`), with the host compiler alone:
reprojected(true) sets it beside temporal_current, reprojected(false) and reprojected() leave the temporal plane current and the moments plane not
formed, every event that ends the temporal plane clears it, and nothing else touches it.  Literal values throughout; tests/test_gpu_moments.py walks
the same enders and keepers on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "rt_frame_state.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static rt::FrameState with_moments() {
    rt::FrameState f;
    f.launched(2, true);
    f.reprojected(true);
    EXPECT(f.temporal_current == true && f.moments_formed == true);
    return f;
}

// the event ends the temporal plane, and the flag goes with it
template <class Event> static void ends(const char *what, Event event) {
    rt::FrameState f = with_moments();
    event(f);
    if (f.temporal_current != false || f.moments_formed != false) {
        std::printf("%s: temporal_current %d, moments_formed %d, want 0, 0\n", what, (int)f.temporal_current, (int)f.moments_formed);
        ++failures;
    }
}

// the event leaves both planes as they are
template <class Event> static void keeps(const char *what, Event event) {
    rt::FrameState f = with_moments();
    event(f);
    if (f.temporal_current != true || f.moments_formed != true) {
        std::printf("%s: temporal_current %d, moments_formed %d, want 1, 1\n", what, (int)f.temporal_current, (int)f.moments_formed);
        ++failures;
    }
}

int main() {
    rt::FrameState f;
    EXPECT(f.temporal_current == false && f.moments_formed == false);
    f.reprojected(true);
    EXPECT(f.temporal_current == true && f.moments_formed == true && f.atrous_current == false);
    f.reprojected(false);                                   // the setting off: T is formed again, M is not
    EXPECT(f.temporal_current == true && f.moments_formed == false);
    f.reprojected(true);
    f.reprojected();                                        // (the default says the same)
    EXPECT(f.temporal_current == true && f.moments_formed == false);
    // nothing else of the frame changes, whichever way
    rt::FrameState g;
    g.launched(3, false);
    g.pair_filtered(7);
    g.reprojected(true);
    EXPECT(g.current_sample == 3 && g.launches == 1 && g.pixels_current == false && g.filtered_pair == 7 && g.filtered_behind == 0 && g.ragged == false);

    // the ten events that end T
    ends("a reset", [](rt::FrameState &s) { s.reset_blocking(); });
    ends("an in-place reset", [](rt::FrameState &s) { s.reset_in_place(); });
    ends("a written state", [](rt::FrameState &s) { s.state_written(5, true); });
    ends("a launch", [](rt::FrameState &s) { s.launched(1, true); });
    ends("a subset launch", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(2, 6); s.launched_subset(1, true, false); });
    ends("a merge", [](rt::FrameState &s) { s.merged(9); });
    ends("a merge by tile", [](rt::FrameState &s) { s.merged_by_tile(9); });
    ends("a filter into the context", [](rt::FrameState &s) { s.colours_replaced(); });
    ends("a feature plane formed again", [](rt::FrameState &s) { s.features_reformed(); });
    {                                                       // a second reprojection with the setting off ends M and forms T again
        rt::FrameState s = with_moments();
        s.reprojected(false);
        EXPECT(s.temporal_current == true && s.moments_formed == false);
    }
    // ... and their kin
    ends("a subset launch of every group", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(6, 18); s.launched_subset(1, true, true); });
    ends("a written state without seeds", [](rt::FrameState &s) { s.state_written(5, false); });
    ends("a seed stream", [](rt::FrameState &s) { s.reset_in_place(); s.custom_seeds_written(); });

    keeps("the wavelet filter", [](rt::FrameState &s) { s.atrous_filtered(); });
    keeps("cross-filtering the halves", [](rt::FrameState &s) { s.pair_filtered(3); });
    keeps("a selection started", [](rt::FrameState &s) { s.selection_started(); });
    keeps("a selection", [](rt::FrameState &s) { s.selection_started(); s.selection_landed(2, 6); });
    keeps("packing the frame", [](rt::FrameState &s) { s.pixels_packed(); });
    keeps("a timed launch's figure", [](rt::FrameState &s) { s.timed(1.0); });
    keeps("reprojecting again with the setting on", [](rt::FrameState &s) { s.reprojected(true); });

    // a flag that went with T does not come back with the next T
    rt::FrameState h = with_moments();
    h.launched(1, true);
    h.reprojected();
    EXPECT(h.temporal_current == true && h.moments_formed == false);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
'''


def test_the_frame_record_knows_whether_the_moments_plane_was_formed(tmp_path):
    src = tmp_path / "plane_state.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "plane_state"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
