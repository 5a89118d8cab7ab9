"""The heavy-first tile schedule (csrc/rt_tile_order.h TileOrder) on the host alone: a small C++ program drives the record through the
sequences the GPU tests of tests/test_gpu_features.py describe (a priced first frame, long frames, windows of short launches, a moved
camera) and checks the plan of every launch.  No device: the record holds no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "rt_tile_order.h"

using rt::TileOrder;
static int bad = 0;
static uint32_t cells[2];

// a plan as four letters: S = sort now, O = walk the order, C = write costs, A = add them to what is there
static void expect(const char *what, const TileOrder::Plan &p, const char *want) {
    char got[5] = { p.sort_now ? 'S' : '-', p.use_order ? 'O' : '-', p.write_costs ? 'C' : '-', p.accumulate ? 'A' : '-', 0 };
    if (std::string_view(got) != want) { printf("%s: plan %s, expected %s\n", what, got, want); bad = 1; }
}
static void check(const char *what, bool ok) { if (!ok) { printf("%s\n", what); bad = 1; } }

static TileOrder fresh(uint32_t cap = 100) {
    TileOrder t;
    t.d_tile_cost = &cells[0]; t.d_order = &cells[1]; t.n_tiles = cap;          // (never dereferenced here)
    return t;
}
// one launch: plan, check, report
static void go(TileOrder &t, const char *what, uint32_t tiles, int passes, const char *want, bool natural = false, bool logs = true) {
    const TileOrder::Plan p = t.plan(tiles, passes, natural, logs);
    expect(what, p, want);
    t.launched(p, passes, tiles);
}

int main() {
    {   // long launches of one scene: the first leaves costs, the second sorts from them, the third walks that order
        TileOrder t = fresh();
        check("a fresh record has no order and 100 tiles", !t.has_order() && t.tiles_in_use() == 100);
        go(t, "first long launch", 100, 8, "--C-");
        go(t, "second long launch", 100, 8, "SOC-");
        go(t, "third long launch", 100, 64, "-OC-");
        check("order in hand after long launches", t.has_order());
        // scene or camera moved: the order stays in use and the next long launch sorts again
        t.scene_or_camera_moved();
        check("a stale order is still an order", t.has_order());
        go(t, "long launch after a move", 100, 8, "SOC-");
        go(t, "long launch after that", 100, 8, "-OC-");
        // ... as does a short launch, at once, from the long launch's costs; it leaves them alone
        t.scene_or_camera_moved();
        go(t, "short launch after a move, long costs", 100, 1, "SO--");
        go(t, "short launch under a fresh order", 100, 4, "-O--");
        // natural order (the hierarchy's probe): never sorts, never hands the order out; a long launch still leaves its costs
        t.scene_or_camera_moved();
        go(t, "natural order, stale order", 100, 8, "--C-", true);
        go(t, "natural order, short", 100, 2, "--C-", true);                     // (a stale order: the short launch starts a window)
        go(t, "heavy first again", 100, 8, "-OC-");                              // (two passes' worth of costs sorts nothing; the stale order is walked)
        go(t, "and sorted from that launch", 100, 8, "SOC-");
        // another tile count: everything starts over
        go(t, "another tile shape", 25, 8, "--C-");
        check("tiles in use follow the launch", t.tiles_in_use() == 25 && !t.has_order());
        go(t, "second launch of that shape", 25, 8, "SOC-");
        // more tiles than the arrays hold: nothing planned, nothing changed
        go(t, "more tiles than the arrays hold", 101, 8, "----");
        check("... and nothing changed", t.tiles_in_use() == 25 && t.has_order());
        // an instance that keeps no costs
        go(t, "instance without tile costs", 25, 8, "----", false, false);
        check("... changed nothing either", t.tiles_in_use() == 25 && t.has_order());
        // a new scene
        t.forget();
        check("forgotten", !t.has_order() && t.tiles_in_use() == 100);
        go(t, "first long launch of the new scene", 25, 8, "--C-");
        go(t, "second", 25, 8, "SOC-");
    }
    {   // short launches without an order: the first replaces the costs, later ones add up, the one that finds 16 passes' worth sorts
        TileOrder t = fresh();
        go(t, "short 1", 100, 1, "--C-");
        go(t, "short 2", 100, 2, "--CA");
        go(t, "short 4", 100, 4, "--CA");                                        // 7 passes
        go(t, "short 4 again", 100, 4, "--CA");                                  // 11
        go(t, "short 4 once more", 100, 4, "--CA");                              // 15
        go(t, "short 1, 15 in the window", 100, 1, "--CA");                      // 16
        check("no order before the window is full", !t.has_order());
        go(t, "the launch that finds 16 passes", 100, 1, "SO--");                // sorts; the window is spent, the costs are left alone
        for (int k = 0; k < 7; ++k) go(t, "short launch under a fresh order", 100, k % 2 ? 2 : 1, "-O--");
        // a moved camera: the order stays in use, the window starts again
        t.scene_or_camera_moved();
        go(t, "first short launch after the move", 100, 1, "-OC-");              // replaces
        for (int k = 0; k < 15; ++k) go(t, "window after the move", 100, 1, "-OCA");
        go(t, "the 17th sorts again", 100, 1, "SO--");
        go(t, "and the 18th walks it", 100, 1, "-O--");
        // a move in the middle of a window empties it
        t.scene_or_camera_moved();
        for (int k = 0; k < 8; ++k) go(t, "half a window", 100, 2, k ? "-OCA" : "-OC-");
        t.scene_or_camera_moved();
        go(t, "window restarted", 100, 2, "-OC-");
        for (int k = 0; k < 7; ++k) go(t, "window refilled", 100, 2, "-OCA");
        go(t, "full: sorts", 100, 2, "SO--");
        // a long launch ends the window regime: it replaces the costs, and a stale order is then sorted by the next launch of any length
        go(t, "long launch under a fresh order", 100, 8, "-OC-");
        t.scene_or_camera_moved();
        go(t, "short launch, long costs", 100, 1, "SO--");
    }
    {   // fewer than four passes' worth of costs orders nothing
        TileOrder t = fresh();
        go(t, "3 passes", 100, 3, "--C-");
        go(t, "long launch after 3 passes", 100, 8, "--C-");
        go(t, "long launch after 8", 100, 8, "SOC-");
        TileOrder u = fresh();
        go(u, "2 passes", 100, 2, "--C-");
        go(u, "+ 2 passes", 100, 2, "--CA");                                     // four: valid, but a window sorts only once it holds 16
        go(u, "long launch after a window of 4", 100, 8, "SOC-");                // (a long launch sorts from whatever valid costs there are)
    }
    {   // a first frame prices its tiles with four of its own passes, and its order is sorted once more from the whole frame
        TileOrder t = fresh();
        check("a first frame of 24 passes is priced", t.wants_pricing(24) && t.wants_pricing(4096));
        check("one of 23 is not", !t.wants_pricing(23));
        go(t, "pricing launch", 100, TileOrder::kPricePasses, "--C-");
        check("priced: not again", !t.wants_pricing(28));
        go(t, "rest of the first frame", 100, 28, "SOC-");
        t.sort_again_from_whole_frame();
        check("no pricing with an order", !t.wants_pricing(32));
        go(t, "second frame", 100, 32, "SOC-");
        go(t, "third frame", 100, 32, "-OC-");
        t.forget();
        check("a new scene is priced again", t.wants_pricing(30));
        t.sort_again_from_whole_frame();                                         // (without an order there is nothing to sort again)
        go(t, "no order: no sort", 100, 8, "--C-");
    }
    {   // heavy first switched off: an empty plan, no pricing; switching drops the order and keeps the costs
        TileOrder t = fresh();
        go(t, "long", 100, 8, "--C-");
        go(t, "long", 100, 8, "SOC-");
        t.enable(false);
        check("off: no order, no pricing", !t.has_order() && !t.wants_pricing(64));
        go(t, "off", 100, 8, "----");
        go(t, "off, short", 100, 1, "----");
        t.enable(true);
        go(t, "on again: sorted from the costs kept", 100, 8, "SOC-");
        TileOrder none;                                                          // a context without rows: no arrays
        go(none, "no arrays", 0, 8, "----");
        check("no arrays: no pricing", !none.wants_pricing(64));
    }
    return bad;
}
'''


def test_tile_order_plans_every_launch_of_the_sequences_the_gpu_tests_describe(tmp_path):
    """csrc/rt_tile_order.h: long launches (costs, then sort, then walk), windows of short launches (replace, add up, sort at 16 passes,
    then hands off the costs), a moved scene or camera (stale order in use, window restarted, next long launch sorts), another tile
    count (start over), natural order (never sorts, never hands out the order), fewer than four passes (order nothing), the priced first
    frame and its second sort, and the switch -- the plan of each launch as the launch path carries it out."""
    src = tmp_path / "tile_order.cpp"
    src.write_text("#include <string_view>\n" + PROGRAM)
    exe = tmp_path / "tile_order"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
