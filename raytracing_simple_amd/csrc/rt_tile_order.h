// rt_tile_order.h -- the heavy-first tile schedule of a context: what the per-tile costs on the device are worth, whether an order
// sorted from them exists, and what the next launch does about both.  Host bookkeeping only: rt_launch.hip launch_form() asks for a
// plan, carries it out (the sort kernel, the launch's order / cost pointers and its flag) and reports the launch; nothing else edits
// this record.  No HIP in here -- tests/test_tile_order_cpu.py drives it through its sequences with the host compiler alone.
//
// Heavy tiles first: launches leave per-tile costs, and a launch of the same scene, camera and tile shape walks the tiles in descending order of
// cost (sorted on the device, once per change of scene or camera).  A LONG launch (8 passes and more) replaces the costs with its own and sorts
// from the last long launch's.  SHORT launches -- the reference's own regime is a pass per call, the adapter's display loop about a millisecond's
// worth -- used to get nothing of this: no costs from fewer than 4 passes, no sort below 8.  Yet once the order exists it is worth as much to them
// (complex.scn 12 %, C3 8-13 %, 8192 spheres 12-22 % on launches of 1 / 2 / 4 passes: profiles/r06_order_short_launches.jsonl).  So while the order is
// missing or stale, short launches ADD their costs up in a window (launch flag bit 1: the kernel's epilogue adds instead of stores), and the short
// launch that finds 16 passes' worth there sorts from them; with a valid order short launches do not touch the costs at all.
#pragma once

#include <cstdint>

namespace rt {

struct TileOrder {
    static constexpr int kLongLaunch = 8, kShortWindow = 16;
    static constexpr uint32_t kMinPasses = 4;           // fewer than four passes' worth of costs orders nothing
    // A long launch that would walk its tiles in image order although their costs can be had -- the first frame of a scene --
    // renders 4 of its passes first, which prices the tiles, and the rest heavy first (rt_launch.hip launch_priced)
    static constexpr int kPricePasses = 4, kPriceFrom = 24;

    uint32_t *d_tile_cost = nullptr, *d_order = nullptr;    // device arrays (rt_trace.inc.h): per-tile cost of the last launch, and the order derived from it
    uint32_t n_tiles = 0;               // capacity of the two arrays (8x8 tiles)
    uint32_t cost_tiles = 0;            // tile count of the launch the costs come from
    bool cost_valid = false, order_valid = false;
    uint32_t cost_passes = 0;           // passes behind the costs now in d_tile_cost
    bool cost_window = false;           // ... which come from a window of SHORT launches (fewer than 8 passes each) adding up, not from one long launch
    bool order_stale = false;           // scene or camera have changed since the order was sorted: it stays in use until a long launch sorts it again
    int use_order = 1;                  // diagnostics knob (enable): 0 = tiles in their natural order, no costs kept

    // What one launch does about the schedule.  sort_now: sort d_order from d_tile_cost ahead of the launch; use_order: the launch walks d_order;
    // write_costs: it leaves its per-tile costs in d_tile_cost; accumulate: ... ADDING them to what is there (launch flag bit 1)
    struct Plan { bool sort_now = false, use_order = false, write_costs = false, accumulate = false; };

    // a new scene, or something else wrote over the costs: neither costs nor order say anything
    void forget() { cost_valid = order_valid = false; }

    // The last frame's costs still predict the next one (moving spheres, a moved camera): the order stays in use and the next long launch sorts it
    // again from them -- or the next window of short launches, which starts again
    void scene_or_camera_moved() { order_stale = true; if (cost_window) cost_passes = 0; }

    // The order a priced first frame walked came from four passes' worth of costs; the frame itself has now left the costs of all its passes,
    // a better prediction of the next frame: the next long launch sorts once more from those (C2 2.63 -> 2.58 ms per steady frame,
    // the same on passes not seen before; profiles/r05_resort_after_pricing_ab.jsonl)
    void sort_again_from_whole_frame() { if (order_valid) order_stale = true; }

    // diagnostics: heavy first on / off; either way the order in hand is dropped (the costs stay)
    void enable(bool on) { use_order = on ? 1 : 0; order_valid = false; }

    // The plan of a launch of `tiles` tiles and `n_samples` passes.  `natural_order`: this launch neither sorts nor walks the order (the hierarchy's
    // probe times both forms in image order); `instance_logs_cost`: its kernel keeps the schedule's arrays at all (rt_device.h kInstNoTileCost).
    // A planned sort counts as done: the caller runs it, or calls forget() if it cannot.
    Plan plan(uint32_t tiles, int n_samples, bool natural_order, bool instance_logs_cost) {
        Plan p;
        if (!use_order || !d_tile_cost || tiles > n_tiles || !instance_logs_cost) return p;
        if (cost_tiles != tiles) {                                  // another tile shape: start over
            cost_valid = order_valid = false;
            cost_passes = 0;
        }
        const bool short_launch = n_samples < kLongLaunch;
        const bool order_wanted = !order_valid || order_stale;
        // (a short launch sorts from a long launch's costs whenever the order is stale -- they still predict the next frame -- and from a window's once it is full)
        const bool costs_ripe = !short_launch || !cost_window || cost_passes >= (uint32_t)kShortWindow;
        if (cost_valid && order_wanted && !natural_order && costs_ripe) {
            p.sort_now = true;
            order_valid = true;
            order_stale = false;
            if (short_launch && cost_window) cost_passes = 0;       // (the window's costs are spent)
        }
        p.use_order = order_valid && !natural_order;
        if (!short_launch || !order_valid || order_stale) {         // (a short launch under a valid order leaves the costs alone)
            p.write_costs = true;
            p.accumulate = short_launch && cost_window && cost_passes > 0;
        }
        return p;
    }

    // the launch planned so has been queued
    void launched(const Plan &p, int n_samples, uint32_t tiles) {
        if (!p.write_costs) return;
        if (n_samples >= kLongLaunch) {
            cost_window = false;
            cost_passes = (uint32_t)n_samples;
        } else if (p.accumulate) {
            cost_passes += (uint32_t)n_samples;
        } else {                                        // a short launch has replaced the costs with its own: a new window
            cost_window = true;
            cost_passes = (uint32_t)n_samples;
        }
        cost_valid = cost_passes >= kMinPasses;
        cost_tiles = tiles;
    }

    // a launch this long has nothing to walk its tiles by and could price them first (kPricePasses of its own passes)
    bool wants_pricing(int n_samples) const { return use_order && d_tile_cost && n_samples >= kPriceFrom && !order_valid && !cost_valid; }
    // an order sorted from costs is in hand (fresh or stale)
    bool has_order() const { return order_valid; }
    // the tiles of the last launch's workgroup shape: how much of the two arrays means something
    uint32_t tiles_in_use() const { return cost_valid && cost_tiles ? cost_tiles : n_tiles; }
};

}  // namespace rt
