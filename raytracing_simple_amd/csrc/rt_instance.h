// rt_instance.h -- which kernel instance a launch gets: the context's thresholds and diagnostics knobs (Knobs), what the rule reads of a scene
// (SceneFacts), and the rule itself -- pick_shape() says role, workgroup shape and what rides along in LDS, instance_lds() sizes the dynamic LDS of
// the instance that was found, tile_width() says how wide its tile is.  rt_launch.hip looks the row up and carries the launch out; rt_debug.hip
// writes the knobs and asks the same rule for its staging probe; nothing else decides any of this.  No HIP in here --
// tests/test_instance_cpu.py drives the rule with the host compiler alone (tools/sanitize/instance_main.cpp).
// DESIGN.md section 5.14 lists who writes and who reads the record, and the thresholds with the measurement behind each.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_api.h"      // RT_MODE_PARITY, RT_MODE_FAST
#include "rt_choice.h"                  // Form, Choice::Facts

namespace rt {

constexpr int kMaxK2Table = 1024;   // running-average reciprocals kept in LDS up to this many passes per launch
constexpr uint32_t kBvhTopPairs = 255;      // eight full levels: 16 KiB of LDS beside the stacks, five workgroups per CU still fit
constexpr size_t kLdsMax = 152 * 1024;              // what the kernels' dynamic-LDS attribute allows

// LDS of the instance that walks the pairs: hdr | pairs | slots | per-lane stacks (u16) for `threads` lanes
inline size_t lds_bytes_pairs(uint32_t n_spheres, uint32_t n_lights, bool mat_in_lds, int n_samples, uint32_t n_leaves,
                              uint32_t n_slots, uint32_t stack_depth, int threads) {
    size_t b = (2 + 4 * (size_t)(n_leaves ? n_leaves - 1 : 0) + n_slots) * 16 + (size_t)n_lights * 32;
    b += (((size_t)stack_depth * threads * 2) + 15) & ~(size_t)15;
    if (mat_in_lds) b += (size_t)n_spheres * 32;
    if (n_samples <= kMaxK2Table) b += (size_t)(n_samples > 0 ? n_samples : 0) * 4;
    return (b + 15) & ~(size_t)15;
}

// LDS bytes the kernels need for a scene
inline size_t lds_bytes(uint32_t n_spheres, uint32_t n_lights, bool mat_in_lds, int n_samples = 0) {
    size_t b = (size_t)n_spheres * 16 + (size_t)n_lights * 32;
    if (mat_in_lds) b += (size_t)n_spheres * 32;
    if (n_samples <= kMaxK2Table) b += (size_t)(n_samples > 0 ? n_samples : 0) * 4;
    return (b + 15) & ~(size_t)15;
}

// ---- the kernel instances ------------------------------------------------------------------------------
// One row per instance (rt_device.h Instance), written next to the instantiations in rt_kernel_parity.hip / rt_kernel_fast.hip: what the
// instance is and what it needs.  rt_launch.hip picks an instance by ROLE, sizes its LDS from `tables` and refuses a
// launch whose instance needs a table the context does not have -- nothing in the host code depends on the order of
// the rows.  The product library holds the shipped rows only; the diagnostics build (librt_hip_diag.so) adds the
// A/B and verification instances (rt_set_mode 100 + row / 200 + row, or by name: rt_debug_instance).
enum InstanceTables : uint8_t {
    kTabSweepLds = 0,       // geometry + light tables staged in LDS (lds_bytes)
    kTabSweepGlobal = 1,    // ... read where they lie in HBM / L2
    kTabPairsLds = 2,       // the hierarchy (pairs, slots, stacks) staged in LDS (lds_bytes_pairs); needs BvhTables
    kTabPairsGlobal = 3,    // ... pairs and slots read where they lie; staged: header and stacks; needs BvhTables
    kTabPairsLdsSlotsGlobal = 4,   // ... the pairs staged, the slots read where they lie (the pairs fit the LDS budget, the whole tables do not)
    kTabPairsTopLds = 5,    // ... pairs and slots read where they lie but for the promoted top of the tree (BvhTables::n_top pairs), which is staged
    kTabPairsPacked = 6,    // ... the PACKED pair table (BvhTables::packed_at) and the slots read where they lie; staged: header, frame and stacks
};
// the instance walks a hierarchy: it needs the scene's BvhTables
inline bool walks_hierarchy(uint8_t tables) {
    return tables == kTabPairsLds || tables == kTabPairsGlobal || tables == kTabPairsLdsSlotsGlobal || tables == kTabPairsTopLds || tables == kTabPairsPacked;
}
enum InstanceRole : uint8_t {
    kRoleNone = 0,          // diagnostics: reachable by row / name only
    kRolePlain,             // small scenes
    kRoleCoop,              // 12 spheres and more: cooperative any-hit
    kRolePairs,             // large scenes through the hierarchy
    kRolePairsGlobal,       // ... tables beyond the LDS budget
    kRolePairsMixed,        // ... whose pairs still fit it (rt_trace_*_pairs_m)
    kRoleSweepGlobal,       // no hierarchy (or it lost the measurement) and a table beyond the sweep's LDS budget (Knobs::sweep_lds_limit)
    kRolePersist,           // diagnostics: persistent wavefronts (rt_debug_set_persist)
    kRolePersistCoop,
    kRoleTimelog,           // diagnostics: the shipped shape + device wall-clock logging
};
enum InstanceFlags : uint8_t {
    kInstPersistent = 1,    // the grid only fills the machine; tiles come from the queue at counters[30]
    kInstNoTileCost = 2,    // neither reads the heavy-first order nor leaves per-tile costs
    kInstStaticCoop = 4,    // carries the cooperative any-hit mailbox (1.5 KiB of static LDS per wavefront)
    kInstTwoRays = 8,       // diagnostics: two pixels per lane -- a wavefront's tile is 16 x 8, and every lane has two stacks
};
// pixels across the tile of a workgroup of `waves` wavefronts: one 8x8 sub-tile per wavefront, 16x8 with two pixels per lane
inline int tile_width(int waves, uint8_t flags) { return 8 * waves * ((flags & kInstTwoRays) ? 2 : 1); }

// What a launch is made of besides the scene: arithmetic mode, thresholds, diagnostics knobs.  Written by rt_create (n_cus), rt_set_mode (mode) and
// the rt_debug_set_* calls (rt_debug.hip: everything else); read by pick_shape() below, rt_launch.hip, the hierarchy's builders (rt_bvh.hip) and
// whoever packs a frame or sizes a grid by the machine
struct Knobs {
    // ---- which instance ----
    int wg_waves = 0;                   // diagnostics knob: 0 = automatic, 1 / 4 = force the workgroup shape
    int mode = RT_MODE_PARITY;
    int regen_gate = 0;                 // 0 = choose from the scene size
    int mat_lds_limit = 24 * 1024;
    int sweep_lds_limit = 40 * 1024;    // the plain / cooperative sweep stages its tables while four workgroups of that size fit a CU; beyond, the table is read through the
                                        // scalar cache at six wavefronts per SIMD whatever its size (rt_trace_*_g).  Measured at 1080p on scenes without a hierarchy
                                        // (profiles/r06_g_threshold.jsonl): at 48 KB (3 per CU) rt_trace_*_g takes 0.62 / 0.92 x the staged sweep's time (NaN records / a closed
                                        // box of mirrors), at 64 KB (2) 0.41 / 0.63, at 96 KB and more (1) 0.19; at 32 KB (4) 0.80 / 1.12, below that 0.9 ... 1.3
    int coop_kmax = 0;                  // cooperative any-hit only while no more than this many shadow rays are pending in the wavefront (0 = no limit)
    int direct_max = 3;                 // RT_OPT_DIRECT_CAMERA: candidate spheres per tile up to which camera rays are resolved lane by lane (-1 = never; rt_debug_set_direct_camera)
    int coop_min = 12;                  // scenes with at least this many spheres use the cooperative any-hit instance (0 = never)
    int persist = 0;                    // diagnostics: persistent-wavefront instances
    int n_cus = 256;
    // ---- the hierarchy's build ----
    int bvh_sah = 1;                    // the hierarchy's shape is chosen by surface area (rt_bvh.hip): 1 = uploads below kAlwaysWalkFrom tree spheres on the host,
                                        // larger uploads and every device-resident update on the device; 2 = the device for uploads too; 0 = the fixed (halved) shape
    int bvh_min = 56;                   // scenes with at least this many spheres inside the tree use it (0 = never)
    int bvh_lds_limit = 31 * 1024;      // its tables are staged in LDS while five workgroups of that size fit a CU (2048 spheres: 6.2 ms from L2 with
                                        // 4-5 waves per SIMD against 9.5 ms from LDS with two workgroups per CU); larger ones are read from HBM / L2
    int bvh_top_pairs = 0;              // pairs promoted to the front of the table for the A/B walks that stage the top (rt_bvh.hip promote_top; diagnostics only,
                                        // rt_debug_set_bvh_layout: 0 = none -- the product's layout, which keeps the builders' numbering)
    int bvh_packed = 0;                 // the packed pair table behind the blob for the A/B walk that reads it (rt_bvh.hip pack_pairs; diagnostics only, 0 = none)
    int bvh_mixed = 1;                  // tables beyond that limit whose PAIRS fit it: pairs staged, slots from HBM / L2 (rt_trace_*_pairs_m); diagnostics knob: 0 = everything from L2
    // ---- the walk ----
    int walk_gate = 16, walk_round = 4; // rt_walk.inc.h: ready lanes that make the wavefront shade; pair steps in a row before a leaf step
                                        // (round 4, this kernel: 2 / 3 / 4 / 6 in a row = 5.42 / 5.37 / 5.22 / 5.45 ms on C3, profiles/r04k_walk_sweep.jsonl)
    int walk_tail = 0;                  // lanes that may be left walking when a trip's walk phase ends (0 = none: every walk runs to its end within the trip)
    int walk_forced = 0;                // 0 = measured choice (rt_ctx::choice); diagnostics: 1 = the hierarchy whenever the scene has one
    // ---- the feature plane ----
    int features_form = 0;              // 0 = the rule (features_form below); diagnostics (rt_debug_set_features_form): 1 = the sweep, 2 = the hierarchy

    // ---- what `mode` means, said once: RT_MODE_PARITY / RT_MODE_FAST, or (diagnostics build; rt_set_mode checks the range) a row of the parity
    // table as 100 + row, of the fast table as 200 + row ----
    bool by_row() const { return mode >= 100; }
    bool fast() const { return mode == RT_MODE_FAST || mode >= 200; }      // which arithmetic renders -- and which toInt packs the frame
    int row() const { return mode - (mode >= 200 ? 200 : 100); }          // (of a launch by_row())
};

// What the rule reads of a scene (rt_launch.hip scene_facts fills it from rt_ctx::scene)
struct SceneFacts {
    uint32_t n_spheres = 0, n_lights = 0;
    bool has_hierarchy = false;         // SceneState::has_hierarchy(); the members below are BvhTables' and mean something only with it
    uint32_t n_leaves = 0, n_slots = 0, stack_depth = 0;
    uint32_t n_top = 0, packed_at = 0;  // the diagnostics' tables: the promoted top of the tree, the packed pair table (0 = none)
};

// the plain sweep's tables (geometry and lights) fit LDS for this launch
inline bool sweep_tables_fit(const SceneFacts &s, int n_samples) { return lds_bytes(s.n_spheres, s.n_lights, false, n_samples) <= kLdsMax; }
// the scene has a hierarchy and the context may use it
inline bool bvh_usable(const Knobs &k, const SceneFacts &s) { return s.has_hierarchy && k.wg_waves != 1 && k.persist == 0; }

// What Choice::next_launch is told of the context and its scene for a call of n_samples passes.  `can_render`: the context has rows, a scene and
// a camera; n_tree, n_always: the spheres inside the tree and outside it
inline Choice::Facts choice_facts(const Knobs &k, const SceneFacts &s, int n_samples, bool can_render, uint32_t n_tree, uint32_t n_always) {
    Choice::Facts f;
    f.diagnostics = k.walk_forced != 0 || k.by_row();
    f.nothing_to_render = n_samples <= 0 || !can_render;         // (or the error: launch_form says which)
    f.hierarchy = bvh_usable(k, s);
    f.tables_fit = sweep_tables_fit(s, n_samples);
    f.n_tree = n_tree;
    f.n_always = n_always;
    f.n_spheres = s.n_spheres;
    f.coop_min = k.coop_min;
    f.wg_waves = k.wg_waves;
    f.persist = k.persist;
    return f;
}

// Which instance renders a launch of `form`: its role and workgroup shape (the row is rt_launch.hip's to find -- a launch by_row() takes its row
// whatever this says), and the launch parameters that go with the choice
struct Shape {
    uint8_t role = kRoleNone;           // InstanceRole
    int waves = 4;                      // wavefronts per workgroup
    bool mat_in_lds = false;            // the material tables ride along in LDS (an instance that stages no sweep tables drops it: instance_lds)
    int regen_gate = 1;                 // LaunchParams::regen_gate
};
inline Shape pick_shape(const Knobs &k, const SceneFacts &s, int n_samples, Form form) {
    Shape out;
    const size_t lds_all = lds_bytes(s.n_spheres, s.n_lights, true, n_samples);
    // materials ride along in LDS only while that keeps at least 6 workgroups per CU resident
    // (160 KiB / 24 KiB); larger scenes read them from L2 once per hit
    out.mat_in_lds = lds_all <= (size_t)k.mat_lds_limit;
    const size_t lds_sweep = lds_bytes(s.n_spheres, s.n_lights, out.mat_in_lds, n_samples);

    // which instance: arithmetic mode x role x workgroup shape.  Single-wavefront workgroups (8x8 tiles) keep the wave
    // slots of a CU full (a 4-wavefront workgroup waits for four free slots at once) and give the heavy-first order a
    // finer granule; each stages its own copy of the tables, so only while 24 copies fit a CU.
    const bool coop = form == Form::SweepCoop ? true : (form == Form::SweepPlain ? false : (k.coop_min > 0 && s.n_spheres >= (uint32_t)k.coop_min));
    const bool w1 = k.wg_waves == 1 || (k.wg_waves == 0 && lds_sweep + (coop ? 1536u : 256u) <= 6 * 1024);   // + the instance's static LDS
    out.role = coop ? kRoleCoop : kRolePlain;
    out.waves = w1 ? 1 : 4;
    out.regen_gate = k.regen_gate > 0 ? k.regen_gate : (s.n_spheres <= 512 ? 8 : 1);
    if (!sweeps(form) && bvh_usable(k, s)) {
        // large scenes: the walk over the hierarchy, from LDS while its tables leave room for five workgroups per CU; otherwise the walk reads them
        // from HBM / L2 -- but for its PAIRS (header | pairs | stacks) where at least those fit: the chain of dependent fetches a walk consists of then stays in LDS
        const size_t all = lds_bytes_pairs(s.n_spheres, s.n_lights, false, n_samples, s.n_leaves, s.n_slots, s.stack_depth, 256);
        const size_t pairs = lds_bytes_pairs(0, 0, false, n_samples, s.n_leaves, 0, s.stack_depth, 256);
        out.role = all <= (size_t)k.bvh_lds_limit ? kRolePairs : (k.bvh_mixed != 0 && pairs <= (size_t)k.bvh_lds_limit ? kRolePairsMixed : kRolePairsGlobal);
        out.waves = 4;
        if (k.regen_gate <= 0) out.regen_gate = k.walk_gate;
    } else if (lds_bytes(s.n_spheres, s.n_lights, false, n_samples) > (size_t)(k.sweep_lds_limit < (int)kLdsMax ? k.sweep_lds_limit : (int)kLdsMax)) {
        // no hierarchy (or it lost the measurement) and a table beyond the sweep's LDS budget: the plain sweep over the table in HBM / L2.  Tables are
        // staged while at least four workgroups of that size fit a CU; larger ones go through the scalar cache (rt_trace_*_g), which keeps six wavefronts
        // per SIMD at any size: a sweep over 96 KB of staged tables runs ONE workgroup per CU and takes five times as long (Knobs::sweep_lds_limit)
        out.role = kRoleSweepGlobal;
        out.waves = 4;
    }
    if (k.persist != 0 && !k.by_row()) {        // diagnostics: persistent wavefronts
        out.role = coop ? kRolePersistCoop : kRolePersist;
        out.waves = 4;
    }
    return out;
}

// ---- the feature plane (rt_features_async) -------------------------------------------------------------
// Which kernel forms it: the plain sweep of rt_features.hip, pixels x records, or ONE closest-hit query per pixel through the hierarchy
// (rt_walk.inc.h rt_features_pairs*), at the table placement the render walk's LDS limits give.  The plane is one query per pixel and times nothing:
// workgroup shape, persistent wavefronts and the render path's hierarchy-against-sweep measurement do not enter.
enum FeaturesForm : int {
    kFeaturesSweep = 0,     // rt_features_kernel
    kFeaturesPairs,         // rt_features_pairs: header, pairs, slots and stacks in LDS
    kFeaturesPairsM,        // rt_features_pairs_m: the pairs staged, the slots where they lie in HBM / L2
    kFeaturesPairsG,        // rt_features_pairs_g: pairs and slots where they lie
};
// Scenes of at least this many records that have a hierarchy form their plane through it.  MEASURED (tools/features_probe.py,
// profiles/r35_features_walk.jsonl: the smallest probed count from which the hierarchy is faster at 800x600 and at 1920x1080 and stays faster at
// every larger probed count).  The hierarchy never lost, from 57 records -- the smallest random scene that has one -- to 262 144: so this is 56,
// the fewest tree spheres a hierarchy is built from (Knobs::bvh_min), and the rule's first clause decides alone
constexpr uint32_t kFeaturesWalkMin = 56;
inline bool features_walks(int form) { return form != kFeaturesSweep; }
// `s` describes the scene AFTER refresh_tables (has_hierarchy: the blob describes the records as they are).  Knobs::features_form forces either side
// (diagnostics): 2 on a scene without a hierarchy still answers kFeaturesSweep, and rt_features_async refuses
inline FeaturesForm features_form(const Knobs &k, const SceneFacts &s) {
    if (!s.has_hierarchy || k.features_form == 1) return kFeaturesSweep;
    if (k.features_form != 2 && s.n_spheres < kFeaturesWalkMin) return kFeaturesSweep;
    const size_t all = lds_bytes_pairs(0, 0, false, 0, s.n_leaves, s.n_slots, s.stack_depth, 256);
    const size_t pairs = lds_bytes_pairs(0, 0, false, 0, s.n_leaves, 0, s.stack_depth, 256);
    return all <= (size_t)k.bvh_lds_limit ? kFeaturesPairs : (k.bvh_mixed != 0 && pairs <= (size_t)k.bvh_lds_limit ? kFeaturesPairsM : kFeaturesPairsG);
}
// the dynamic LDS of a form that walks: hdr | pairs | slots | stacks, what is not staged left out (a workgroup is 256 lanes)
inline size_t features_lds(int form, const SceneFacts &s) {
    return form == kFeaturesPairs    ? lds_bytes_pairs(0, 0, false, 0, s.n_leaves, s.n_slots, s.stack_depth, 256)
           : form == kFeaturesPairsM ? lds_bytes_pairs(0, 0, false, 0, s.n_leaves, 0, s.stack_depth, 256)
           : form == kFeaturesPairsG ? lds_bytes_pairs(0, 0, false, 0, 1, 0, s.stack_depth, 256)
                                     : 0;
}

// The dynamic LDS an instance of table kind `tables` needs for the scene, checked against what the scene has
enum InstanceLds : int {
    kLdsOk = 0,
    kLdsNoHierarchy,        // the instance walks a hierarchy and the scene has none
    kLdsNoPackedTable,      // ... reads the packed pair table and the hierarchy has none
    kLdsNoPromotedTop,      // ... stages the promoted top of the tree and the hierarchy has none
    kLdsUnknownKind,
    kLdsBeyondMax,          // more than kLdsMax (*lds says how much)
};
inline int instance_lds(uint8_t tables, int waves, uint8_t flags, const SceneFacts &s, bool mat_in_lds, int n_samples, size_t *lds) {
    *lds = 0;
    if (walks_hierarchy(tables) && !s.has_hierarchy) return kLdsNoHierarchy;
    switch (tables) {
        case kTabSweepLds:
            *lds = lds_bytes(s.n_spheres, s.n_lights, mat_in_lds, n_samples);
            break;
        case kTabSweepGlobal:
            *lds = lds_bytes(0, 0, false, n_samples);
            break;
        case kTabPairsLds:                  // (the walk reads a hit's material by slot from the hierarchy's blob: nothing of it is staged)
            *lds = lds_bytes_pairs(s.n_spheres, s.n_lights, false, n_samples, s.n_leaves, s.n_slots, s.stack_depth, 64 * waves * ((flags & kInstTwoRays) ? 2 : 1));
            break;
        case kTabPairsGlobal:
            *lds = lds_bytes_pairs(0, 0, false, n_samples, 1, 0, s.stack_depth, 64 * waves);
            break;
        case kTabPairsLdsSlotsGlobal:
            *lds = lds_bytes_pairs(0, 0, false, n_samples, s.n_leaves, 0, s.stack_depth, 64 * waves);
            break;
        case kTabPairsPacked:               // header | the packed table's frame | stacks
            if (s.packed_at == 0 && s.n_leaves >= 2) return kLdsNoPackedTable;     // (a tree of one leaf has no pairs: the walk starts at the leaf and the frame is never used)
            *lds = lds_bytes_pairs(0, 0, false, n_samples, 1, 0, s.stack_depth, 64 * waves) + 32;
            break;
        case kTabPairsTopLds:               // header | the promoted top of the tree (n_top pairs = "n_top + 1 leaves") | stacks
            if (s.n_top == 0 && s.n_leaves >= 2) return kLdsNoPromotedTop;         // (without a promoted top the root is not pair 0: rt_debug_set_bvh_layout asks for one)
            *lds = lds_bytes_pairs(0, 0, false, n_samples, s.n_top + 1, 0, s.stack_depth, 64 * waves);
            break;
        default:
            return kLdsUnknownKind;
    }
    return *lds > kLdsMax ? kLdsBeyondMax : kLdsOk;
}

}  // namespace rt
