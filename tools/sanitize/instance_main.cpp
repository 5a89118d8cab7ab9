// The rule that says which kernel instance a launch gets (csrc/rt_instance.h) alone, under AddressSanitizer + UndefinedBehaviorSanitizer: the knobs, what
// the rule reads of a scene, pick_shape(), instance_lds(), tile_width(), the mode's meaning and the filling of Choice::Facts -- no HIP, no device.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I raytracing_simple_amd/csrc tools/sanitize/instance_main.cpp -o instance_san && ./instance_san
// One line per case ("ok <case>" / "FAILED <case>: ..."), then "instance: clean"; the exit status is the number of failed cases.
// The expectations are literals, worked out by hand from the formulas of rt_device.h and rt_launch.hip as they stood before the rule had a file of
// its own (lds_bytes, lds_bytes_pairs, choose_instance, bind_tables); the arithmetic stands beside each.  Throughout:
//   sweep(n, L, mat, p)  = round16(16 n + 32 L + (mat ? 32 n : 0) + (p <= 1024 ? 4 p : 0))
//   pairs(n_leaves, n_slots, L, depth, lanes, p) = round16(16 (2 + 4 (n_leaves - 1) + n_slots) + 32 L + round16(2 depth lanes) + (p <= 1024 ? 4 p : 0))
// The hierarchies are real ones: profiles/r29_instance_facts.jsonl (tools/record_instance_facts.py), each row with the kernel the library picked before.
#include <cstdio>
#include <cstring>
#include <string>

#include "rt_choice.h"
#include "rt_instance.h"

using namespace rt;

namespace {
int g_failed = 0;
std::string g_why;
void expect(bool ok, const char *what) {
    if (!ok) { g_why += g_why.empty() ? "" : "; "; g_why += what; }
}
#define EXPECT(cond) expect((cond), #cond)
void done(const char *name) {
    if (g_why.empty()) printf("ok %s\n", name);
    else { printf("FAILED %s: %s\n", name, g_why.c_str()); g_failed += 1; }
    g_why.clear();
}

SceneFacts flat(uint32_t n_spheres, uint32_t n_lights) {     // a scene without a hierarchy
    SceneFacts s;
    s.n_spheres = n_spheres;
    s.n_lights = n_lights;
    return s;
}
SceneFacts tree(uint32_t n_spheres, uint32_t n_lights, uint32_t n_leaves, uint32_t n_slots, uint32_t stack_depth) {
    SceneFacts s = flat(n_spheres, n_lights);
    s.has_hierarchy = true;
    s.n_leaves = n_leaves;
    s.n_slots = n_slots;
    s.stack_depth = stack_depth;
    return s;
}
bool is(const Shape &sh, int role, int waves) { return sh.role == role && sh.waves == waves; }

// profiles/r29_instance_facts.jsonl: random_spheres(1024) = C3, _many_spheres(2000), _many_spheres(5000)
SceneFacts c3() { return tree(1024, 1, 129, 1033, 9); }
SceneFacts slab2000() { return tree(2000, 1, 250, 2001, 11); }
SceneFacts slab5000() { return tree(5000, 1, 625, 5001, 13); }

void small_scene_plain_w1() {
    const Knobs k;
    const SceneFacts demo = flat(6, 1);
    // sweep(6, 1, mat, 64) = 96 + 32 + 192 + 256 = 576 <= 24 576: materials staged; 576 + 256 = 832 <= 6144: one wavefront; 6 < 12: plain; 6 <= 512: gate 8
    Shape sh = pick_shape(k, demo, 64, Form::Auto);
    EXPECT(is(sh, kRolePlain, 1));
    EXPECT(sh.mat_in_lds);
    EXPECT(sh.regen_gate == 8);
    // the cooperative arm of the small-scene measurement: 576 + 1536 = 2112 <= 6144
    sh = pick_shape(k, demo, 64, Form::SweepCoop);
    EXPECT(is(sh, kRoleCoop, 1));
    EXPECT(sh.mat_in_lds);
    EXPECT(is(pick_shape(k, demo, 64, Form::SweepPlain), kRolePlain, 1));
    EXPECT(is(pick_shape(k, demo, 64, Form::Sweep), kRolePlain, 1));
    done("small_scene_plain_w1");
}

void coop_from_twelve() {
    Knobs k;
    EXPECT(is(pick_shape(k, flat(11, 1), 1, Form::Auto), kRolePlain, 1));
    EXPECT(is(pick_shape(k, flat(12, 1), 1, Form::Auto), kRoleCoop, 1));        // sweep(12, 1, mat, 1) = 192 + 32 + 384 + 4 -> 624; + 1536 <= 6144
    EXPECT(is(pick_shape(k, flat(12, 1), 1, Form::SweepPlain), kRolePlain, 1));    // (the form decides where it says so)
    k.coop_min = 0;
    EXPECT(is(pick_shape(k, flat(12, 1), 1, Form::Auto), kRolePlain, 1));
    EXPECT(pick_shape(k, flat(1000, 1), 1, Form::Auto).role == kRolePlain);
    k.coop_min = 5;
    EXPECT(is(pick_shape(k, flat(5, 1), 1, Form::Auto), kRoleCoop, 1));
    EXPECT(is(pick_shape(k, flat(4, 1), 1, Form::Auto), kRolePlain, 1));
    done("coop_from_twelve");
}

void w1_boundary_moves_with_the_pass_count() {
    const Knobs k;
    const SceneFacts s = flat(64, 1);
    // sweep(64, 1, mat, p) = round16(1024 + 32 + 2048 + 4 p) = round16(3104 + 4 p), materials staged throughout (<= 24 576); cooperative: + 1536 of static LDS
    EXPECT(is(pick_shape(k, s, 376, Form::Auto), kRoleCoop, 1));       // 3104 + 1504 = 4608; 4608 + 1536 = 6144 <= 6144
    EXPECT(is(pick_shape(k, s, 377, Form::Auto), kRoleCoop, 4));       // 3104 + 1508 = 4612 -> 4624; 4624 + 1536 = 6160
    EXPECT(is(pick_shape(k, s, 1024, Form::Auto), kRoleCoop, 4));      // 3104 + 4096 = 7200
    EXPECT(is(pick_shape(k, s, 1025, Form::Auto), kRoleCoop, 1));      // the table of reciprocals has left LDS: 3104 + 1536 = 4640
    // ... and the plain instance of the same scene carries 256 bytes: round16(3104 + 4 p) + 256 <= 6144 up to p = 696 (3104 + 2784 = 5888)
    EXPECT(is(pick_shape(k, s, 696, Form::SweepPlain), kRolePlain, 1));
    EXPECT(is(pick_shape(k, s, 697, Form::SweepPlain), kRolePlain, 4));     // 3104 + 2788 = 5892 -> 5904; + 256 = 6160
    done("w1_boundary_moves_with_the_pass_count");
}

void materials_leave_lds_at_24k() {
    const Knobs k;
    // sweep(n, 1, mat, 1) = round16(48 n + 36): n = 511 -> 24 564 -> 24 576; n = 512 -> 24 612 -> 24 624
    EXPECT(lds_bytes(511, 1, true, 1) == 24576);
    EXPECT(lds_bytes(512, 1, true, 1) == 24624);
    Shape sh = pick_shape(k, flat(511, 1), 1, Form::Auto);
    EXPECT(sh.mat_in_lds);
    EXPECT(is(sh, kRoleCoop, 4));
    sh = pick_shape(k, flat(512, 1), 1, Form::Auto);
    EXPECT(!sh.mat_in_lds);
    EXPECT(is(sh, kRoleCoop, 4));           // without them sweep(512, 1, no, 1) = 8192 + 36 -> 8240: beyond the single wavefront's 6144 all the same
    EXPECT(sh.regen_gate == 8);
    EXPECT(pick_shape(k, flat(513, 1), 1, Form::Auto).regen_gate == 1);     // (the gate's own threshold: 512 spheres)
    Knobs tight;
    tight.mat_lds_limit = 1024;             // sweep(21, 1, mat, 1) = 1008 + 36 -> 1056 > 1024; sweep(20, ...) = 996 -> 1008
    EXPECT(!pick_shape(tight, flat(21, 1), 1, Form::Auto).mat_in_lds);
    EXPECT(pick_shape(tight, flat(20, 1), 1, Form::Auto).mat_in_lds);
    done("materials_leave_lds_at_24k");
}

void sweep_leaves_lds_at_40k() {
    Knobs k;
    // sweep(n, 3, no, 2) = round16(16 n + 96 + 8) = 16 n + 112 <= 40 960 up to n = 2553 (40 848 + 104 = 40 952 -> 40 960); n = 2554 -> 40 976
    size_t lds = 0;
    Shape sh = pick_shape(k, flat(2553, 3), 2, Form::Auto);
    EXPECT(is(sh, kRoleCoop, 4));
    EXPECT(!sh.mat_in_lds);
    EXPECT(instance_lds(kTabSweepLds, 4, kInstStaticCoop, flat(2553, 3), sh.mat_in_lds, 2, &lds) == kLdsOk && lds == 40960);
    sh = pick_shape(k, flat(2554, 3), 2, Form::Auto);
    EXPECT(is(sh, kRoleSweepGlobal, 4));
    EXPECT(instance_lds(kTabSweepGlobal, 4, 0, flat(2554, 3), sh.mat_in_lds, 2, &lds) == kLdsOk && lds == 16);       // the two reciprocals: 8 -> 16
    EXPECT(is(pick_shape(k, flat(2554, 3), 2, Form::Sweep), kRoleSweepGlobal, 4));
    k.sweep_lds_limit = 1 << 20;            // clamps to kLdsMax = 155 648: sweep(9000, 3, no, 2) = 144 112 stays staged, sweep(10 000, 3, no, 2) = 160 112 does not
    EXPECT(is(pick_shape(k, flat(9000, 3), 2, Form::Auto), kRoleCoop, 4));
    EXPECT(is(pick_shape(k, flat(10000, 3), 2, Form::Auto), kRoleSweepGlobal, 4));
    k.sweep_lds_limit = 8 * 1024;           // sweep(505, 3, no, 2) = 8080 + 104 -> 8192; sweep(506, ...) = 8200 -> 8208
    EXPECT(is(pick_shape(k, flat(505, 3), 2, Form::Auto), kRoleCoop, 4));
    EXPECT(is(pick_shape(k, flat(506, 3), 2, Form::Auto), kRoleSweepGlobal, 4));
    done("sweep_leaves_lds_at_40k");
}

void hierarchy_roles() {
    Knobs k;
    // one pass; lanes = 256.  C3: pairs(129, 1033, 1, 9, 256, 1) = 16 * 1547 + 32 + 4608 + 4 = 29 396 -> 29 408 <= 31 744
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRolePairs, 4));
    EXPECT(is(pick_shape(k, c3(), 1, Form::Walk), kRolePairs, 4));
    // 2000 in a slab: 16 * 2999 + 32 + 5632 + 4 = 53 652 > 31 744; its pairs alone: 16 * 998 + 5632 + 4 = 21 604 -> 21 616 <= 31 744
    EXPECT(is(pick_shape(k, slab2000(), 1, Form::Auto), kRolePairsMixed, 4));
    // 5000 in a slab: the pairs alone 16 * 2498 + 6656 + 4 = 46 628 > 31 744
    EXPECT(is(pick_shape(k, slab5000(), 1, Form::Auto), kRolePairsGlobal, 4));
    EXPECT(pick_shape(k, c3(), 1, Form::Walk).regen_gate == 16);        // the walk's gate ...
    k.regen_gate = 5;
    EXPECT(pick_shape(k, c3(), 1, Form::Walk).regen_gate == 5);         // ... unless the knob is set
    k.regen_gate = 0;
    k.walk_gate = 24;
    EXPECT(pick_shape(k, c3(), 1, Form::Walk).regen_gate == 24);
    EXPECT(pick_shape(k, c3(), 1, Form::Sweep).regen_gate == 1);        // (a sweep of 1024 spheres: free-running)
    k = Knobs();
    k.bvh_mixed = 0;
    EXPECT(is(pick_shape(k, slab2000(), 1, Form::Auto), kRolePairsGlobal, 4));
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRolePairs, 4));
    k = Knobs();
    k.bvh_lds_limit = 1024;                 // C3's pairs alone: 16 * 514 + 4608 + 4 = 12 836
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRolePairsGlobal, 4));
    // the sweeps of the same scenes, one pass: sweep(1024, 1, no, 1) = 16 420 -> 16 432, sweep(2000, ...) = 32 036 -> 32 048 (both staged, both beyond one
    // wavefront's 6144), sweep(5000, ...) = 80 036 > 40 960
    k = Knobs();
    EXPECT(is(pick_shape(k, c3(), 1, Form::Sweep), kRoleCoop, 4));
    EXPECT(is(pick_shape(k, slab2000(), 1, Form::Sweep), kRoleCoop, 4));
    EXPECT(is(pick_shape(k, slab5000(), 1, Form::Sweep), kRoleSweepGlobal, 4));
    k.wg_waves = 1;                         // the hierarchy is not used; the shape is forced where the table is staged
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRoleCoop, 1));
    EXPECT(is(pick_shape(k, slab2000(), 1, Form::Auto), kRoleCoop, 1));
    EXPECT(is(pick_shape(k, slab5000(), 1, Form::Auto), kRoleSweepGlobal, 4));
    k = Knobs();
    k.wg_waves = 4;                         // (forces nothing here: a walk has four wavefronts)
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRolePairs, 4));
    EXPECT(is(pick_shape(k, flat(6, 1), 1, Form::Auto), kRolePlain, 4));
    k = Knobs();
    k.persist = 1;
    EXPECT(is(pick_shape(k, c3(), 1, Form::Auto), kRolePersistCoop, 4));
    EXPECT(is(pick_shape(k, slab2000(), 1, Form::Auto), kRolePersistCoop, 4));
    EXPECT(is(pick_shape(k, slab5000(), 1, Form::Auto), kRolePersistCoop, 4));
    EXPECT(is(pick_shape(k, flat(6, 1), 1, Form::Auto), kRolePersist, 4));
    k.mode = 137;                           // a launch by row: the persistent roles are not for it
    EXPECT(is(pick_shape(k, flat(6, 1), 1, Form::Auto), kRolePlain, 1));
    done("hierarchy_roles");
}

// profiles/r29_instance_facts.jsonl, row for row: what the library picked for real scenes before the rule moved
void recorded_scenes_get_their_kernels() {
    struct Row { const char *scene; SceneFacts s; int passes; Form form; const char *kernel; int role, waves; };
    const Row rows[] = {
        { "random_spheres(1024)", tree(1024, 1, 129, 1033, 9), 1, Form::Walk, "rt_trace_parity_pairs", kRolePairs, 4 },
        { "_many_spheres(2000)", tree(2000, 1, 250, 2001, 11), 1, Form::Walk, "rt_trace_parity_pairs_m", kRolePairsMixed, 4 },
        { "_many_spheres(5000)", tree(5000, 1, 625, 5001, 13), 1, Form::Walk, "rt_trace_parity_pairs_g", kRolePairsGlobal, 4 },
        { "_many_spheres(9500)", tree(9500, 1, 1188, 9505, 12), 1, Form::Walk, "rt_trace_parity_pairs_g", kRolePairsGlobal, 4 },
        { "mirror_box(120)", tree(120, 1, 15, 126, 5), 1, Form::Walk, "rt_trace_parity_pairs", kRolePairs, 4 },
        { "mirror_box(64)", tree(64, 1, 8, 70, 4), 1, Form::Sweep, "rt_trace_parity_coop_w1", kRoleCoop, 1 },
        { "demo_plus(16)", flat(16, 1), 1, Form::Sweep, "rt_trace_parity_coop_w1", kRoleCoop, 1 },
        { "Demo", flat(6, 1), 1, Form::SweepCoop, "rt_trace_parity_coop_w1", kRoleCoop, 1 },
    };
    const Knobs k;
    for (const Row &r : rows) {
        const Shape sh = pick_shape(k, r.s, r.passes, r.form);
        if (!is(sh, r.role, r.waves)) expect(false, r.scene);
        // the kernel's symbol says role and shape: rt_trace_parity[_coop | _pairs | _pairs_m | _pairs_g][_w1]
        const std::string name = r.kernel;
        const bool w1 = name.size() > 3 && name.compare(name.size() - 3, 3, "_w1") == 0;
        const std::string stem = w1 ? name.substr(0, name.size() - 3) : name;
        const int role = stem == "rt_trace_parity_pairs" ? kRolePairs : stem == "rt_trace_parity_pairs_m" ? kRolePairsMixed
                       : stem == "rt_trace_parity_pairs_g" ? kRolePairsGlobal : stem == "rt_trace_parity_coop" ? kRoleCoop : kRoleNone;
        if (role != r.role || (w1 ? 1 : 4) != r.waves) expect(false, r.kernel);
    }
    done("recorded_scenes_get_their_kernels");
}

void lds_per_table_kind() {
    // _many_spheres(2000)'s tree, a promoted top of 255 pairs and a packed table somewhere behind the blob; one pass, four wavefronts = 256 lanes:
    // stacks = 2 * 11 * 256 = 5632
    SceneFacts s = slab2000();
    s.n_top = 255;
    s.packed_at = 100;
    size_t lds = 0;
    EXPECT(instance_lds(kTabSweepLds, 4, 0, s, false, 1, &lds) == kLdsOk && lds == 32048);           // 32 000 + 32 + 4 = 32 036
    EXPECT(instance_lds(kTabSweepLds, 4, 0, s, true, 1, &lds) == kLdsOk && lds == 96048);            // + 64 000 = 96 036
    EXPECT(instance_lds(kTabSweepGlobal, 4, 0, s, true, 1, &lds) == kLdsOk && lds == 16);            // the reciprocal alone: 4
    EXPECT(instance_lds(kTabSweepGlobal, 4, 0, s, false, 2000, &lds) == kLdsOk && lds == 0);         // ... and beyond 1024 passes not even that
    EXPECT(instance_lds(kTabPairsLds, 4, 0, s, true, 1, &lds) == kLdsOk && lds == 53664);            // 16 * 2999 + 32 + 5632 + 4 = 53 652 (no materials, whatever is asked)
    EXPECT(instance_lds(kTabPairsLds, 4, kInstTwoRays, s, false, 1, &lds) == kLdsOk && lds == 59296);    // two stacks per lane: 47 984 + 32 + 11 264 + 4 = 59 284
    EXPECT(instance_lds(kTabPairsGlobal, 4, 0, s, false, 1, &lds) == kLdsOk && lds == 5680);         // header and stacks: 32 + 5632 + 4 = 5668
    EXPECT(instance_lds(kTabPairsGlobal, 1, 0, s, false, 1, &lds) == kLdsOk && lds == 1456);         // 64 lanes: 32 + 1408 + 4 = 1444
    EXPECT(instance_lds(kTabPairsLdsSlotsGlobal, 4, 0, s, false, 1, &lds) == kLdsOk && lds == 21616);    // 16 * 998 + 5632 + 4 = 21 604
    EXPECT(instance_lds(kTabPairsPacked, 4, 0, s, false, 1, &lds) == kLdsOk && lds == 5712);         // 5680 + the frame's 32
    EXPECT(instance_lds(kTabPairsTopLds, 4, 0, s, false, 1, &lds) == kLdsOk && lds == 22000);        // 16 * (2 + 4 * 255) + 5632 + 4 = 21 988
    // the refusals
    SceneFacts none = flat(2000, 1);
    for (int t : { kTabPairsLds, kTabPairsGlobal, kTabPairsLdsSlotsGlobal, kTabPairsTopLds, kTabPairsPacked })
        EXPECT(instance_lds((uint8_t)t, 4, 0, none, false, 1, &lds) == kLdsNoHierarchy);
    EXPECT(instance_lds(kTabSweepLds, 4, 0, none, false, 1, &lds) == kLdsOk);
    SceneFacts bare = slab2000();           // the product's layout: neither table
    EXPECT(instance_lds(kTabPairsPacked, 4, 0, bare, false, 1, &lds) == kLdsNoPackedTable);
    EXPECT(instance_lds(kTabPairsTopLds, 4, 0, bare, false, 1, &lds) == kLdsNoPromotedTop);
    SceneFacts leaf = tree(60, 1, 1, 60, 1);    // a tree of one leaf has no pairs: neither is missed.  Stacks 2 * 1 * 256 = 512
    EXPECT(instance_lds(kTabPairsPacked, 4, 0, leaf, false, 1, &lds) == kLdsOk && lds == 592);       // 32 + 512 + 4 -> 560, + 32
    EXPECT(instance_lds(kTabPairsTopLds, 4, 0, leaf, false, 1, &lds) == kLdsOk && lds == 560);
    EXPECT(instance_lds(7, 4, 0, s, false, 1, &lds) == kLdsUnknownKind);
    // 152 KB = 155 648: sweep(9725, 1, no, 1) = 155 600 + 36 -> 155 648 fits, sweep(9726, ...) = 155 652 -> 155 664 does not
    EXPECT(instance_lds(kTabSweepLds, 4, 0, flat(9725, 1), false, 1, &lds) == kLdsOk && lds == 155648);
    EXPECT(instance_lds(kTabSweepLds, 4, 0, flat(9726, 1), false, 1, &lds) == kLdsBeyondMax && lds == 155664);
    EXPECT(sweep_tables_fit(flat(9725, 1), 1) && !sweep_tables_fit(flat(9726, 1), 1));
    // the tile of a workgroup
    EXPECT(tile_width(1, 0) == 8 && tile_width(4, 0) == 32 && tile_width(4, kInstStaticCoop) == 32 && tile_width(4, kInstTwoRays) == 64);
    done("lds_per_table_kind");
}

void mode_said_once() {
    Knobs k;
    EXPECT(k.mode == 0 && !k.fast() && !k.by_row());
    k.mode = 1;
    EXPECT(k.fast() && !k.by_row());
    k.mode = 100;
    EXPECT(!k.fast() && k.by_row() && k.row() == 0);
    k.mode = 137;
    EXPECT(!k.fast() && k.by_row() && k.row() == 37);
    k.mode = 200;
    EXPECT(k.fast() && k.by_row() && k.row() == 0);
    k.mode = 215;
    EXPECT(k.fast() && k.by_row() && k.row() == 15);
    done("mode_said_once");
}

void choice_facts_from_knobs() {
    Knobs k;
    Choice::Facts f = choice_facts(k, c3(), 4, true, 1023, 1);
    EXPECT(!f.diagnostics && !f.nothing_to_render && f.hierarchy && f.tables_fit);
    EXPECT(f.n_tree == 1023 && f.n_always == 1 && f.n_spheres == 1024);
    EXPECT(f.coop_min == 12 && f.wg_waves == 0 && f.persist == 0);
    EXPECT(choice_facts(k, c3(), 0, true, 1023, 1).nothing_to_render);
    EXPECT(choice_facts(k, c3(), 4, false, 1023, 1).nothing_to_render);
    EXPECT(!choice_facts(k, flat(6, 1), 4, true, 0, 0).hierarchy);
    EXPECT(!choice_facts(k, flat(10000, 1), 4, true, 0, 0).tables_fit);     // 160 000 + 32 + 16 > 155 648
    k.mode = 137;
    EXPECT(choice_facts(k, c3(), 4, true, 1023, 1).diagnostics);
    k = Knobs();
    k.walk_forced = 1;
    EXPECT(choice_facts(k, c3(), 4, true, 1023, 1).diagnostics);
    k = Knobs();
    k.mode = RT_MODE_FAST;
    EXPECT(!choice_facts(k, c3(), 4, true, 1023, 1).diagnostics);
    k.wg_waves = 1;
    k.coop_min = 7;
    f = choice_facts(k, c3(), 4, true, 1023, 1);
    EXPECT(!f.hierarchy && f.wg_waves == 1 && f.coop_min == 7 && f.persist == 0);
    k.wg_waves = 4;
    k.persist = 1;
    f = choice_facts(k, c3(), 4, true, 1023, 1);
    EXPECT(!f.hierarchy && f.wg_waves == 4 && f.persist == 1);
    done("choice_facts_from_knobs");
}
}  // namespace

int main() {
    small_scene_plain_w1();
    coop_from_twelve();
    w1_boundary_moves_with_the_pass_count();
    materials_leave_lds_at_24k();
    sweep_leaves_lds_at_40k();
    hierarchy_roles();
    recorded_scenes_get_their_kernels();
    lds_per_table_kind();
    mode_said_once();
    choice_facts_from_knobs();
    if (g_failed == 0) printf("instance: clean\n");
    return g_failed;
}
