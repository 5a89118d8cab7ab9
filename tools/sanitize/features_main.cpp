// Which kernel forms the feature plane (csrc/rt_instance.h features_form, features_lds), on the host alone, and what the hierarchy's host work
// (csrc/rt_bvh_host.cpp bvh_mark_repeats, bvh_plan) makes of a file of records -- no HIP, no device.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I raytracing_simple_amd/csrc tools/sanitize/features_main.cpp raytracing_simple_amd/csrc/rt_bvh_host.cpp -o features_san
//   ./features_san                  the rule: one line per case ("ok <case>" / "FAILED <case>: ..."), then "features: clean"; exit status = failed cases
//   ./features_san lds L S D        features_lds of the three placements for a tree of L leaves, S slots and depth D, on one line
//   ./features_san FILE             FILE holds rt_sphere records: "records N repeats D always A tree T r_cut R" and, per record, "outside I" for the
//                                   records of the always-list and "repeat I" for those that repeat an earlier one (tests/test_features_walk_cpu.py)
// The count either side of the threshold is rt::kFeaturesWalkMin itself, never a copy.  The hierarchy is a real one: random_spheres(1024) of
// profiles/r29_instance_facts.jsonl, 129 leaves, 1033 slots, depth 9:
//   all   = 16 (2 + 4 * 128 + 1033) + round16(2 * 9 * 256) = 24 752 + 4 608 = 29 360
//   pairs = 16 (2 + 4 * 128)        + 4 608                =  8 224 + 4 608 = 12 832
//   none  = 16 * 2                  + 4 608                =                   4 640
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_bvh_host.h"
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

SceneFacts flat(uint32_t n_spheres) {
    SceneFacts s;
    s.n_spheres = n_spheres;
    s.n_lights = 1;
    return s;
}
SceneFacts tree(uint32_t n_spheres, uint32_t n_leaves, uint32_t n_slots, uint32_t stack_depth) {
    SceneFacts s = flat(n_spheres);
    s.has_hierarchy = true;
    s.n_leaves = n_leaves;
    s.n_slots = n_slots;
    s.stack_depth = stack_depth;
    return s;
}
SceneFacts c3() { return tree(1024, 129, 1033, 9); }

void no_hierarchy_is_swept() {
    Knobs k;
    for (uint32_t n : { 0u, 6u, 55u, 56u, 1024u, 262144u }) EXPECT(features_form(k, flat(n)) == kFeaturesSweep);
    k.features_form = 2;                    // forced: still the sweep's answer -- rt_features_async refuses
    EXPECT(features_form(k, flat(1024)) == kFeaturesSweep);
    EXPECT(!features_walks(kFeaturesSweep) && features_walks(kFeaturesPairs) && features_walks(kFeaturesPairsM) && features_walks(kFeaturesPairsG));
    done("no_hierarchy_is_swept");
}

void count_either_side_of_the_threshold() {
    const Knobs k;
    // seven leaves of eight: the smallest tree the builders make (56 spheres)
    EXPECT(features_form(k, tree(kFeaturesWalkMin, 7, 56, 4)) == kFeaturesPairs);
    EXPECT(features_form(k, tree(kFeaturesWalkMin + 1, 7, 57, 4)) == kFeaturesPairs);
    if (kFeaturesWalkMin > 0) EXPECT(features_form(k, tree(kFeaturesWalkMin - 1, 7, 56, 4)) == kFeaturesSweep);
    EXPECT(features_form(k, tree(262144, 32768, 262145, 40)) != kFeaturesSweep);
    done("count_either_side_of_the_threshold");
}

void placements_either_side_of_the_lds_limits() {
    Knobs k;
    EXPECT(k.bvh_lds_limit == 31 * 1024 && k.bvh_mixed == 1);
    EXPECT(features_form(k, c3()) == kFeaturesPairs);
    EXPECT(features_lds(kFeaturesPairs, c3()) == 29360 && features_lds(kFeaturesPairsM, c3()) == 12832 && features_lds(kFeaturesPairsG, c3()) == 4640);
    EXPECT(features_lds(kFeaturesSweep, c3()) == 0);
    k.bvh_lds_limit = 29360;
    EXPECT(features_form(k, c3()) == kFeaturesPairs);
    k.bvh_lds_limit = 29359;
    EXPECT(features_form(k, c3()) == kFeaturesPairsM);
    k.bvh_mixed = 0;
    EXPECT(features_form(k, c3()) == kFeaturesPairsG);
    k.bvh_mixed = 1;
    k.bvh_lds_limit = 12832;
    EXPECT(features_form(k, c3()) == kFeaturesPairsM);
    k.bvh_lds_limit = 12831;
    EXPECT(features_form(k, c3()) == kFeaturesPairsG);
    k.bvh_lds_limit = 1;
    EXPECT(features_form(k, c3()) == kFeaturesPairsG);
    // the render rule's limits, without its passes and lights: a scene the render walk stages (n_samples 0, no lights) is staged here too
    k = Knobs{};
    EXPECT(pick_shape(k, c3(), 0, Form::Walk).role == kRolePairs);
    done("placements_either_side_of_the_lds_limits");
}

void render_knobs_change_nothing() {
    for (const SceneFacts &s : { c3(), tree(kFeaturesWalkMin, 7, 56, 4), flat(1024) }) {
        const FeaturesForm want = features_form(Knobs{}, s);
        Knobs k;
        k.wg_waves = 1;
        EXPECT(features_form(k, s) == want);
        k.wg_waves = 4;
        k.persist = 1;
        EXPECT(features_form(k, s) == want);
        k = Knobs{};
        k.walk_forced = 1;
        k.mode = RT_MODE_FAST;
        k.coop_min = 0;
        EXPECT(features_form(k, s) == want);
    }
    done("render_knobs_change_nothing");
}

void forced_forms() {
    Knobs k;
    k.features_form = 1;
    EXPECT(features_form(k, c3()) == kFeaturesSweep);
    k.features_form = 2;
    EXPECT(features_form(k, c3()) == kFeaturesPairs);
    if (kFeaturesWalkMin > 0) EXPECT(features_form(k, tree(kFeaturesWalkMin - 1, 7, 56, 4)) == kFeaturesPairs);       // below the threshold: the hierarchy all the same
    k.bvh_lds_limit = 1;
    EXPECT(features_form(k, c3()) == kFeaturesPairsG);
    done("forced_forms");
}

int scene_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 2; }
    std::vector<rt_sphere> sph;
    rt_sphere s;
    while (fread(&s, sizeof s, 1, f) == 1) sph.push_back(s);
    fclose(f);
    const uint32_t n = (uint32_t)sph.size();
    std::vector<uint8_t> flags;
    const uint32_t repeats = bvh_mark_repeats(sph.data(), n, flags);
    BvhPlan plan{};
    if (!bvh_plan(sph.data(), n, repeats ? flags.data() : nullptr, repeats, &plan)) { printf("records %u repeats %u always 0 tree 0 r_cut 0\n", n, repeats); return 0; }
    printf("records %u repeats %u always %u tree %u r_cut %.9g\n", n, repeats, plan.n_always, plan.n_tree, (double)plan.r_cut);
    for (uint32_t i = 0; i < n; ++i) {
        const bool rep = repeats && flags[i];
        if (rep) printf("repeat %u\n", i);
        else if (bvh_outside(sph[i].rad, sph[i].p.x, sph[i].p.y, sph[i].p.z, plan.r_cut)) printf("outside %u\n", i);
    }
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && strcmp(argv[1], "lds") == 0) {       // lds N_LEAVES N_SLOTS DEPTH: features_lds of the three placements
        const SceneFacts s = tree(0, (uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]));
        printf("%zu %zu %zu\n", features_lds(kFeaturesPairs, s), features_lds(kFeaturesPairsM, s), features_lds(kFeaturesPairsG, s));
        return 0;
    }
    if (argc > 1) return scene_file(argv[1]);
    no_hierarchy_is_swept();
    count_either_side_of_the_threshold();
    placements_either_side_of_the_lds_limits();
    render_knobs_change_nothing();
    forced_forms();
    if (!g_failed) printf("features: clean\n");
    return g_failed;
}
