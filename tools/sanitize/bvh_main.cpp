// The hierarchy's host builders (csrc/rt_bvh_host.cpp) under the sanitizers, on the CPU: trees of generated record sets through both
// builders, each held to cheap invariants -- every record of the plan in exactly one slot, the always list in scene order, the
// counts the plan's, every reference in range.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raytracing_simple_amd/csrc/rt_bvh_host.h"

namespace {

uint32_t g_state = 12345u;
float uniform(float lo, float hi) {
    g_state = g_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(g_state >> 8) / 16777216.f;
}

std::vector<rt_sphere> scattered(uint32_t n) {
    std::vector<rt_sphere> s(n);
    for (uint32_t i = 0; i < n; ++i) {
        memset(&s[i], 0, sizeof(rt_sphere));
        s[i].rad = uniform(0.3f, 3.f);
        s[i].p = { uniform(-90.f, 90.f), uniform(0.5f, 20.f), uniform(-90.f, 90.f) };
        s[i].c = { 0.5f, 0.5f, 0.5f };
        s[i].refl = (int)(i % 3u);
    }
    if (n > 2) { s[0].rad = 1000.f; s[0].p = { 0.f, -1000.f, 0.f }; }       // a ground: the always list
    return s;
}

// NaN, infinite, zero and negative radii, exact repeats, and a block of zero-radius records in front
std::vector<rt_sphere> hostile() {
    std::vector<rt_sphere> real = scattered(200), s(40);
    for (auto &z : s) memset(&z, 0, sizeof(rt_sphere));
    s.insert(s.end(), real.begin(), real.end());
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    s[50].rad = nan; s[51].rad = inf; s[52].rad = 0.f; s[53].rad = -2.f; s[54].p.y = -inf; s[55].p.x = nan;
    for (uint32_t k = 0; k < 12; ++k) { s[120 + k] = s[60 + k]; s[120 + k].refl = 2; }
    s[140] = s[40];                                                         // the ground, repeated
    s[141] = s[61]; s[141].rad = -s[61].rad;                                // the same radius^2
    return s;
}

int g_bad = 0;
void complain(const char *what, const char *shape, size_t n) {
    printf("FAIL %s: %s tree of %zu records\n", what, shape, n);
    g_bad += 1;
}

void check(const std::vector<rt_sphere> &sph, const uint8_t *dup, const rt::BvhPlan &plan, bool by_area) {
    const char *shape = by_area ? "by-area" : "halved";
    const uint32_t n = (uint32_t)sph.size();
    rt::BvhHostTree tree;
    if (!(by_area ? rt::bvh_shape_by_area : rt::bvh_shape_halved)(sph.data(), n, dup, plan, &tree)) return complain("the split is not the plan's", shape, n);
    const uint32_t n_leaves = tree.n_leaves(), n_slots = tree.n_slots();
    if (tree.too_deep) return complain("too deep", shape, n);
    if (tree.always.size() != plan.n_always || tree.order.size() != plan.n_tree) complain("counts", shape, n);
    if (!by_area && n_leaves != (plan.n_tree + rt::kBvhLeaf - 1) / rt::kBvhLeaf) complain("leaf count", shape, n);
    std::vector<rt::Float4> blob(rt::bvh_blob_float4s(n_leaves, n_slots));
    rt::bvh_emit(tree, sph.data(), blob.data());
    const uint32_t *index = reinterpret_cast<const uint32_t *>(blob.data() + rt::bvh_index_at(n_slots));
    std::vector<uint8_t> seen(n, 0);
    uint32_t in_tree = 0;
    for (uint32_t j = 0; j < n_slots; ++j) {
        const uint32_t ix = index[j];
        const bool padding = ix == 0xffffffffu;
        if (padding != std::isnan(blob[rt::bvh_slots_at() + j].x) && !(ix < n && std::isnan(sph[ix].p.x))) complain("padding and NaN slots disagree", shape, n);
        if (padding) {
            if (j < plan.n_always) complain("padding in the always list", shape, n);
            continue;
        }
        if (ix >= n || seen[ix]) return complain("a slot's record out of range or held twice", shape, n);
        seen[ix] = 1;
        const rt_sphere &s = sph[ix];
        if (rt::bvh_outside(s.rad, s.p.x, s.p.y, s.p.z, plan.r_cut) != (j < plan.n_always)) complain("a record on the wrong side of the cut", shape, n);
        if (j > 0 && j < plan.n_always && index[j - 1] >= ix) complain("always list out of scene order", shape, n);
        in_tree += j >= plan.n_always ? 1u : 0u;
    }
    if (in_tree != plan.n_tree) complain("tree records in the slots", shape, n);
    for (uint32_t i = 0; i < n; ++i)
        if ((seen[i] != 0) == (dup && dup[i])) complain("a record missing, or a repeat present", shape, n);
    auto ref_ok = [&](uint32_t ref) { return (ref & rt::kBvhLeafRef) ? (ref & (rt::kBvhLeafRef - 1u)) < n_leaves : ref + 1u < n_leaves; };
    const rt::Float4 *pairs = blob.data() + rt::bvh_pairs_at(n_slots);
    for (uint32_t m = 0; m + 1 < n_leaves; ++m)
        for (int side = 0; side < 2; ++side) {
            uint32_t ref, low;
            memcpy(&ref, &pairs[4 * m + 2 * side].w, 4);
            memcpy(&low, &pairs[4 * m + 2 * side + 1].w, 4);
            if (!ref_ok(ref) || low >= n) complain("a pair's reference out of range", shape, n);
        }
    uint32_t root;
    memcpy(&root, &blob[1].w, 4);
    if (!ref_ok(root) || (n_leaves == 1) != (root == rt::kBvhLeafRef)) complain("the root's reference", shape, n);
    double est_pairs, est_leaves;
    (void)rt::bvh_estimate(tree, &est_pairs, &est_leaves);
    printf("%-8s %5zu records: %u always, %u in the tree, %u leaves, %u levels, estimate %.3f / %.3f\n", shape, (size_t)n, plan.n_always, plan.n_tree, n_leaves,
           tree.depth, est_pairs, est_leaves);
}

void both(const std::vector<rt_sphere> &sph) {
    std::vector<uint8_t> flags;
    const uint32_t n = (uint32_t)sph.size(), found = rt::bvh_mark_repeats(sph.data(), n, flags);
    const uint8_t *dup = found ? flags.data() : nullptr;
    rt::BvhPlan plan;
    if (!rt::bvh_plan(sph.data(), n, dup, found, &plan)) return complain("no plan", "any", n);
    if (plan.n_tree == 0) return;
    check(sph, dup, plan, false);
    check(sph, dup, plan, true);
}

}  // namespace

int main() {
    for (uint32_t n : { 1u, 8u, 9u, 97u, 300u, 1499u, 9500u }) both(scattered(n));
    both(hostile());
    printf(g_bad ? "bvh builders: %d complaints\n" : "bvh builders: clean\n", g_bad);
    return g_bad ? 1 : 0;
}
