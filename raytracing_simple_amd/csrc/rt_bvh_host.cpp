// rt_bvh_host.cpp -- the hierarchy's host work (rt_bvh_host.h): plain C++, nothing of HIP, so that it runs and is sanitized where
// there is no device (tools/sanitize/bvh_main.cpp).  The device's builders are rt_bvh.hip's kernels; all four write the same layout.
#include "rt_bvh_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rt {

namespace {

inline float bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline Float4 make4(float x, float y, float z, float w) { return Float4{ x, y, z, w }; }
inline float coord(const rt_sphere &s, int axis) { return axis == 0 ? s.p.x : (axis == 1 ? s.p.y : s.p.z); }
inline bool finite_record(const rt_sphere &s) { return fabsf(s.rad) <= 3.0e38f && fabsf(s.p.x) <= 3.0e38f && fabsf(s.p.y) <= 3.0e38f && fabsf(s.p.z) <= 3.0e38f; }

const HostBox kEmptyBox{ { 3.4e38f, 3.4e38f, 3.4e38f }, { -3.4e38f, -3.4e38f, -3.4e38f }, 0xffffffffu };
inline double box_area(const HostBox &b) {
    const double dx = (double)b.hi[0] - b.lo[0], dy = (double)b.hi[1] - b.lo[1], dz = (double)b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}
inline HostBox box_union(const HostBox &l, const HostBox &r) {
    HostBox u = l;
    for (int a = 0; a < 3; ++a) {
        u.lo[a] = fminf(l.lo[a], r.lo[a]);
        u.hi[a] = fmaxf(l.hi[a], r.hi[a]);
    }
    u.low = l.low < r.low ? l.low : r.low;
    return u;
}

// The cut: a sphere stays outside the tree when it is of the SCENE's size -- a ground plane, a wall: its box would lie over every box above it, every
// ray visits it anyway.  16 x the median radius says that for scenes of one size class (every BASELINE and reference scene: their cut is this term).
// A scene of two classes -- thousands of small spheres ("dust") among hundreds of objects fifty times their size -- put every object outside by that
// term alone, and every ray swept them all: 6 000 small + 4 000 large spheres 27 ms a pass at 1080p against 0.5 ms for the small ones alone
// (profiles/r06_always_list.jsonl).  So the cut is never below an eighth of the extent of the scene itself: the 2 % .. 98 % range of the centres of the
// spheres under the first term, along the widest axis (quantiles: one record far away does not stretch it).  Nothing else depends on it: the
// builders take the radius range for the walk's pad from what is IN the tree.
// Returns false when no record has a radius to take the scale from.
bool cut_radius(const rt_sphere *sph, uint32_t n, const uint8_t *dup, float *r_cut_out, float *r_floor_out) {
    auto repeated = [&](uint32_t i) { return dup && dup[i] != 0; };
    std::vector<float> radii;
    radii.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float r = fabsf(sph[i].rad);
        if (r <= 3.0e38f && r > 0.f) radii.push_back(r);       // (zero-radius records -- the loader's phantoms -- say nothing about the scene's scale)
    }
    if (radii.empty()) return false;
    std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
    const float r_median = radii[radii.size() / 2];
    float r_cut = 16.f * r_median;
    // (asked only when the first term would put MORE THAN 8 spheres outside: a ground plane, six walls, a light are swept at no cost worth a hierarchy,
    // and every scene that has no more than those -- every BASELINE and reference scene -- pays nothing for the question.  Not more than 8: in a scene of
    // 150 spheres with radii over three decades, 15 above the first term cost the walk as much as its tree -- 0.50 against 0.20 ms, profiles/r06_choice_fuzz.jsonl)
    uint32_t n_over = 0;
    for (uint32_t i = 0; i < n && n_over <= 8; ++i) n_over += (fabsf(sph[i].rad) > r_cut && finite_record(sph[i]) && !repeated(i)) ? 1u : 0u;
    if (n_over > 8) {
        std::vector<float> axis[3];
        for (uint32_t i = 0; i < n; ++i) {
            const rt_sphere &s = sph[i];
            if (repeated(i) || bvh_outside(s.rad, s.p.x, s.p.y, s.p.z, r_cut) || !(fabsf(s.rad) > 0.f)) continue;
            axis[0].push_back(s.p.x);
            axis[1].push_back(s.p.y);
            axis[2].push_back(s.p.z);
        }
        float extent = 0.f;
        if (axis[0].size() >= 50)
            for (int a = 0; a < 3; ++a) {
                const size_t m = axis[a].size(), lo = m / 50, hi = m - 1 - m / 50;
                std::nth_element(axis[a].begin(), axis[a].begin() + lo, axis[a].end());
                const float q_lo = axis[a][lo];
                std::nth_element(axis[a].begin(), axis[a].begin() + hi, axis[a].end());
                extent = std::max(extent, axis[a][hi] - q_lo);
            }
        if (extent <= 3.0e38f) r_cut = std::max(r_cut, extent / 8.f);
    }
    *r_cut_out = r_cut;
    *r_floor_out = r_median / 16.f;                             // radii below this are "small": bvh_half_width
    return true;
}

// The records split into the always list and the tree's spheres, both in scene order for a start, and the tree's radius range.
bool split_records(const rt_sphere *sph, uint32_t n, const uint8_t *dup, const BvhPlan &plan, BvhHostTree *t) {
    t->order.reserve(plan.n_tree);
    float rmin = 3.4e38f, rmin_all = 3.4e38f, rmax = 0.f;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_sphere &s = sph[i];
        if (dup && dup[i]) continue;
        if (bvh_outside(s.rad, s.p.x, s.p.y, s.p.z, plan.r_cut)) {
            t->always.push_back(i);
        } else {
            t->order.push_back(i);
            rmin_all = fminf(rmin_all, fabsf(s.rad));
            if (fabsf(s.rad) >= plan.r_floor) rmin = fminf(rmin, fabsf(s.rad));
            rmax = fmaxf(rmax, fabsf(s.rad));
        }
    }
    const bool have_regular = rmin < 3.4e38f;          // (bvh_half_width: the header's r_min is the smallest regular radius, smaller spheres' boxes grow by half of it)
    t->rmin = have_regular ? rmin : rmin_all;
    t->rmax = rmax;
    t->grow = have_regular ? 0.5f * t->rmin : 0.f;
    return t->always.size() == plan.n_always && t->order.size() == plan.n_tree;
}

struct Node {
    HostBox box;
    uint32_t ref;       // kBvhLeafRef | leaf, or the node's own pair
    uint32_t depth;
};

// What both shapes are made of: the spheres by a coordinate (ties go by scene index), a leaf from a range of `order`, a pair from its two children.
struct Shaper {
    const rt_sphere *sph;
    float r_floor;
    BvhHostTree &t;

    auto by_axis(int axis) const {
        const rt_sphere *s = sph;
        return [s, axis](uint32_t x, uint32_t y) {
            const float cx = coord(s[x], axis), cy = coord(s[y], axis);
            return cx < cy || (cx == cy && x < y);
        };
    }
    void grow(HostBox &b, uint32_t ix) const {
        const rt_sphere &s = sph[ix];
        const float p[3] = { s.p.x, s.p.y, s.p.z }, ar = bvh_half_width(fabsf(s.rad), r_floor, t.grow);
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = fminf(b.lo[a], bvh_down(p[a] - ar));
            b.hi[a] = fmaxf(b.hi[a], bvh_up(p[a] + ar));
        }
        b.low = ix < b.low ? ix : b.low;
    }
    Node leaf(size_t first, size_t last) const {            // leaves are numbered in the order they are made
        Node out{ kEmptyBox, kBvhLeafRef | t.n_leaves(), 1u };
        t.leaf_first.push_back((uint32_t)first);
        t.leaf_count.push_back((uint32_t)(last - first));
        for (size_t j = first; j < last; ++j) grow(out.box, t.order[j]);
        return out;
    }
    Node pair(uint32_t mid, const Node &L, const Node &R) const {       // the inner node in front of leaf `mid`: its pair sits at mid - 1
        if (t.pair_rows.size() < 4 * (size_t)mid) t.pair_rows.resize(4 * (size_t)mid, make4(0.f, 0.f, 0.f, 0.f));
        const Node *side[2] = { &L, &R };
        for (int sd = 0; sd < 2; ++sd) {
            const HostBox &b = side[sd]->box;
            ((side[sd]->ref & kBvhLeafRef) ? t.area_leaf : t.area_inner) += box_area(b);
            t.pair_rows[4 * (size_t)(mid - 1) + 2 * sd] = make4(b.lo[0], b.lo[1], b.lo[2], bits_float(side[sd]->ref));
            t.pair_rows[4 * (size_t)(mid - 1) + 2 * sd + 1] = make4(b.hi[0], b.hi[1], b.hi[2], bits_float(b.low));
        }
        return Node{ box_union(L.box, R.box), mid - 1u, 1u + (L.depth > R.depth ? L.depth : R.depth) };
    }
    void finish(const Node &root) const {
        t.root_box = root.box;
        t.root_ref = t.n_leaves() > 1 ? root.ref : kBvhLeafRef;
        t.depth = root.depth;
    }
};

}  // namespace

uint32_t bvh_mark_repeats(const rt_sphere *sph, uint32_t n, std::vector<uint8_t> &flags) {
    uint32_t cap = 16;
    while (cap < 2u * n) cap *= 2;
    static thread_local std::vector<uint32_t> table;    // open addressing over the four words: record index + 1
    table.assign(cap, 0u);
    flags.assign(n, 0);
    auto key_of = [&](uint32_t i, uint32_t k[4]) {
        const rt_sphere &s = sph[i];
        const float rr = s.rad * s.rad;
        memcpy(&k[0], &s.p.x, 4); memcpy(&k[1], &s.p.y, 4); memcpy(&k[2], &s.p.z, 4); memcpy(&k[3], &rr, 4);
    };
    uint32_t found = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t k[4];
        key_of(i, k);
        if (!finite_record(sph[i])) continue;           // (NaN never equals itself; infinities stay as they are)
        uint32_t h = k[0] * 0x9E3779B1u ^ (k[1] + 0x7F4A7C15u) * 0x85EBCA77u ^ (k[2] + 0x165667B1u) * 0xC2B2AE3Du ^ (k[3] + 0x27D4EB2Fu) * 0x2545F491u;
        h ^= h >> 15;
        for (uint32_t at = h & (cap - 1);; at = (at + 1) & (cap - 1)) {
            const uint32_t e = table[at];
            if (e == 0u) { table[at] = i + 1u; break; }
            uint32_t q[4];
            key_of(e - 1u, q);
            if (q[0] == k[0] && q[1] == k[1] && q[2] == k[2] && q[3] == k[3]) { flags[i] = 1; found += 1; break; }
        }
    }
    return found;
}

bool bvh_plan(const rt_sphere *sph, uint32_t n, const uint8_t *dup, uint32_t n_dups, BvhPlan *plan) {
    if (!cut_radius(sph, n, dup, &plan->r_cut, &plan->r_floor)) return false;
    plan->n_tree = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_sphere &s = sph[i];
        plan->n_tree += ((dup && dup[i]) || bvh_outside(s.rad, s.p.x, s.p.y, s.p.z, plan->r_cut)) ? 0u : 1u;
    }
    plan->n_always = n - n_dups - plan->n_tree;
    return true;
}

// The halved shape: leaves of kBvhLeaf spheres, leaf ranges split in the middle -- the same tree rt_bvh_build_kernel builds (same
// split, same top-down median ordering, same leaves, same sibling pairs, boxes rounded outwards the same way).  Small uploads, whose
// surface areas the host then knows, and trees beyond what one workgroup sorts in LDS (milliseconds of host time at that size).
bool bvh_shape_halved(const rt_sphere *sph, uint32_t n, const uint8_t *dup, const BvhPlan &plan, BvhHostTree *tree) {
    if (!split_records(sph, n, dup, plan, tree)) return false;
    const Shaper sh{ sph, plan.r_floor, *tree };
    std::vector<uint32_t> &order = tree->order;
    const uint32_t n_tree = plan.n_tree, n_leaves = (n_tree + kBvhLeaf - 1) / kBvhLeaf;
    // order: top-down, every node's spheres partitioned at the median along the longest axis of the box of their centres
    // (the left child takes the first half of the node's leaves; ties go by scene index), as the device build does
    struct Range { uint32_t a, b; };
    std::vector<Range> todo{ { 0, n_leaves } };
    while (!todo.empty()) {
        const Range rg = todo.back();
        todo.pop_back();
        if (rg.b - rg.a <= 1) continue;
        const size_t first = (size_t)rg.a * kBvhLeaf, last = std::min((size_t)rg.b * kBvhLeaf, (size_t)n_tree);
        float lo[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, hi[3] = { -3.4e38f, -3.4e38f, -3.4e38f };
        for (size_t j = first; j < last; ++j)
            for (int a3 = 0; a3 < 3; ++a3) {
                lo[a3] = fminf(lo[a3], coord(sph[order[j]], a3));
                hi[a3] = fmaxf(hi[a3], coord(sph[order[j]], a3));
            }
        const float ext[3] = { hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2] };
        int axis = 0;
        if (ext[1] > ext[axis]) axis = 1;
        if (ext[2] > ext[axis]) axis = 2;
        const uint32_t mid = (rg.a + rg.b) / 2;
        const size_t cut = std::min((size_t)mid * kBvhLeaf, last);
        std::nth_element(order.begin() + first, order.begin() + cut, order.begin() + last, sh.by_axis(axis));
        todo.push_back({ rg.a, mid });
        todo.push_back({ mid, rg.b });
    }
    // leaves and sibling pairs: a recursion over leaf ranges (a range's box is the union of its halves'; depth = log2 of the leaf count: 15 at most)
    auto range = [&](uint32_t a, uint32_t b, auto &&self) -> Node {
        if (b - a == 1) return sh.leaf((size_t)a * kBvhLeaf, std::min((size_t)b * kBvhLeaf, (size_t)n_tree));
        const uint32_t mid = (a + b) / 2;
        const Node L = self(a, mid, self), R = self(mid, b, self);
        return sh.pair(mid, L, R);
    };
    sh.finish(range(0, n_leaves, range));
    return true;
}

// The same tables with the tree's SHAPE chosen by surface area (a full scene upload, where the host has the records and the call
// blocks anyway).  Top-down: a node's spheres are
// sorted along each axis in turn and cut where  area(left) * leaves(left) + area(right) * leaves(right)  is smallest
// (leaves(n) = ceil(n / 8): the cost of a visit is a leaf's eight sphere tests whether the leaf is full or not, so partial
// leaves are made only where they pay); 8 spheres or fewer are a leaf.  Leaves are numbered in the order the recursion emits
// them, every subtree holds a contiguous range of them, and the pair of a node sits at (first leaf of its right child) - 1 --
// the numbering of the fixed shape, which never depended on where the split lies.  The root's pair goes out through
// the header since it is no longer n_leaves / 2 - 1.  Against the fixed shape, on C3's rays (a host model, profiles/r03y_tree_shape_model.txt): pair
// steps per ray -15 % (shadow rays -28 %), leaf visits -7 %.  tree->too_deep: the result is not to be used (the caller then takes
// the fixed shape), as when it does not fit the tables' allocation.
constexpr uint32_t kSahMaxDepth = 30;
bool bvh_shape_by_area(const rt_sphere *sph, uint32_t n, const uint8_t *dup, const BvhPlan &plan, BvhHostTree *tree) {
    if (!split_records(sph, n, dup, plan, tree)) return false;
    const Shaper sh{ sph, plan.r_floor, *tree };
    std::vector<uint32_t> &order = tree->order;
    std::vector<double> right_area;
    auto build = [&](size_t first, size_t last, uint32_t depth, auto &&self) -> Node {
        const size_t count = last - first;
        if (depth > kSahMaxDepth) tree->too_deep = true;
        if (count <= (size_t)kBvhLeaf) return sh.leaf(first, last);
        size_t cut;
        if (tree->too_deep) {
            // (the rest becomes leaves of 8 in whatever order it is in -- the result is discarded anyway)
            cut = std::min(((count / 2 + kBvhLeaf - 1) / kBvhLeaf) * kBvhLeaf, count - 1);
        } else {
            int best_axis = 0;
            size_t best_cut = count / 2;
            double best = 1e300;
            right_area.resize(count);
            for (int axis = 0; axis < 3; ++axis) {
                std::sort(order.begin() + first, order.begin() + last, sh.by_axis(axis));
                HostBox b = kEmptyBox;
                for (size_t i = count; i-- > 1;) {              // right_area[i] = area of spheres [i, count)
                    sh.grow(b, order[first + i]);
                    right_area[i] = box_area(b);
                }
                b = kEmptyBox;
                for (size_t c = 1; c < count; ++c) {
                    sh.grow(b, order[first + c - 1]);
                    const double cost = box_area(b) * (double)((c + kBvhLeaf - 1) / kBvhLeaf) +
                                        right_area[c] * (double)((count - c + kBvhLeaf - 1) / kBvhLeaf);
                    if (cost < best) {
                        best = cost;
                        best_axis = axis;
                        best_cut = c;
                    }
                }
            }
            if (best_axis != 2) std::sort(order.begin() + first, order.begin() + last, sh.by_axis(best_axis));
            cut = best_cut;
        }
        const Node L = self(first, first + cut, depth + 1, self);
        const uint32_t mid = tree->n_leaves();
        const Node R = self(first + cut, last, depth + 1, self);
        return sh.pair(mid, L, R);
    };
    sh.finish(build(0, order.size(), 1u, build));
    return true;
}

void bvh_emit(const BvhHostTree &t, const rt_sphere *sph, Float4 *blob) {
    const uint32_t n_always = (uint32_t)t.always.size(), n_leaves = t.n_leaves(), n_slots = t.n_slots();
    Float4 *hdr = blob, *slots = blob + bvh_slots_at(), *pairs = blob + bvh_pairs_at(n_slots);
    Float4 *emis = blob + bvh_emis_at(n_leaves, n_slots), *colr = blob + bvh_colr_at(n_leaves, n_slots);
    uint32_t *index = reinterpret_cast<uint32_t *>(blob + bvh_index_at(n_slots));
    // the index words: the always list, then kBvhLeaf per leaf (padding: ~0), whole float4s of them
    for (uint32_t k = 0; k < n_always; ++k) index[k] = t.always[k];
    for (uint32_t l = 0; l < n_leaves; ++l)
        for (uint32_t q = 0; q < (uint32_t)kBvhLeaf; ++q) index[n_always + (size_t)kBvhLeaf * l + q] = q < t.leaf_count[l] ? t.order[t.leaf_first[l] + q] : 0xffffffffu;
    for (uint32_t j = n_slots; j < (n_slots + 3u) / 4u * 4u; ++j) index[j] = 0u;
    // what a ray test reads, and the material records, by slot; padding records never hit (NaN centre: every comparison of the test is false)
    const float qnan = bits_float(0x7fc00000u);
    for (uint32_t j = 0; j < n_slots; ++j) {
        const uint32_t ix = index[j];
        if (ix == 0xffffffffu) {
            slots[j] = make4(qnan, qnan, qnan, qnan);
            emis[j] = colr[j] = make4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const rt_sphere &s = sph[ix];
        float refl_bits;
        memcpy(&refl_bits, &s.refl, 4);
        slots[j] = make4(s.p.x, s.p.y, s.p.z, s.rad * s.rad);
        emis[j] = make4(s.e.x, s.e.y, s.e.z, refl_bits);
        colr[j] = make4(s.c.x, s.c.y, s.c.z, s.rad);
    }
    for (size_t k = 0; k < 4 * (size_t)(n_leaves ? n_leaves - 1 : 0); ++k) pairs[k] = k < t.pair_rows.size() ? t.pair_rows[k] : make4(0.f, 0.f, 0.f, 0.f);
    // the header: root box (centre, half diagonal) and radius range
    const HostBox &rb = t.root_box;
    const float cx = 0.5f * rb.lo[0] + 0.5f * rb.hi[0], cy = 0.5f * rb.lo[1] + 0.5f * rb.hi[1], cz = 0.5f * rb.lo[2] + 0.5f * rb.hi[2];
    const float ex = rb.hi[0] - cx, ey = rb.hi[1] - cy, ez = rb.hi[2] - cz;
    hdr[0] = make4(cx, cy, cz, sqrtf(ex * ex + ey * ey + ez * ez) * 1.001f);
    hdr[1] = make4(t.rmin, t.rmax, 1.f / (2.f * t.rmin), bits_float(t.root_ref));
}

bool bvh_estimate(const BvhHostTree &t, double *pairs, double *leaves) {
    const double a_root = box_area(t.root_box);
    const bool valid = a_root > 0.0 && std::isfinite(a_root);
    *pairs = valid ? (t.n_leaves() > 1 ? 1.0 : 0.0) + t.area_inner / a_root : 0.0;
    *leaves = valid ? (t.n_leaves() == 1 ? a_root : t.area_leaf) / a_root : 0.0;
    return valid;
}

}  // namespace rt
