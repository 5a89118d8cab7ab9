// rt_bvh_host.h -- the hierarchy's host work that needs no device (rt_bvh_host.cpp, plain C++): which records repeat an earlier
// one, the cut between the tree and the always list, and the two builders that shape a tree from the host mirror of the records
// and write the blob of rt_device.h BvhTables into a buffer of the caller's.  rt_bvh.hip stages, uploads and adopts.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/rt_api.h"
#include "rt_bvh_layout.h"

namespace rt {

struct Float4 {         // the layout of HIP's float4
    float x, y, z, w;
};

// One byte per record: 1 = the record repeats an EARLIER one bit for bit in centre and radius^2 (rt_bvh.hip mark_duplicates says why
// such a record stays out of the hierarchy).  Returns how many do.
uint32_t bvh_mark_repeats(const rt_sphere *sph, uint32_t n, std::vector<uint8_t> &flags);

// The cut and the counts every builder is launched with.  `dup`: the flags above, or null when no record repeats.
struct BvhPlan {
    float r_cut, r_floor;           // outside the tree: |rad| > r_cut or not finite (bvh_outside); "small": |rad| < r_floor (bvh_half_width)
    uint32_t n_tree, n_always;
};
bool bvh_plan(const rt_sphere *sph, uint32_t n, const uint8_t *dup, uint32_t n_dups, BvhPlan *plan);   // false: no record has a radius to take the scale from

struct HostBox {
    float lo[3], hi[3];
    uint32_t low;                   // lowest scene index inside
};
// A tree shaped on the host, before it is written out: its size is known only now (the build by surface area makes partial leaves).
struct BvhHostTree {
    std::vector<uint32_t> order, always;            // scene indices: the tree's spheres in leaf order, the always list in scene order
    float rmin = 0.f, rmax = 0.f, grow = 0.f;       // radius range of the tree's spheres (rmin: the smallest regular one, if any), growth of a small sphere's box
    std::vector<uint32_t> leaf_first, leaf_count;   // per leaf: its range of `order`
    std::vector<Float4> pair_rows;                  // 4 per pair; the pair in front of leaf m at 4 * (m - 1)
    HostBox root_box{};
    uint32_t root_ref = kBvhLeafRef, depth = 1;
    bool too_deep = false;                          // (by surface area only: the result is to be discarded)
    double area_inner = 0.0, area_leaf = 0.0;       // surface areas of the inner nodes below the root / of the leaves
    uint32_t n_leaves() const { return (uint32_t)leaf_first.size(); }
    uint32_t n_slots() const { return (uint32_t)always.size() + (uint32_t)kBvhLeaf * n_leaves(); }
};
// Both return false when the split of the records does not give the plan's counts.
bool bvh_shape_halved(const rt_sphere *sph, uint32_t n, const uint8_t *dup, const BvhPlan &plan, BvhHostTree *tree);
bool bvh_shape_by_area(const rt_sphere *sph, uint32_t n, const uint8_t *dup, const BvhPlan &plan, BvhHostTree *tree);
// the whole blob, bvh_blob_float4s(tree.n_leaves(), tree.n_slots()) float4 of it
void bvh_emit(const BvhHostTree &tree, const rt_sphere *sph, Float4 *blob);
// What a random line through the root box is expected to visit: pair steps and leaf visits (the choice between hierarchy and sweep
// is estimated from these); false when the root box has no area to divide by.
bool bvh_estimate(const BvhHostTree &tree, double *pairs, double *leaves);

}  // namespace rt
