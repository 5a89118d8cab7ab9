// rt_bvh_layout.h -- what every builder of the hierarchy (rt_device.h BvhTables) and its walk agree on: the leaf size, the offsets
// into the blob, and the predicates the builders apply to the same bits on the host and on the device.  Usable from plain C++
// (rt_bvh_host.cpp) and from HIP (rt_device.h includes it).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rt {

#ifndef RT_BVH_LEAF
#define RT_BVH_LEAF 8                   /* spheres per leaf (4 measured in round 4: tools/leaf_size_ab.sh) */
#endif
constexpr int kBvhLeaf = RT_BVH_LEAF;
constexpr uint32_t kBvhLeafRef = 0x8000u;
// offsets into the blob, in float4 units
RT_HD inline uint32_t bvh_slots_at() { return 2u; }
RT_HD inline uint32_t bvh_index_at(uint32_t n_slots) { return 2u + n_slots; }
RT_HD inline uint32_t bvh_pairs_at(uint32_t n_slots) { return 2u + n_slots + (n_slots + 3u) / 4u; }
RT_HD inline uint32_t bvh_emis_at(uint32_t n_leaves, uint32_t n_slots) { return bvh_pairs_at(n_slots) + 4u * (n_leaves ? n_leaves - 1u : 0u); }
RT_HD inline uint32_t bvh_colr_at(uint32_t n_leaves, uint32_t n_slots) { return bvh_emis_at(n_leaves, n_slots) + n_slots; }
inline size_t bvh_blob_float4s(uint32_t n_leaves, uint32_t n_slots) { return (size_t)bvh_colr_at(n_leaves, n_slots) + (size_t)n_slots; }
// ... and what a context allocates for a scene capacity of `scene_cap` records: hdr 2 + slots (< cap + 8; up to twice that with the partial leaves of the
// shaped tree) + index (a quarter of the slots) + pairs (< cap / 2 + 4) + two material records per slot.  A tree that needs more is not uploaded, and
// the diagnostics' tables behind the blob are made only where they fit: every such check asks here
inline size_t bvh_blob_capacity(uint32_t scene_cap) { return (size_t)scene_cap * 6 + 64; }

// A sphere stays outside the tree ("always" list, scene order kept) unless its radius and centre are finite and |rad| <= r_cut.
// Host and device agree on the counts because they apply the same test to the same bits.
RT_HD inline bool bvh_outside(float rad, float px, float py, float pz, float r_cut) {
    const float big = 3.0e38f;
    const bool finite = (fabsf(rad) <= big) && (fabsf(px) <= big) && (fabsf(py) <= big) && (fabsf(pz) <= big);   // false for NaN
    return !(finite && fabsf(rad) <= r_cut);
}
// Half the width of a sphere's box.  The walk grows every box by a per-ray pad min(sqrt(eps), eps / 2 r_min) (rt_walk.inc.h), r_min the
// smallest radius in the tree -- so ONE zero-radius record (the .scn loader's doubling puts N of them at the origin, Utility.cpp:120,154)
// would turn that into sqrt(eps) for every box of the tree and every ray: complex.scn's walk took 18 % more pair steps and 46 % more leaf
// visits for its 783 phantoms (profiles/r06_reference_scenes.jsonl).  Instead the header's r_min is the smallest REGULAR radius R
// (|rad| >= r_floor = 1/16 of the median radius) and the boxes of the smaller spheres are grown by g = R / 2 at build time: for a sphere of
// radius r_s < R the point X of the derivation lies within r_s + min(sqrt(eps), eps / 2 r_s) <= r_s + sqrt(eps) of its centre, and
// g + min(s, s^2 / 2R) >= s for every s = sqrt(eps) >= 0 (the difference s - s^2 / 2R peaks at s = R with R / 2; beyond s = 2R the pad is s itself).
// A tree without a regular sphere keeps the true minimum and g = 0, as before.
RT_HD inline float bvh_half_width(float ar, float r_floor, float g) { return ar >= r_floor ? ar : ar + g; }
// box planes are rounded outwards
RT_HD inline float bvh_down(float v) { return v - (fabsf(v) * 0x1p-22f + 1e-30f); }
RT_HD inline float bvh_up(float v) { return v + (fabsf(v) * 0x1p-22f + 1e-30f); }

}  // namespace rt
