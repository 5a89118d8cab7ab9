// rt_plane.inc.h -- what the per-pixel kernels of the library's extensions share on the device (rt_features.hip, rt_reproject.hip, rt_atrous.hip, and
// the NL-means body of rt_denoise.inc.h): the workgroup's shape, the lane-to-pixel mapping, the launch grid, the "3 or 4 floats a texel" load and the
// pack of a filtered plane.  The rules' arithmetic itself is rt_rules.h.  Every unit that includes this is compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_detmath.h"
#include "rt_rules.h"

namespace {

constexpr int kPlaneTileW = 32, kPlaneTileH = 8, kPlaneLanes = kPlaneTileW * kPlaneTileH;      // a workgroup's pixels: four wavefronts, as the render kernels'

// The moments arm of the reprojection kernel (rt_reproject.hip; include/rt_api.h, rule 25): none, a tap's moments from the luminance of U, or from S's
// moments plane
enum { kNoMoments = 0, kMomentsOfLuminance = 1, kMomentsOfPlane = 2 };

// The shadow arm of the same kernel (rule 31): the pair list goes through LDS in chunks of this many records of five float4 -- 5120 bytes a workgroup
constexpr int kShadowChunk = RT_SHADOW_PAIR_CHUNK;

struct PlanePixel {
    int x, y;
};

// One lane per pixel, a wavefront on an 8x8 tile, the four tiles side by side.  (The NL-means body deals its lanes out by rows of 32: dn_body.)
__device__ __forceinline__ PlanePixel plane_pixel() {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    return PlanePixel{ (int)blockIdx.x * kPlaneTileW + wave * 8 + (lane & 7), (int)blockIdx.y * kPlaneTileH + (lane >> 3) };
}

// the grid whose workgroups cover a w x h plane
inline dim3 plane_grid(int w, int h) { return dim3((unsigned)((w + kPlaneTileW - 1) / kPlaneTileW), (unsigned)((h + kPlaneTileH - 1) / kPlaneTileH)); }

// The texel at array position `at` of a plane of kCh floats a pixel: rgb and n (kCh = 4, a temporal plane), or rgb and `n_all` (kCh = 3, a colour
// plane, every pixel at the same pass count)
template <int kCh>
__device__ __forceinline__ float4 plane_texel(const float *__restrict__ u, size_t at, float n_all) {
    if constexpr (kCh == 4) return reinterpret_cast<const float4 *>(u)[at];
    else return make_float4(u[3 * at], u[3 * at + 1], u[3 * at + 2], n_all);
}

// .cl:34, the pack kernel's toInt (rt_trace.inc.h to_int): parity's restated powf, or fast mode's exp2 / log2 with the fused multiply-add that
// unit's contraction makes of g * 255 + .5 (these units contract nothing, so it is written out)
__device__ __forceinline__ uint32_t dn_to_int(float v, bool fast) {
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    if (fast) return (uint32_t)(int)__builtin_fmaf(rt::fm_powf(c, 1.f / 2.2f), 255.f, .5f);
    return (uint32_t)(int)(rt::dm_powf(c, 1.f / 2.2f) * 255.f + .5f);
}

// ... of three channels, as one word of a packed plane
__device__ __forceinline__ uint32_t pack_rgb(float r, float g, float b, bool fast) { return dn_to_int(r, fast) | (dn_to_int(g, fast) << 8) | (dn_to_int(b, fast) << 16); }

}  // namespace
