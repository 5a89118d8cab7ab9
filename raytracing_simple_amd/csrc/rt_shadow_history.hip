// rt_shadow_history.hip -- shadow-aware history (include/rt_api.h, "shadow-aware history"): a pixel's history ends where a moved sphere's shadow comes or goes --
//   rt_set_shadow_history    the per-context setting that rt_reproject_async INTO the context consults
//   rt_read_history_flags    the context's flag plane K, one byte per pixel
// and the kernel instances behind the setting: the reprojection kernel with its shadow arm (rules 29-32), for each of the three moments arms and both
// texel widths of the source.  Their statements are rt_reproject_body.inc.h, ONE text with rt_reproject_kernel and rt_reproject_moments_kernel, the arm
// chosen at compile time; they are instantiated HERE, in a unit of their own, so that the code objects of rt_reproject.hip and rt_moments.hip stay what
// they were: with the setting off, which is the default, every call launches the kernel it launched before.  rt_reproject_shadow_planes (rt_host.cpp)
// is the same arithmetic as plain loops; the rules' arithmetic itself is rt_rules.h, and the pair list is built by ONE function for both sides.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division), like the units it extends.
// Nothing here writes anything but dst's two temporal planes, its moments plane, its flag plane and its pair list.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::dot3;
using rt::fail;

extern "C" int rt_host_shadow_history_params(const rt_shadow_history_params *p, rt_shadow_history_params *out);      // rt_host.cpp: the parameter rule (null = defaults)
extern "C" size_t rt_host_shadow_pairs(const rt_sphere *S, const rt_sphere *D, uint32_t count, float *out, size_t cap);   // rt_host.cpp: rule 29's list

static_assert(rt::kShadowPairFloats == 20, "a pair is five float4 texels in LDS and on the device");

// rt_reproject_kernel<kCh> / rt_reproject_moments_kernel<kCh, ..> (lanes, loads and bounds are stated there) with the shadow arm.  kMom: the moments
// arm beside it (rt_plane.inc.h); out_m and m_s are null and not touched where the arm does not use them.  out_k is dst's flag plane, one byte at the
// lane's own pixel.  `pairs` holds n_pairs records of five float4; they go through s_pairs, kShadowChunk records (5120 bytes of LDS) at a time, a
// barrier either side of a chunk, and EVERY lane of the workgroup -- outside the image, over the sky, without history -- stays until the last barrier.
template <int kCh, int kMom>
__global__ void __launch_bounds__(kPlaneLanes) rt_reproject_shadow_kernel(float4 *__restrict__ out, uint32_t *__restrict__ out_px, float4 *__restrict__ out_m,
                                                                          uint8_t *__restrict__ out_k, const float4 *__restrict__ feat_d,
                                                                          const float4 *__restrict__ feat_s, const float *__restrict__ col_d,
                                                                          const float *__restrict__ u_s, const float4 *__restrict__ m_s,
                                                                          const float4 *__restrict__ geom_d, const float4 *__restrict__ geom_s,
                                                                          const float4 *__restrict__ pairs, uint32_t n_pairs, uint32_t n, rt::PixelCamera cam_d,
                                                                          rt::PixelCamera cam_s, float k_pos, float max_history, float keep, float nd, float ns, int w,
                                                                          int h, int fast) {
    static_assert(kMom != kMomentsOfPlane || kCh == 4, "S's moments plane is current only beside its temporal plane");
    constexpr bool kShadow = true;
    __shared__ float4 s_pairs[5 * kShadowChunk];
#include "rt_reproject_body.inc.h"
}

namespace rt {

// rule 29 for rt_reproject_async: the pair list of (src's records, dst's records) from the two mirrors, through dst's staging ring into dst's block on
// `stream`, without a host wait.  A list that outgrows the block replaces it (the runtime waits for the device before a block goes)
static int stage_pairs(rt_ctx *dst, const rt_ctx *src, hipStream_t stream, uint32_t *n_pairs) {
    Planes &pl = dst->planes;
    const uint32_t count = dst->scene.tables.n_spheres;
    const rt_sphere *S = src->scene.h_spheres.data(), *D = dst->scene.h_spheres.data();
    const size_t n = rt_host_shadow_pairs(S, D, count, nullptr, 0);
    *n_pairs = (uint32_t)n;
    if (n == 0) return RT_OK;
    if (n > pl.pairs_cap) {
        size_t cap = 64;
        while (cap < n) cap *= 2;
        float4 *grown = nullptr;
        RT_TRY(own_device(dst->owned, &grown, 5 * cap));
        dst->owned.drop(pl.pairs);
        pl.pairs = grown;
        pl.pairs_cap = cap;
    }
    float4 *stage = nullptr;
    RT_TRY(pl.pair_stage.acquire(dst->owned, 5 * n, &stage));
    rt_host_shadow_pairs(S, D, count, reinterpret_cast<float *>(stage), n);
    HIP_TRY(hipMemcpyAsync(pl.pairs, stage, 5 * n * sizeof(float4), hipMemcpyHostToDevice, stream));
    RT_TRY(pl.pair_stage.sent(dst->owned, stream));
    return RT_OK;
}

template <int kCh, int kMom> static auto shadow_instance() { return rt_reproject_shadow_kernel<kCh, kMom>; }

int reproject_shadow(rt_ctx *dst, rt_ctx *src, const rt_reproject_params &q, const PlaneInput &in, bool moments, hipStream_t stream) {
    Planes &pl = dst->planes;
    RT_TRY(ensure_device(dst->owned, &pl.flags, image_pixels(dst)));
    uint32_t n_pairs = 0;
    RT_TRY(stage_pairs(dst, src, stream, &n_pairs));
    const auto kernel = !moments           ? (in.channels == 4 ? shadow_instance<4, kNoMoments>() : shadow_instance<3, kNoMoments>())
                        : in.m             ? shadow_instance<4, kMomentsOfPlane>()
                        : in.channels == 4 ? shadow_instance<4, kMomentsOfLuminance>()
                                           : shadow_instance<3, kMomentsOfLuminance>();
    hipLaunchKernelGGL(kernel, plane_grid(dst->w, dst->h), dim3(kPlaneLanes), 0, stream, reinterpret_cast<float4 *>(pl.temporal), pl.temporal_px,
                       moments ? reinterpret_cast<float4 *>(pl.moments) : (float4 *)nullptr, pl.flags, reinterpret_cast<const float4 *>(dst->scene.d_features),
                       reinterpret_cast<const float4 *>(src->scene.d_features), (const float *)dst->d_colors, in.u, moments ? in.m : (const float4 *)nullptr,
                       dst->scene.tables.geom, src->scene.tables.geom, (const float4 *)pl.pairs, n_pairs, dst->scene.tables.n_spheres, pixel_camera(dst->cam),
                       pixel_camera(src->cam), q.k_pos, q.max_history, pl.shadow_set.params.keep, (float)dst->frame.current_sample, in.passes, dst->w, dst->h,
                       dst->knobs.fast() ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // namespace rt

using namespace rt;

extern "C" {

RT_API int rt_set_shadow_history(rt_ctx *c, const rt_shadow_history_params *params) {
    RT_TRY(tiles_refuse(c, "rt_set_shadow_history"));
    rt_shadow_history_params q{};
    if (params && rt_host_shadow_history_params(params, &q) != RT_OK) return RT_ERR_ARG;
    c->planes.shadow_set = { q, params != nullptr };
    return RT_OK;
}

RT_API int rt_read_history_flags(rt_ctx *c, uint8_t *k_host) {
    const char *const call = "rt_read_history_flags";
    RT_TRY(tiles_refuse(c, call));
    if (!k_host) return fail(RT_ERR_ARG, "%s: k_host is null", call);
    if (!flags_current(c))
        return fail(RT_ERR_STATE, "%s: the context holds no current flag plane (rt_reproject_async into it forms one while rt_set_shadow_history is on; whatever ends "
                                  "the temporal plane, or a reprojection into the context with the setting off, ends it)", call);
    return read_back(c, k_host, c->planes.flags, image_pixels(c));
}

}  // extern "C"
