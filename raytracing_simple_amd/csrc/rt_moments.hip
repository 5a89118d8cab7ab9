// rt_moments.hip -- temporal luminance moments (include/rt_api.h, "temporal luminance moments"): the a-trous variance from a pixel's history --
//   rt_set_temporal_moments  the per-context setting that rt_reproject_async INTO the context and rt_atrous_async OF it consult
//   rt_read_moments          the context's moments plane M, (m1, m2, k, v) per pixel (read_plane, rt_internal.h)
// and the kernel instances behind the setting: the reprojection kernel with its moments arm (rules 25-27) and the a-trous preparation kernel with
// its own (rule 28).  Their statements are those of rt_reproject_kernel and rt_atrous_prepare_kernel -- rt_reproject_body.inc.h and
// rt_atrous_prepare_body.inc.h, ONE text each -- with the arm chosen at compile time.  They are instantiated HERE, in a unit of their own, so that the
// code objects of rt_reproject.hip and rt_atrous.hip stay what they were (as rt_denoise_guided.hip does for rt_denoise.hip): with the setting off,
// which is the default, every call launches the kernel it launched before.  rt_reproject_moments_planes and rt_atrous_moments_planes (rt_host.cpp)
// are the same arithmetic as plain loops; the rules' arithmetic itself is rt_rules.h.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division and square root), like the two units it extends.
// Nothing here writes anything but dst's two temporal planes, its moments plane and the context's filter planes.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::dot3;
using rt::fail;

extern "C" int rt_host_moments_params(const rt_moments_params *p, rt_moments_params *out);     // rt_host.cpp: the parameter rule (null = defaults)

// rt_reproject_kernel<kCh> (rt_reproject.hip: lanes, loads and bounds are stated there) with the moments arm.  out_m is dst's moments plane, written at
// the lane's own pixel as one float4.  kFromPlane: m_s is S's moments plane, current beside S's temporal plane (so kCh == 4), read as one float4 at each
// tap that COUNTS -- behind the in-image test of rule 17, like U; otherwise m_s is null and not read: a tap's moments are the luminance of U.
template <int kCh, bool kFromPlane>
__global__ void __launch_bounds__(kPlaneLanes) rt_reproject_moments_kernel(float4 *__restrict__ out, uint32_t *__restrict__ out_px, float4 *__restrict__ out_m,
                                                                           const float4 *__restrict__ feat_d, const float4 *__restrict__ feat_s,
                                                                           const float *__restrict__ col_d, const float *__restrict__ u_s, const float4 *__restrict__ m_s,
                                                                           const float4 *__restrict__ geom_d, const float4 *__restrict__ geom_s, uint32_t n,
                                                                           rt::PixelCamera cam_d, rt::PixelCamera cam_s, float k_pos, float max_history, float nd, float ns,
                                                                           int w, int h, int fast) {
    constexpr int kMom = kFromPlane ? kMomentsOfPlane : kMomentsOfLuminance;
    constexpr bool kShadow = false;                         // the shadow arm (rt_shadow_history.hip) is discarded, as in rt_reproject_kernel
    constexpr const float4 *pairs = nullptr;
    constexpr uint32_t n_pairs = 0;
    constexpr float keep = 0.0f;
    constexpr uint8_t *out_k = nullptr;
    constexpr float4 *s_pairs = nullptr;
#include "rt_reproject_body.inc.h"
}

// rt_atrous_prepare_kernel<4> (rt_atrous.hip) with rule 28: U is the temporal plane -- M is current only beside it -- and m its moments plane as
// float2 pairs: texel `at` is m[2 * at] = (m1, m2) and m[2 * at + 1] = (k, v), of which the second is read, at the lane's own pixel.
__global__ void __launch_bounds__(kPlaneLanes) rt_atrous_prepare_moments_kernel(float4 *__restrict__ out, float4 *__restrict__ guide, float *__restrict__ n_out,
                                                                                uint32_t *__restrict__ px, const float *__restrict__ u, const float4 *__restrict__ feat,
                                                                                const float2 *__restrict__ m, float k_min, int w, int h, int fast) {
    constexpr int kCh = 4;
    constexpr bool kMom = true;
    constexpr float n_all = 0.0f;                           // (a temporal texel carries its own n)
#include "rt_atrous_prepare_body.inc.h"
}

namespace rt {

// for rt_reproject_async, which has checked, chained and acquired everything: T, its packed plane and M of dst on `stream`, from `in` (filter_input of src)
int reproject_moments(rt_ctx *dst, const rt_ctx *src, const rt_reproject_params &q, const PlaneInput &in, hipStream_t stream) {
    const auto kernel = in.m ? rt_reproject_moments_kernel<4, true> : in.channels == 4 ? rt_reproject_moments_kernel<4, false> : rt_reproject_moments_kernel<3, false>;
    hipLaunchKernelGGL(kernel, plane_grid(dst->w, dst->h), dim3(kPlaneLanes), 0, stream, reinterpret_cast<float4 *>(dst->planes.temporal), dst->planes.temporal_px,
                       reinterpret_cast<float4 *>(dst->planes.moments), reinterpret_cast<const float4 *>(dst->scene.d_features),
                       reinterpret_cast<const float4 *>(src->scene.d_features), (const float *)dst->d_colors, in.u, in.m, dst->scene.tables.geom,
                       src->scene.tables.geom, dst->scene.tables.n_spheres, pixel_camera(dst->cam), pixel_camera(src->cam), q.k_pos, q.max_history,
                       (float)dst->frame.current_sample, in.passes, dst->w, dst->h, dst->knobs.fast() ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// for rt_atrous_async, the same, from `in` with its moments plane (filter_input of c): (U's rgb, V0 by rule 28) into `out`, the guide and n planes, and --
// `pack`: no level follows -- the packed plane
int atrous_prepare_moments(rt_ctx *c, const PlaneInput &in, float4 *out, bool pack, hipStream_t stream) {
    hipLaunchKernelGGL(rt_atrous_prepare_moments_kernel, plane_grid(c->w, c->h), dim3(kPlaneLanes), 0, stream, out, reinterpret_cast<float4 *>(c->planes.guide),
                       c->planes.n, pack ? c->planes.atrous_px : (uint32_t *)nullptr, in.u, reinterpret_cast<const float4 *>(c->scene.d_features),
                       reinterpret_cast<const float2 *>(in.m), c->planes.moments_set.params.k_min, c->w, c->h, c->knobs.fast() ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // namespace rt

using namespace rt;

extern "C" {

RT_API int rt_set_temporal_moments(rt_ctx *c, const rt_moments_params *m) {
    RT_TRY(tiles_refuse(c, "rt_set_temporal_moments"));
    rt_moments_params q{};
    if (m && rt_host_moments_params(m, &q) != RT_OK) return RT_ERR_ARG;
    c->planes.moments_set = { q, m != nullptr };
    return RT_OK;
}

RT_API int rt_read_moments(rt_ctx *c, float *m_host) { return read_plane(c, "rt_read_moments", Plane::Moments, m_host); }

}  // extern "C"
