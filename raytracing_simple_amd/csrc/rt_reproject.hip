// rt_reproject.hip -- temporal reprojection (include/rt_api.h, "temporal reprojection"): a frame's samples carried to a moved camera --
//   rt_reproject_async       src's history warped into dst's view through the first-hit geometry of the two feature planes and blended with dst's
//                            colour plane, into a temporal plane (rgb, n) and its packed plane that dst owns
//   rt_read_temporal         those two planes (read_plane, rt_internal.h)
// and the kernel behind the first.  rt_reproject_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 15-19, and
// the comments below name the rule a line implements.  The reference reprojects nothing: this is the library's own extension.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division and square root): every multiply, add, division and square
// root below is an operation of its own, in the written order -- whatever rt_set_mode says.
// The render kernels are not touched, and nothing here writes anything but the two temporal planes -- and, with rt_set_temporal_moments on for dst,
// its moments plane, through the kernel instances of rt_moments.hip, and, with rt_set_shadow_history on for dst, its flag plane, through those of
// rt_shadow_history.hip.  The kernel's STATEMENTS are rt_reproject_body.inc.h, shared with those units.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::dot3;
using rt::fail;

extern "C" int rt_host_reproject_params(const rt_reproject_params *p, rt_reproject_params *out);     // rt_host.cpp: the parameter rules (null = defaults)

// One lane per pixel of D.  kCh: the source plane U holds 3 floats a pixel (S's colour plane, every pixel at `ns` samples) or 4 (S's temporal plane).
// Both cameras, the parameters and nd are kernel arguments and stay in scalar registers.  FD and each tap's words of FS are read as two float4, a
// temporal texel as one; the taps are gathers, but neighbouring lanes land on neighbouring pixels of S.  No LDS, no barrier: a lane outside the image
// leaves at once.
// Bounds: FD, CD and the two stores at the lane's own pixel, x < w && y < h; the centres at id < n, the size of both tables (the host refuses scenes
// that differ in it); a tap's words of FS and U only for 0 <= qx < w && 0 <= qy < h.
template <int kCh>
__global__ void __launch_bounds__(kPlaneLanes) rt_reproject_kernel(float4 *__restrict__ out, uint32_t *__restrict__ out_px, const float4 *__restrict__ feat_d,
                                                                   const float4 *__restrict__ feat_s, const float *__restrict__ col_d, const float *__restrict__ u_s,
                                                                   const float4 *__restrict__ geom_d, const float4 *__restrict__ geom_s, uint32_t n, rt::PixelCamera cam_d,
                                                                   rt::PixelCamera cam_s, float k_pos, float max_history, float nd, float ns, int w, int h, int fast) {
    constexpr int kMom = kNoMoments;                        // the moments arm (rt_moments.hip) is discarded: its two planes are not arguments here
    constexpr float4 *out_m = nullptr;
    constexpr const float4 *m_s = nullptr;
    constexpr bool kShadow = false;                         // ... and so is the shadow arm (rt_shadow_history.hip), with its list, its setting, its plane and its LDS
    constexpr const float4 *pairs = nullptr;
    constexpr uint32_t n_pairs = 0;
    constexpr float keep = 0.0f;
    constexpr uint8_t *out_k = nullptr;
    constexpr float4 *s_pairs = nullptr;
#include "rt_reproject_body.inc.h"
}

using namespace rt;

extern "C" {

RT_API int rt_reproject_async(rt_ctx *dst, rt_ctx *src, const rt_reproject_params *p, void *hip_stream) {
    const char *const call = "rt_reproject_async";
    if (!dst || !src) return fail(RT_ERR_ARG, "%s: ctx is null", call);
    int rc = tiles_refuse(dst, call);
    if (rc == RT_OK) rc = tiles_refuse(src, call);
    // (no context is sharded by now: rows per tile say nothing about an unsharded frame)
    if (rc == RT_OK) rc = same_frame(dst, src, call, "the destination", "the source", false);
    if (rc != RT_OK) return rc;
    rt_reproject_params q;
    if (rt_host_reproject_params(p, &q) != RT_OK) return RT_ERR_ARG;
    for (const rt_ctx *c : { dst, src }) {
        RT_TRY(features_refuse(c, call, "", c == dst ? " of the destination" : " of the source"));
        RT_TRY(ragged_refuse(c, call, c == dst ? "the destination" : "the source"));
    }
    if (dst->scene.tables.n_spheres != src->scene.tables.n_spheres)
        return fail(RT_ERR_STATE, "%s: the destination's scene holds %u records, the source's %u", call, dst->scene.tables.n_spheres, src->scene.tables.n_spheres);
    const bool moments = dst->planes.moments_set.on;       // the setting of dst: M is formed beside T (rules 25-27), from S's M while that is current, else from U's luminance
    const bool shadow = dst->planes.shadow_set.on;         // ... and K beside T (rules 29-32), through the kernels of rt_shadow_history.hip
    PlaneInput in;
    RT_TRY(filter_input(src, call, "the source", moments, &in));
    RT_TRY(select_device(dst));
    Planes &pl = dst->planes;
    RT_TRY(ensure_device(dst->owned, &pl.temporal, 4 * image_pixels(dst)));
    RT_TRY(ensure_device(dst->owned, &pl.temporal_px, image_pixels(dst)));
    if (moments) RT_TRY(ensure_device(dst->owned, &pl.moments, 4 * image_pixels(dst)));
    // behind everything the two contexts have queued, their later work behind the call; the tables from the records as they are now
    hipStream_t stream = (hipStream_t)hip_stream;
    RT_TRY(chain_all(stream, { dst, src }));
    RT_TRY(refresh_tables(dst, stream));
    RT_TRY(refresh_tables(src, stream));
    if (shadow) RT_TRY(reproject_shadow(dst, src, q, in, moments, stream));   // rt_shadow_history.hip: the kernels with the shadow arm, or -- no pair -- one below
    else if (moments) RT_TRY(reproject_moments(dst, src, q, in, stream));     // rt_moments.hip: the kernel with the moments arm
    else {
        const auto kernel = in.channels == 4 ? rt_reproject_kernel<4> : rt_reproject_kernel<3>;
        hipLaunchKernelGGL(kernel, plane_grid(dst->w, dst->h), dim3(kPlaneLanes), 0, stream, reinterpret_cast<float4 *>(pl.temporal), pl.temporal_px,
                           reinterpret_cast<const float4 *>(dst->scene.d_features), reinterpret_cast<const float4 *>(src->scene.d_features),
                           (const float *)dst->d_colors, in.u, dst->scene.tables.geom, src->scene.tables.geom, dst->scene.tables.n_spheres, pixel_camera(dst->cam),
                           pixel_camera(src->cam), q.k_pos, q.max_history, (float)dst->frame.current_sample, in.passes, dst->w, dst->h, dst->knobs.fast() ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    dst->frame.reprojected(moments);
    pl.flags_formed = shadow;
    return RT_OK;
}

RT_API int rt_read_temporal(rt_ctx *c, float *rgbn_host, uint32_t *packed_host) { return read_plane(c, "rt_read_temporal", Plane::Temporal, rgbn_host, packed_host); }

}  // extern "C"
