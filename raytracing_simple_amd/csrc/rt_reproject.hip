// rt_reproject.hip -- temporal reprojection (include/rt_api.h, "temporal reprojection"): a frame's samples carried to a moved camera --
//   rt_reproject_async       src's history warped into dst's view through the first-hit geometry of the two feature planes and blended with dst's
//                            colour plane, into a temporal plane (rgb, n) and its packed plane that dst owns
//   rt_read_temporal         those two planes
// and the kernel behind the first.  rt_reproject_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 15-19, and
// the comments below name the rule a line implements.  The reference reprojects nothing: this is the library's own extension.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division and square root): every multiply, add, division and square
// root below is an operation of its own, in the written order -- whatever rt_set_mode says.
// The render kernels are not touched, and nothing here writes anything but the two temporal planes.
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
    const auto [x, y] = plane_pixel();
    if (x >= w || y >= h) return;
    const size_t at = (size_t)(h - 1 - y) * (size_t)w + (size_t)x;
    const float inv_w = 1.f / (float)w, inv_h = 1.f / (float)h, fw = (float)w, fh = (float)h;

    float sw = 0.0f, sn = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f;
    // rule 15: the point and where it was
    const float4 fd_hi = feat_d[2 * at + 1];                 // (words 4-7; words 0-3 of FD are not needed)
    const uint32_t id = __float_as_uint(fd_hi.w);
    if (id < n) {
        const float t = fd_hi.z;
        const rt::PixelRay r = rt::pixel_ray(cam_d, x, y, inv_w, inv_h);       // rule 10
        const float4 gd = geom_d[id], gs = geom_s[id];
        const float ppx = (r.ox + r.dx * t) - (gd.x - gs.x), ppy = (r.oy + r.dy * t) - (gd.y - gs.y), ppz = (r.oz + r.dz * t) - (gd.z - gs.z);
        // rule 16: where S saw it
        const float vx = ppx - cam_s.ox, vy = ppy - cam_s.oy, vz = ppz - cam_s.oz;
        const float z = dot3(vx, vy, vz, cam_s.dx, cam_s.dy, cam_s.dz);
        if (z > 0.0f) {
            const float dd = dot3(cam_s.dx, cam_s.dy, cam_s.dz, cam_s.dx, cam_s.dy, cam_s.dz);
            const float xx = dot3(cam_s.xx, cam_s.xy, cam_s.xz, cam_s.xx, cam_s.xy, cam_s.xz);
            const float yy = dot3(cam_s.yx, cam_s.yy, cam_s.yz, cam_s.yx, cam_s.yy, cam_s.yz);
            const float kx = (dot3(vx, vy, vz, cam_s.xx, cam_s.xy, cam_s.xz) * dd) / (z * xx);
            const float ky = (dot3(vx, vy, vz, cam_s.yx, cam_s.yy, cam_s.yz) * dd) / (z * yy);
            const float fx = (kx + 0.5f) * fw, fy = (ky + 0.5f) * fh;
            if (fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                const float x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0;
                const float foot = sqrtf(xx) * (1.f / (float)w);
                // rule 17: the taps
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = (int)x0 + i, qy = (int)y0 + j;
                        const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const size_t aq = (size_t)(h - 1 - qy) * (size_t)w + (size_t)qx;
                        const float4 fs_hi = feat_s[2 * aq + 1];
                        if (__float_as_uint(fs_hi.w) != id) continue;
                        const float tq = fs_hi.z;
                        const rt::PixelRay rq = rt::pixel_ray(cam_s, qx, qy, inv_w, inv_h);
                        const float ex = (rq.ox + rq.dx * tq) - ppx, ey = (rq.oy + rq.dy * tq) - ppy, ez = (rq.oz + rq.dz * tq) - ppz;
                        const float rr = k_pos * (tq * foot);
                        if (!(dot3(ex, ey, ez, ex, ey, ez) <= rr * rr)) continue;
                        const float4 u = plane_texel<kCh>(u_s, aq, ns);
                        if (!rt::usable(u.x, u.y, u.z, u.w)) continue;
                        // rule 18: the history
                        sw = sw + b;
                        sn = sn + b * u.w;
                        sc0 = sc0 + b * u.x;
                        sc1 = sc1 + b * u.y;
                        sc2 = sc2 + b * u.z;
                    }
            }
        }
    }
    // rule 19: the blend (D's colour plane is not read at pass 0)
    const bool have_d = nd != 0.0f;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (have_d) c0 = col_d[3 * at], c1 = col_d[3 * at + 1], c2 = col_d[3 * at + 2];
    float t0, t1, t2, tn;
    rt::temporal_blend(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history);
    out[at] = make_float4(t0, t1, t2, tn);
    out_px[(size_t)y * (size_t)w + (size_t)x] = pack_rgb(t0, t1, t2, fast != 0);
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
        const char *who = c == dst ? "the destination" : "the source";
        RT_TRY(features_refuse(c, call, "", c == dst ? " of the destination" : " of the source"));
        if (c->frame.ragged) return fail(RT_ERR_STATE, "%s: %s is ragged (its tiles hold different pass counts)", call, who);
    }
    if (dst->scene.tables.n_spheres != src->scene.tables.n_spheres)
        return fail(RT_ERR_STATE, "%s: the destination's scene holds %u records, the source's %u", call, dst->scene.tables.n_spheres, src->scene.tables.n_spheres);
    const bool from_temporal = temporal_current(src);
    if (!from_temporal && src->frame.current_sample <= 0)
        return fail(RT_ERR_STATE, "%s: the source holds neither a current temporal plane nor a pass", call);
    rc = select_device(dst);
    if (rc != RT_OK) return rc;
    RT_TRY(ensure_device(dst->owned, &dst->d_temporal, 4 * image_pixels(dst)));
    RT_TRY(ensure_device(dst->owned, &dst->d_temporal_px, image_pixels(dst)));
    // behind everything the two contexts have queued, their later work behind the call; the tables from the records as they are now
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(dst, stream);
    if (rc == RT_OK) rc = chain(src, stream);
    if (rc == RT_OK) rc = refresh_tables(dst, stream);
    if (rc == RT_OK) rc = refresh_tables(src, stream);
    if (rc != RT_OK) return rc;
    const auto kernel = from_temporal ? rt_reproject_kernel<4> : rt_reproject_kernel<3>;
    hipLaunchKernelGGL(kernel, plane_grid(dst->w, dst->h), dim3(kPlaneLanes), 0, stream, reinterpret_cast<float4 *>(dst->d_temporal), dst->d_temporal_px,
                       reinterpret_cast<const float4 *>(dst->scene.d_features), reinterpret_cast<const float4 *>(src->scene.d_features),
                       (const float *)dst->d_colors, (const float *)(from_temporal ? src->d_temporal : src->d_colors), dst->scene.tables.geom, src->scene.tables.geom,
                       dst->scene.tables.n_spheres, pixel_camera(dst->cam), pixel_camera(src->cam), q.k_pos, q.max_history, (float)dst->frame.current_sample,
                       (float)src->frame.current_sample, dst->w, dst->h, dst->knobs.fast() ? 1 : 0);
    HIP_TRY(hipGetLastError());
    dst->frame.reprojected();
    return RT_OK;
}

RT_API int rt_read_temporal(rt_ctx *c, float *rgbn_host, uint32_t *packed_host) {
    return read_plane4(c, "rt_read_temporal", rgbn_host, packed_host, temporal_current, &rt_ctx::d_temporal, &rt_ctx::d_temporal_px,
                       "temporal plane (rt_reproject_async forms one; whatever moves the colour plane or ends the feature plane ends it)");
}

}  // extern "C"
