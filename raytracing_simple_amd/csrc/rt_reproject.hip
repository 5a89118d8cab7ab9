// rt_reproject.hip -- temporal reprojection (include/rt_api.h, "temporal reprojection"): a frame's samples carried to a moved camera --
//   rt_reproject_async       src's history warped into dst's view through the first-hit geometry of the two feature planes and blended with dst's
//                            colour plane, into a temporal plane (rgb, n) and its packed plane that dst owns
//   rt_read_temporal         those two planes (read_plane, rt_internal.h)
// with the two per-context settings that rt_reproject_async INTO a context consults, and their planes --
//   rt_set_temporal_moments  temporal luminance moments (rules 25-27): dst's moments plane M is formed beside T (rt_atrous_async consults the setting too)
//   rt_read_moments          that plane, (m1, m2, k, v) per pixel
//   rt_set_shadow_history    shadow-aware history (rules 29-32): a pixel's history ends where a moved sphere's shadow comes or goes
//   rt_read_history_flags    the context's flag plane K, one byte per pixel
// and the ONE kernel behind them, rt_reproject_kernel<kCh, kMom, kShadow>: the two settings are arms of it, chosen at compile time, and one function
// below names the instance a state launches.  rt_reproject_planes, rt_reproject_moments_planes and rt_reproject_shadow_planes (rt_host.cpp) are the
// same arithmetic as plain loops; the header states it as rules 15-19, 25-27 and 29-32, the rules' arithmetic itself is rt_rules.h, the pair list is built
// by ONE function for both sides, and the comments below name the rule a line implements.  The reference reprojects nothing: this is the library's own
// extension.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division and square root): every multiply, add, division and square
// root below is an operation of its own, in the written order -- whatever rt_set_mode says.
// The render kernels are not touched, and nothing here writes anything but dst's two temporal planes and, under the settings, its moments plane, its
// flag plane and its pair list.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::dot3;
using rt::fail;

extern "C" int rt_host_reproject_params(const rt_reproject_params *p, rt_reproject_params *out);     // rt_host.cpp: the parameter rules (null = defaults)
extern "C" int rt_host_moments_params(const rt_moments_params *p, rt_moments_params *out);
extern "C" int rt_host_shadow_history_params(const rt_shadow_history_params *p, rt_shadow_history_params *out);
extern "C" size_t rt_host_shadow_pairs(const rt_sphere *S, const rt_sphere *D, uint32_t count, float *out, size_t cap);   // rt_host.cpp: rule 29's list

static_assert(rt::kShadowPairFloats == 20, "a pair is five float4 texels in LDS and on the device");

// One lane per pixel of D.  kCh: the source plane U holds 3 floats a pixel (S's colour plane, every pixel at `ns` samples) or 4 (S's temporal plane).
// Both cameras, the parameters and nd are kernel arguments and stay in scalar registers.  FD and each tap's words of FS are read as two float4, a
// temporal texel as one; the taps are gathers, but neighbouring lanes land on neighbouring pixels of S.  Never any scratch.  An argument that an
// instance's arms do not read is passed null or zero and not touched.
// THE MOMENTS ARM (kMom, rt_plane.inc.h; rules 25-27): kNoMoments discards it; kMomentsOfLuminance takes a tap's moments from the luminance of U
// (rule 25's fallback); kMomentsOfPlane from S's moments plane m_s, current only beside S's temporal plane (so kCh == 4) -- one more float4 load per
// tap that COUNTS, beside U's.  Both store the lane's texel of dst's moments plane out_m as ONE float4.
// THE SHADOW ARM (kShadow; rules 29-32): `pairs` holds n_pairs records of five float4 (rt_rules.h kShadowPairFloats); they go through s_pairs,
// kShadowChunk records (5120 bytes of LDS) at a time, a barrier either side of a chunk, and are read back at wave-uniform addresses.  out_k is dst's
// flag plane, one byte at the lane's own pixel: with no pair, a plane of zeros.
// Barriers: without kShadow, no LDS and no barrier: a lane outside the image leaves at once.  Under kShadow NO LANE LEAVES before the last barrier: a
// lane outside the image takes the nearest pixel inside it -- every load below is then in bounds as stated -- computes what that pixel's lane
// computes and stores nothing, so that EVERY lane of the workgroup -- outside the image, over the sky, without history -- reaches both barriers of
// every chunk.  Only the pair arithmetic and the stores are predicated.
// Bounds: FD, CD and the stores (out, out_px, out_m, out_k) at the lane's own pixel, x < w && y < h; the centres at id < n, the size of both tables
// (the host refuses scenes that differ in it); a tap's words of FS, U and m_s only at `aq`, a position that passed 0 <= qx < w && 0 <= qy < h (and, for
// m_s, every later test); a chunk stages texels [5 * base, 5 * min(base + kShadowChunk, n_pairs)) of a list of 5 * n_pairs and tests exactly those records.
template <int kCh, int kMom, bool kShadow>
__global__ void __launch_bounds__(kPlaneLanes) rt_reproject_kernel(float4 *__restrict__ out, uint32_t *__restrict__ out_px, float4 *__restrict__ out_m,
                                                                   uint8_t *__restrict__ out_k, const float4 *__restrict__ feat_d,
                                                                   const float4 *__restrict__ feat_s, const float *__restrict__ col_d,
                                                                   const float *__restrict__ u_s, const float4 *__restrict__ m_s,
                                                                   const float4 *__restrict__ geom_d, const float4 *__restrict__ geom_s,
                                                                   const float4 *__restrict__ pairs, uint32_t n_pairs, uint32_t n, rt::PixelCamera cam_d,
                                                                   rt::PixelCamera cam_s, float k_pos, float max_history, float nd, float ns, int w, int h,
                                                                   int fast, float keep) {
    static_assert(kMom != kMomentsOfPlane || kCh == 4, "S's moments plane is current only beside its temporal plane");
    const auto [lane_x, lane_y] = plane_pixel();
    if constexpr (!kShadow) {
        if (lane_x >= w || lane_y >= h) return;
    }
    [[maybe_unused]] const bool inside = lane_x < w && lane_y < h;
    const int x = kShadow ? min(lane_x, w - 1) : lane_x, y = kShadow ? min(lane_y, h - 1) : lane_y;
    const size_t at = (size_t)(h - 1 - y) * (size_t)w + (size_t)x;
    const float inv_w = 1.f / (float)w, inv_h = 1.f / (float)h, fw = (float)w, fh = (float)h;

    float sw = 0.0f, sn = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f;
    [[maybe_unused]] float s1 = 0.0f, s2 = 0.0f, sk = 0.0f;           // rule 26
    [[maybe_unused]] float px = 0.0f, py = 0.0f, pz = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;       // rule 31: P and Pp, kept for the pairs
    // rule 15: the point and where it was
    const float4 fd_hi = feat_d[2 * at + 1];                 // (words 4-7; words 0-3 of FD are not needed)
    const uint32_t id = __float_as_uint(fd_hi.w);
    if (id < n) {
        const float t = fd_hi.z;
        const rt::PixelRay r = rt::pixel_ray(cam_d, x, y, inv_w, inv_h);       // rule 10
        const float4 gd = geom_d[id], gs = geom_s[id];
        const float ppx = (r.ox + r.dx * t) - (gd.x - gs.x), ppy = (r.oy + r.dy * t) - (gd.y - gs.y), ppz = (r.oz + r.dz * t) - (gd.z - gs.z);
        // rule 16: where S saw it
        if constexpr (kShadow) px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t, wx = ppx, wy = ppy, wz = ppz;
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
                        if constexpr (kMom != kNoMoments) {
                            // rule 25: the tap's moments; rule 26: their sums
                            float m1q, m2q, kq;
                            if constexpr (kMom == kMomentsOfPlane) {
                                const float4 mq = m_s[aq];
                                m1q = mq.x, m2q = mq.y, kq = mq.z;
                            } else {
                                const float lq = rt::luminance(u.x, u.y, u.z);
                                m1q = lq, m2q = lq * lq, kq = 1.0f;
                            }
                            s1 = s1 + b * m1q;
                            s2 = s2 + b * m2q;
                            sk = sk + b * kq;
                        }
                    }
            }
        }
    }
    const bool have_d = nd != 0.0f;
    [[maybe_unused]] bool flagged = false;
    if constexpr (kShadow) {
        // rule 31: the pairs, a chunk at a time
        __shared__ float4 s_pairs[5 * kShadowChunk];
        const bool candidate = inside && sw > 0.0f && have_d;         // (history implies a record under the pixel)
        for (uint32_t base = 0; base < n_pairs; base += kShadowChunk) {
            const uint32_t m = min((uint32_t)kShadowChunk, n_pairs - base);
            for (uint32_t i = threadIdx.x; i < 5 * m; i += (uint32_t)kPlaneLanes) s_pairs[i] = pairs[5 * (size_t)base + i];
            __syncthreads();
            if (candidate && !flagged)                                // (a flagged lane skips the arithmetic, never a barrier)
                for (uint32_t i = 0; i < m; ++i) {
                    const float4 lj = s_pairs[5 * i + 4];
                    if (__float_as_uint(lj.x) == id || __float_as_uint(lj.y) == id) continue;
                    const float4 ls = s_pairs[5 * i], ld = s_pairs[5 * i + 1], js = s_pairs[5 * i + 2], jd = s_pairs[5 * i + 3];
                    const int before = rt::shadow_state(wx, wy, wz, ls.x, ls.y, ls.z, ls.w, js.x, js.y, js.z, js.w);      // rule 30
                    const int after = rt::shadow_state(px, py, pz, ld.x, ld.y, ld.z, ld.w, jd.x, jd.y, jd.z, jd.w);
                    flagged = flagged || rt::shadow_changes(before, after);
                }
            __syncthreads();
        }
        if (!inside) return;                                          // (behind the last barrier)
        out_k[at] = flagged ? 1 : 0;
    }
    // rule 19: the blend (D's colour plane is not read at pass 0), with rule 32's cap under kShadow
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (have_d) c0 = col_d[3 * at], c1 = col_d[3 * at + 1], c2 = col_d[3 * at + 2];
    float t0, t1, t2, tn;
    if constexpr (kShadow) rt::temporal_blend_as<true>(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history, flagged, keep);
    else rt::temporal_blend(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history);
    out[at] = make_float4(t0, t1, t2, tn);
    out_px[(size_t)y * (size_t)w + (size_t)x] = pack_rgb(t0, t1, t2, fast != 0);
    if constexpr (kMom != kNoMoments) {
        // rule 27: the moments' blend
        float m1, m2, k, v;
        if constexpr (kShadow)
            rt::moments_blend_as<true>(m1, m2, k, v, have_d ? rt::luminance(c0, c1, c2) : 0.0f, nd, have_d, sw, sn, s1, s2, sk, max_history, flagged, keep);
        else rt::moments_blend(m1, m2, k, v, have_d ? rt::luminance(c0, c1, c2) : 0.0f, nd, have_d, sw, sn, s1, s2, sk, max_history);
        out_m[at] = make_float4(m1, m2, k, v);
    }
}

using namespace rt;

namespace {

using ReprojectKernel = decltype(&rt_reproject_kernel<4, kNoMoments, false>);

// The instance a state launches, and every instance there is.  channels: 3 or 4 floats a texel of U; moments: dst's setting; from_plane: S's moments
// plane is current (which implies its temporal plane, channels == 4); shadow: dst's setting, whatever the pair list holds
ReprojectKernel reproject_instance(int channels, bool moments, bool from_plane, bool shadow) {
    const bool wide = channels == 4;
    if (!moments)
        return shadow ? (wide ? rt_reproject_kernel<4, kNoMoments, true> : rt_reproject_kernel<3, kNoMoments, true>)
                      : (wide ? rt_reproject_kernel<4, kNoMoments, false> : rt_reproject_kernel<3, kNoMoments, false>);
    if (from_plane) return shadow ? rt_reproject_kernel<4, kMomentsOfPlane, true> : rt_reproject_kernel<4, kMomentsOfPlane, false>;
    return shadow ? (wide ? rt_reproject_kernel<4, kMomentsOfLuminance, true> : rt_reproject_kernel<3, kMomentsOfLuminance, true>)
                  : (wide ? rt_reproject_kernel<4, kMomentsOfLuminance, false> : rt_reproject_kernel<3, kMomentsOfLuminance, false>);
}

// rule 29 for rt_reproject_async: the pair list of (src's records, dst's records) from the two mirrors, through dst's staging ring into dst's block on
// `stream`, without a host wait.  A list that outgrows the block replaces it (the runtime waits for the device before a block goes)
int stage_pairs(rt_ctx *dst, const rt_ctx *src, hipStream_t stream, uint32_t *n_pairs) {
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

}  // namespace

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
    const bool shadow = dst->planes.shadow_set.on;         // ... and K beside T (rules 29-32)
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
    uint32_t n_pairs = 0;
    if (shadow) {
        RT_TRY(ensure_device(dst->owned, &pl.flags, image_pixels(dst)));
        RT_TRY(stage_pairs(dst, src, stream, &n_pairs));
    }
    hipLaunchKernelGGL(reproject_instance(in.channels, moments, in.m != nullptr, shadow), plane_grid(dst->w, dst->h), dim3(kPlaneLanes), 0, stream,
                       reinterpret_cast<float4 *>(pl.temporal), pl.temporal_px, moments ? reinterpret_cast<float4 *>(pl.moments) : (float4 *)nullptr,
                       shadow ? pl.flags : (uint8_t *)nullptr, reinterpret_cast<const float4 *>(dst->scene.d_features),
                       reinterpret_cast<const float4 *>(src->scene.d_features), (const float *)dst->d_colors, in.u, in.m, dst->scene.tables.geom,
                       src->scene.tables.geom, shadow ? (const float4 *)pl.pairs : (const float4 *)nullptr, n_pairs, dst->scene.tables.n_spheres,
                       pixel_camera(dst->cam), pixel_camera(src->cam), q.k_pos, q.max_history, (float)dst->frame.current_sample, in.passes, dst->w, dst->h,
                       dst->knobs.fast() ? 1 : 0, shadow ? pl.shadow_set.params.keep : 0.0f);
    HIP_TRY(hipGetLastError());
    dst->frame.reprojected(moments);
    pl.flags_formed = shadow;
    return RT_OK;
}

RT_API int rt_read_temporal(rt_ctx *c, float *rgbn_host, uint32_t *packed_host) { return read_plane(c, "rt_read_temporal", Plane::Temporal, rgbn_host, packed_host); }

RT_API int rt_set_temporal_moments(rt_ctx *c, const rt_moments_params *m) {
    RT_TRY(tiles_refuse(c, "rt_set_temporal_moments"));
    rt_moments_params q{};
    if (m && rt_host_moments_params(m, &q) != RT_OK) return RT_ERR_ARG;
    c->planes.moments_set = { q, m != nullptr };
    return RT_OK;
}

RT_API int rt_read_moments(rt_ctx *c, float *m_host) { return read_plane(c, "rt_read_moments", Plane::Moments, m_host); }

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
