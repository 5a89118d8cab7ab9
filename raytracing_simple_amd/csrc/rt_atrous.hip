// rt_atrous.hip -- the edge-avoiding wavelet filter (include/rt_api.h, "edge-avoiding wavelet filter"): the frame the interactive loop shows, filtered --
//   rt_atrous_async          the context's temporal plane (or, where none is current, its colour plane) through `levels` a-trous levels steered by the
//                            feature plane and weighted by sample counts, into a plane (rgb, variance) and its packed plane that the context owns
//   rt_read_atrous           those two planes (read_plane, rt_internal.h)
// and the two kernels behind the first.  rt_atrous_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 20-24, and
// the comments below name the rule a line implements.  The reference filters nothing: this is the library's own extension.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division): every multiply, add and division below is an operation of
// its own, in the written order -- whatever rt_set_mode says.
// The render kernels are not touched, and nothing here writes anything but the context's five filter planes.  The preparation kernel's moments arm
// takes V0 from the moments plane (rule 28) when rt_set_temporal_moments is on and that plane is current; rt_atrous_moments_planes is its host statement.
//
// The shape.  rt_atrous_prepare_kernel evaluates rules 20-21 once: it writes (rgb, V0), a 16-byte guide texel (N, id) and beside it one float that is
// n for a usable pixel and +0.0f for any other -- so a level reads three aligned words per tap (4, 16 and 16 bytes) instead of picking words 3-5 and 7
// out of a 32-byte feature texel and judging usability again.  rt_atrous_level_kernel is one level; the launches alternate between two (rgb, V)
// planes and the last one lands in the context's plane and packs it (rule 24).
// EVERY level gathers its taps from global memory (the vector L1 and L2), also steps 1 and 2, where the tile and its halo would fit LDS: a lane's 25
// taps at step s are 25 of the (32 + 4s) x (8 + 4s) texels a staged tile would hold, neighbouring lanes' taps are neighbouring texels at every step, and
// a level of a 1920x1080 frame reads 75 MB and writes 33 MB in all, less than the last-level cache holds.  The staged form has NOT been measured against this one, at step
// 4 or anywhere else.  What this form measures (the header; profiles/r30_atrous.jsonl): 0.17 ms a level at 1920x1080 at steps 1 to 4 and 0.14 ms at steps 8
// and 16 -- the time does not grow with the taps' spread.  An estimate, not a measurement, of why: a tap is some 90 vector instructions (two IEEE divisions of about
// eleven each, the rest the rules' sums and tests), 25 taps about 2300, 32 400 wavefronts at four cycles an instruction on 1024 SIMDs at 2.4 GHz
// about 0.13 ms.  Most of a level is the rules' own arithmetic, which staging would not shorten.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::fail;

extern "C" int rt_host_atrous_params(const rt_atrous_params *p, rt_atrous_params *out);     // rt_host.cpp: the parameter rules (null = defaults)

// Rules 20-21, one lane per pixel; x and y are ARRAY coordinates (the colour plane's row order).  kCh: U holds 3 floats a pixel (the colour plane, every
// pixel at `n_all` samples) or 4 (the temporal plane).  px is null unless levels == 0 (rule 24 on (U's rgb, V0)).  No LDS, no barrier: a lane outside
// the image leaves at once.
// THE MOMENTS ARM (kMom; rule 28): U is the temporal plane -- M is current only beside it -- and m its moments plane as float2 pairs: texel `at` is
// m[2 * at] = (m1, m2) and m[2 * at + 1] = (k, v), of which the second is read and selects between its v and rule 21's result.  Without the arm m and
// k_min are passed null and zero and not touched.
// Bounds: the lane's own texel of U and F and its four stores at x < w && y < h; a neighbour's texel of U and word 7 of F only for 0 <= qx < w &&
// 0 <= qy < h (the test stands before the loads); the packed word at row h - 1 - y < h; the arm reads m at `at`, the lane's own pixel: ONE 8-byte load.
template <int kCh, bool kMom>
__global__ void __launch_bounds__(kPlaneLanes) rt_atrous_prepare_kernel(float4 *__restrict__ out, float4 *__restrict__ guide, float *__restrict__ n_out, uint32_t *__restrict__ px,
                                                                        const float *__restrict__ u, const float4 *__restrict__ feat, float n_all, int w, int h, int fast,
                                                                        const float2 *__restrict__ m, float k_min) {
    static_assert(!kMom || kCh == 4, "the moments plane is current only beside the temporal plane");
    const auto [x, y] = plane_pixel();
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const float4 up = plane_texel<kCh>(u, at, n_all);
    const float4 f_lo = feat[2 * at], f_hi = feat[2 * at + 1];
    const uint32_t id = __float_as_uint(f_hi.w);
    // rule 21
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const size_t aq = (size_t)qy * (size_t)w + (size_t)qx;
            if (__float_as_uint(feat[2 * aq + 1].w) != id) continue;
            const float4 uq = plane_texel<kCh>(u, aq, n_all);
            if (!rt::usable(uq.x, uq.y, uq.z, uq.w)) continue;
            const float l = rt::luminance(uq.x, uq.y, uq.z);
            s0 = s0 + 1.0f;
            s1 = s1 + l;
            s2 = s2 + l * l;
        }
    float v0 = rt::variance_of_sums(s0, s1, s2);
    const bool usable = rt::usable(up.x, up.y, up.z, up.w);      // rule 20
    if constexpr (kMom) {
        const float2 kv = m[2 * at + 1];                         // (k, v): words 2-3 of M[p]
        v0 = rt::variance_from_history(usable, kv.x, kv.y, k_min, v0);      // rule 28
    }
    out[at] = make_float4(up.x, up.y, up.z, v0);
    guide[at] = make_float4(f_lo.w, f_hi.x, f_hi.y, f_hi.w);
    n_out[at] = usable ? up.w : 0.0f;
    if (px) px[(size_t)(h - 1 - y) * (size_t)w + (size_t)x] = pack_rgb(up.x, up.y, up.z, fast != 0);
}

// Rule 22, one lane per pixel, 25 taps at step s.  `n` is the preparation kernel's plane: n > 0.0f says usable.  The tap rows run as a loop, the five
// taps of a row unrolled: fifteen loads in flight per lane.  A tap's address is clamped into the image and its three words are loaded whatever the
// tests say; whether it COUNTS is a predicate on the sums, so that the loads of a row leave together -- a tap that does not count adds nothing, the
// same words as the host's `continue`.  px is null unless this is the last level (rule 24).  No LDS, no barrier.
// Bounds: the lane's own texels and stores at x < w && y < h; a tap's texels at (cx, cy) = (qx, qy) clamped to [0, w - 1] x [0, h - 1]; qx and qy are
// formed in 32 bits: |s * i| <= 32 and x < w <= 65535 (rt_create's limit); the packed word at row h - 1 - y < h.
__global__ void __launch_bounds__(kPlaneLanes) rt_atrous_level_kernel(float4 *__restrict__ out, uint32_t *__restrict__ px, const float4 *__restrict__ in_cv,
                                                                      const float4 *__restrict__ guide, const float *__restrict__ n, int s, float inv_kn2, float kl2,
                                                                      int w, int h, int fast) {
    const auto [x, y] = plane_pixel();
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const float4 cp = in_cv[at];
    const float np = n[at];
    float4 res = cp;                    // a pixel that is not usable keeps its words
    if (np > 0.0f) {
        const float4 gp = guide[at];
        const uint32_t id = __float_as_uint(gp.w);
        const float lp = rt::luminance(cp.x, cp.y, cp.z);
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, aw = 0.0f, av = 0.0f;
#pragma unroll 1
        for (int j = -2; j <= 2; ++j) {
            const int qy = y + s * j, cy = min(max(qy, 0), h - 1);
            const bool row_in = qy == cy;
            const float hj = rt::atrous_tap(j);
            const size_t row = (size_t)cy * (size_t)w;
#pragma unroll
            for (int i = -2; i <= 2; ++i) {
                const int qx = x + s * i, cx = min(max(qx, 0), w - 1);
                const size_t aq = row + (size_t)cx;
                const float nq = n[aq];
                const float4 gq = guide[aq];
                const float4 cq = in_cv[aq];
                const float hi = rt::atrous_tap(i);
                const bool centre = i == 0 && j == 0;
                const bool counts = centre || (row_in && qx == cx && nq > 0.0f && __float_as_uint(gq.w) == id);
                const float g = rt::atrous_edge(gp.x, gp.y, gp.z, gq.x, gq.y, gq.z, inv_kn2, lp, rt::luminance(cq.x, cq.y, cq.z), cp.w, cq.w, kl2);
                const float wgt = centre ? rt::atrous_centre_weight(np) : rt::atrous_tap_weight(hj, hi, g, nq);
                if (counts) {
                    acc0 = acc0 + wgt * cq.x;
                    acc1 = acc1 + wgt * cq.y;
                    acc2 = acc2 + wgt * cq.z;
                    aw = aw + wgt;
                    av = av + (wgt * wgt) * cq.w;
                }
            }
        }
        res = make_float4(acc0 / aw, acc1 / aw, acc2 / aw, av / (aw * aw));
    }
    out[at] = res;
    if (px) px[(size_t)(h - 1 - y) * (size_t)w + (size_t)x] = pack_rgb(res.x, res.y, res.z, fast != 0);
}

using namespace rt;

extern "C" {

RT_API int rt_atrous_async(rt_ctx *c, const rt_atrous_params *p, void *hip_stream) {
    const char *const call = "rt_atrous_async";
    RT_TRY(tiles_refuse(c, call));
    rt_atrous_params q;
    if (rt_host_atrous_params(p, &q) != RT_OK) return RT_ERR_ARG;
    RT_TRY(features_refuse(c, call));
    RT_TRY(ragged_refuse(c, call, "the context"));
    PlaneInput in;
    RT_TRY(filter_input(c, call, "the context", c->planes.moments_set.on, &in));
    RT_TRY(select_device(c));
    const size_t pixels = image_pixels(c);
    Planes &pl = c->planes;
    RT_TRY(ensure_device(c->owned, &pl.atrous, 4 * pixels));
    RT_TRY(ensure_device(c->owned, &pl.atrous_px, pixels));
    RT_TRY(ensure_device(c->owned, &pl.tmp, 4 * pixels));
    RT_TRY(ensure_device(c->owned, &pl.guide, 4 * pixels));
    RT_TRY(ensure_device(c->owned, &pl.n, pixels));
    hipStream_t stream = (hipStream_t)hip_stream;
    RT_TRY(chain(c, stream));           // behind everything the context has queued, its later work behind the call
    const dim3 grid = plane_grid(c->w, c->h);
    const int fast = c->knobs.fast() ? 1 : 0;
    // the levels alternate between the two planes and end in pl.atrous
    float4 *cur = reinterpret_cast<float4 *>(q.levels % 2 == 0 ? pl.atrous : pl.tmp);
    float4 *nxt = reinterpret_cast<float4 *>(q.levels % 2 == 0 ? pl.tmp : pl.atrous);
    float4 *const guide = reinterpret_cast<float4 *>(pl.guide);
    // rule 28's arm: the setting on AND M current (which implies the temporal plane); nothing else decides
    const auto prepare = in.m ? rt_atrous_prepare_kernel<4, true> : in.channels == 4 ? rt_atrous_prepare_kernel<4, false> : rt_atrous_prepare_kernel<3, false>;
    hipLaunchKernelGGL(prepare, grid, dim3(kPlaneLanes), 0, stream, cur, guide, pl.n, q.levels == 0 ? pl.atrous_px : (uint32_t *)nullptr, in.u,
                       reinterpret_cast<const float4 *>(c->scene.d_features), in.passes, c->w, c->h, fast, reinterpret_cast<const float2 *>(in.m),
                       in.m ? pl.moments_set.params.k_min : 0.0f);
    HIP_TRY(hipGetLastError());
    const float inv_kn2 = 1.0f / (q.k_normal * q.k_normal), kl2 = q.k_lum * q.k_lum;
    for (int level = 0; level < q.levels; ++level) {
        hipLaunchKernelGGL(rt_atrous_level_kernel, grid, dim3(kPlaneLanes), 0, stream, nxt, level == q.levels - 1 ? pl.atrous_px : (uint32_t *)nullptr, cur, guide,
                           (const float *)pl.n, 1 << level, inv_kn2, kl2, c->w, c->h, fast);
        HIP_TRY(hipGetLastError());
        float4 *t = cur;
        cur = nxt;
        nxt = t;
    }
    c->frame.atrous_filtered();
    return RT_OK;
}

RT_API int rt_read_atrous(rt_ctx *c, float *rgbv_host, uint32_t *packed_host) { return read_plane(c, "rt_read_atrous", Plane::Atrous, rgbv_host, packed_host); }

}  // extern "C"
