// rt_rules.h -- the arithmetic of the numbered rules of include/rt_api.h's extensions (feature planes, NL-means and its guide, temporal reprojection,
// the a-trous filter, temporal luminance moments, shadow-aware history), stated ONCE: the plain loops of rt_host.cpp (rt_*_planes) and the kernels (rt_features.hip,
// rt_reproject.hip, rt_atrous.hip, rt_denoise.inc.h) call these functions, so the two sides the GPU tests hold together bit for bit cannot drift apart by a copied line.  Usable from plain
// C++ and from HIP, like rt_bvh_layout.h, whose RT_HD it takes.  Every unit that includes it is compiled with -ffp-contract=off: every multiply, add,
// division and square root below is an operation of its own, in the written order and parenthesisation -- which is part of the rule.
// What is NOT here: loops, staging, clamping, and whether a tap that does not count is skipped or predicated.  Those belong to each side.
// A new filter adds its rules here and calls them from both sides.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/rt_api.h"
#include "rt_bvh_layout.h"      // RT_HD

#ifdef __HIPCC__
#define RT_RULE RT_HD inline __attribute__((always_inline))     /* HIP's __forceinline__, spelt out: this header includes no HIP header */
#else
#define RT_RULE RT_HD inline
#endif

namespace rt {

struct PixelCamera {            // what rule 10 reads of an rt_camera: origin, direction, and the two image axes
    float ox, oy, oz, dx, dy, dz, xx, xy, xz, yx, yy, yz;
};

RT_RULE PixelCamera pixel_camera(const rt_camera &m) {
    return PixelCamera{ m.orig.x, m.orig.y, m.orig.z, m.dir.x, m.dir.y, m.dir.z, m.x.x, m.x.y, m.x.z, m.y.x, m.y.y, m.y.z };
}

struct PixelRay {               // origin and unit direction
    float ox, oy, oz, dx, dy, dz;
};

struct Float3 {
    float x, y, z;
};

RT_RULE float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// rule 10: the ray through the centre of image pixel (x, y) (.cl:494-549 with both random numbers 0.5); inv_w = 1.f / (float)w, inv_h alike
RT_RULE PixelRay pixel_ray(const PixelCamera &cam, int x, int y, float inv_w, float inv_h) {
    const float kcx = ((float)x + 0.0f) * inv_w - 0.5f, kcy = ((float)y + 0.0f) * inv_h - 0.5f;
    const float rx = cam.xx * kcx + cam.yx * kcy + cam.dx;
    const float ry = cam.xy * kcx + cam.yy * kcy + cam.dy;
    const float rz = cam.xz * kcx + cam.yz * kcy + cam.dz;
    const float f = 1.f / sqrtf(rx * rx + ry * ry + rz * rz);
    return PixelRay{ 0.1f * rx + cam.ox, 0.1f * ry + cam.oy, 0.1f * rz + cam.oz, rx * f, ry * f, rz * f };
}

// rule 11: the distance at which the ray meets the sphere {centre, radius^2}, 0 for a miss (.cl:173-201)
RT_RULE float sphere_distance(float cx, float cy, float cz, float rad2, const PixelRay &r) {
    const float px = cx - r.ox, py = cy - r.oy, pz = cz - r.oz;
    const float b = px * r.dx + py * r.dy + pz * r.dz;
    float det = b * b - (px * px + py * py + pz * pz) + rad2;
    float dist = 0.f;
    if (!(det < 0.f)) {
        det = sqrtf(det);
        const float t1 = b - det, t2 = b + det;
        dist = t1 > 0.01f ? t1 : (t2 > 0.01f ? t2 : 0.f);
    }
    return dist;
}

// rule 12: the unit normal at distance t along the ray, from the centre of the sphere it hit (.cl:338-347; not turned towards the ray)
RT_RULE Float3 hit_normal(const PixelRay &r, float t, float cx, float cy, float cz) {
    const float nx = (r.ox + r.dx * t) - cx, ny = (r.oy + r.dy * t) - cy, nz = (r.oz + r.dz * t) - cz;
    const float nf = 1.f / sqrtf(nx * nx + ny * ny + nz * nz);
    return Float3{ nx * nf, ny * nf, nz * nf };
}

// the falloff of rules 5, 13 and 22: the weight of a distance g >= 0
RT_RULE float falloff(float g) { return 1.0f / (1.0f + g * (1.0f + g * 0.5f)); }

// rule 3: one channel's term of e(x, o), from the difference t of the two values, and -- the same for every guide -- the offset and the denominator
// of the variances vp (the position's) and vq (its partner's)
RT_RULE float nlm_offset(float alpha, float vp, float vq) {
    const float m = vq < vp ? vq : vp;
    return alpha * (vp + m);
}
RT_RULE float nlm_denominator(float kk, float vp, float vq) { return 1e-10f + kk * (vp + vq); }
RT_RULE float nlm_term(float t, float off, float dnm) { return (t * t - off) / dnm; }

// rule 13: the feature weight of two pixels from words 0-6 of their records of the feature plane (albedo, normal, distance); ia, in, id = 1 / k^2
RT_RULE float guide_weight(const float *fp, const float *fq, float ia, float in, float id) {
    const float a0 = fp[0] - fq[0], a1 = fp[1] - fq[1], a2 = fp[2] - fq[2];
    const float n0 = fp[3] - fq[3], n1 = fp[4] - fq[4], n2 = fp[5] - fq[5];
    const float pa = ((a0 * a0 + a1 * a1) + a2 * a2) * ia;
    const float pn = ((n0 * n0 + n1 * n1) + n2 * n2) * in;
    const float r = (fp[6] - fq[6]) / ((fp[6] + fq[6]) + 1e-10f);
    const float pd = (r * r) * id;
    float phi = 0.0f;
    if (pa > phi) phi = pa;                                  // (a NaN term constrains nothing)
    if (pn > phi) phi = pn;
    if (pd > phi) phi = pd;
    return falloff(phi);
}

// rules 5, 17 and 20: three finite values ...
RT_RULE bool finite3(float a, float b, float c) { return fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX && fabsf(c) <= FLT_MAX; }
// rules 17 and 20: ... that stand for n > 0 samples
RT_RULE bool usable(float r, float g, float b, float n) { return finite3(r, g, b) && n > 0.0f; }

// rule 20: luminance
RT_RULE float luminance(float c0, float c1, float c2) { return (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2; }

// rule 21: the variance of s0 luminances whose sum is s1 and whose squares sum to s2; 0 for none, never negative
RT_RULE float variance_of_sums(float s0, float s1, float s2) {
    float v0 = 0.0f;
    if (s0 > 0.0f) {
        const float m = s1 / s0, v = s2 / s0 - m * m;
        v0 = v > 0.0f ? v : 0.0f;
    }
    return v0;
}

// rule 22: the 5-tap kernel (1/16, 1/4, 3/8, 1/4, 1/16) at tap i = -2 .. 2; a product of two is exact (two significant bits at most each)
RT_RULE float atrous_tap(int i) { return i == 0 ? 0.375f : (i == -1 || i == 1) ? 0.25f : 0.0625f; }
// rule 22: the edge term of pixel p and tap q from their normals, luminances and variances; in = 1 / k_normal^2, kl2 = k_lum^2
RT_RULE float atrous_edge(float np0, float np1, float np2, float nq0, float nq1, float nq2, float in, float lp, float lq, float vp, float vq, float kl2) {
    const float a0 = np0 - nq0, a1 = np1 - nq1, a2 = np2 - nq2;
    const float gn = ((a0 * a0 + a1 * a1) + a2 * a2) * in;
    const float d = lp - lq;
    const float gl = (d * d) / (kl2 * (vp + vq) + 1e-10f);
    float g = 0.0f;
    if (gn > g) g = gn;
    if (gl > g) g = gl;
    return g;
}
// rule 22: the weight of the centre tap at n samples, and of any other tap (hj, hi its two kernel values, g its edge term)
RT_RULE float atrous_centre_weight(float n) { return (0.375f * 0.375f) * n; }
RT_RULE float atrous_tap_weight(float hj, float hi, float g, float n) { return ((hj * hi) * falloff(g)) * n; }

// rule 29: a record that is a LIGHT -- the library's own light test (rt_scene.hip light_test; .cl:135-138,266)
RT_RULE bool light_record(const rt_sphere &s) { return !((s.e.x == 0.f) && (s.e.z == 0.f)); }

// rule 29: a pair of the list as both sides hold it -- S's and D's {centre, radius} of the light l, then of the occluder j, then l and j as words and
// two zero words: five aligned texels
constexpr int kShadowPairFloats = 20;

// rule 30: the state of a pair at the point X -- where the occluder {c, r} stands in the cone from X to the light's bounding sphere {L, rl}:
// 0 clear, 1 penumbra, 2 umbra.  No square root; a NaN past the first test fails every comparison and so gives 1
RT_RULE int shadow_state(float x0, float x1, float x2, float l0, float l1, float l2, float rl, float c0, float c1, float c2, float r) {
    const float g0 = l0 - x0, g1 = l1 - x1, g2 = l2 - x2;
    const float ll = dot3(g0, g1, g2, g0, g1, g2);
    if (!(ll > 0.0f)) return 0;
    float s = dot3(c0 - x0, c1 - x1, c2 - x2, g0, g1, g2) / ll;
    if (!(s > 0.0f)) s = 0.0f;
    if (s > 1.0f) s = 1.0f;
    const float e0 = (x0 + g0 * s) - c0, e1 = (x1 + g1 * s) - c1, e2 = (x2 + g2 * s) - c2;
    const float d2 = dot3(e0, e1, e2, e0, e1, e2), pen = rl * s, a = r + pen, b = r - pen;
    if (d2 > a * a) return 0;
    if (b > 0.0f && d2 < b * b) return 2;
    return 1;
}
// rule 31: a pair CHANGES a pixel whose states before and after the move are these
RT_RULE bool shadow_changes(int before, int after) { return before != after || before == 1 || after == 1; }
// rule 32: the cap of a flagged pixel's history, after rule 18's (hk: rule 26's frames, capped in proportion; a colour-only caller passes a dummy)
RT_RULE void shadow_cap(float &nh, float &hk, float keep) {
    if (nh > keep) {
        hk = hk * (keep / nh);
        nh = keep;
    }
}

// rule 19: the blend of D's colour (c at nd samples; have_d false at pass 0: c is 0 and not counted) with the history of rule 18's sums, into
// (t0, t1, t2) at tn samples.  (Four references, not a struct or an array: either reaches the kernel as a vector and moves its schedule.)
// kShadow: rule 32 between the cap and the blend, for a pixel that rule 31 `flagged`; without it the two last arguments are not read.
template <bool kShadow>
RT_RULE void temporal_blend_as(float &t0, float &t1, float &t2, float &tn, float c0, float c1, float c2, float nd, bool have_d, float sw, float sn, float sc0,
                               float sc1, float sc2, float max_history, [[maybe_unused]] bool flagged, [[maybe_unused]] float keep) {
    t0 = c0, t1 = c1, t2 = c2, tn = nd;
    if (sw > 0.0f) {
        float nh = sn / sw;
        if (nh > max_history) nh = max_history;
        if constexpr (kShadow) {
            float hk = 0.0f;
            if (flagged) shadow_cap(nh, hk, keep);
        }
        const float h0 = sc0 / sw, h1 = sc1 / sw, h2 = sc2 / sw;
        if (!have_d) t0 = h0, t1 = h1, t2 = h2, tn = nh;
        else {
            const float inv = 1.0f / (nd + nh);
            t0 = (c0 * nd + h0 * nh) * inv, t1 = (c1 * nd + h1 * nh) * inv, t2 = (c2 * nd + h2 * nh) * inv, tn = nd + nh;
        }
    }
}
RT_RULE void temporal_blend(float &t0, float &t1, float &t2, float &tn, float c0, float c1, float c2, float nd, bool have_d, float sw, float sn, float sc0, float sc1,
                            float sc2, float max_history) {
    temporal_blend_as<false>(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history, false, 0.0f);
}

// rule 27: the variance of a temporal mean from its moments m1 and m2 over k frames; 0 below two frames, never negative (a NaN fails both tests)
RT_RULE float moments_variance(float m1, float m2, float k) {
    const float d = m2 - m1 * m1;
    return (k > 1.0f && d > 0.0f) ? d / (k - 1.0f) : 0.0f;
}

// rules 26-27: the blend of D's luminance ld (at nd samples; have_d false at pass 0: ld is not counted) with the history of rule 18's sums sw and sn
// and rule 26's sums s1, s2 and sk, into (m1, m2, k, v).  nh and inv are formed as temporal_blend forms them -- rule 32 included, under kShadow.
template <bool kShadow>
RT_RULE void moments_blend_as(float &m1, float &m2, float &k, float &v, float ld, float nd, bool have_d, float sw, float sn, float s1, float s2, float sk,
                              float max_history, [[maybe_unused]] bool flagged, [[maybe_unused]] float keep) {
    m1 = have_d ? ld : 0.0f, m2 = have_d ? ld * ld : 0.0f, k = have_d ? 1.0f : 0.0f;
    if (sw > 0.0f) {
        float nh = sn / sw;
        const float h1 = s1 / sw, h2 = s2 / sw;
        float hk = sk / sw;
        if (nh > max_history) {
            hk = hk * (max_history / nh);                          // frames are capped in proportion to samples
            nh = max_history;
        }
        if constexpr (kShadow) {
            if (flagged) shadow_cap(nh, hk, keep);
        }
        if (!have_d) m1 = h1, m2 = h2, k = hk;
        else {
            const float inv = 1.0f / (nd + nh);
            m1 = (ld * nd + h1 * nh) * inv, m2 = ((ld * ld) * nd + h2 * nh) * inv, k = hk + 1.0f;
        }
    }
    v = moments_variance(m1, m2, k);
}
RT_RULE void moments_blend(float &m1, float &m2, float &k, float &v, float ld, float nd, bool have_d, float sw, float sn, float s1, float s2, float sk,
                           float max_history) {
    moments_blend_as<false>(m1, m2, k, v, ld, nd, have_d, sw, sn, s1, s2, sk, max_history, false, 0.0f);
}

// rule 28: V0 of a pixel whose moments texel holds k frames and the estimate v, where rule 21 gives v21
RT_RULE float variance_from_history(bool usable, float k, float v, float k_min, float v21) { return (usable && k >= k_min) ? v : v21; }

}  // namespace rt
