// rt_host.cpp -- the library's host-side code that needs no GPU, C ABI.  Plain C++, strict binary32/binary64 (-ffp-contract=off).
//   Either side of the render path: the seed streams (the one the reference draws from the C library, and the numbered ones), the
//   camera basis, the built-in scene and the .scn reader.
//   The host statements of the library's extensions, as plain loops, with their defaults and parameter rules: rt_denoise_planes and
//   rt_denoise_pair_planes with their guided forms (rules 1-6, 13-14), rt_features_planes (rules 10-12), rt_reproject_planes (rules 15-19),
//   rt_atrous_planes (rules 20-23), their forms with temporal moments, rt_reproject_moments_planes and rt_atrous_moments_planes (rules 25-28), and rt_reproject_shadow_planes (rules 29-32 beside them).  The kernels are tested against them bit for bit.  The loops, the clamping and the order of the sums are written
//   here; the arithmetic of a rule is rt_rules.h's, which the kernels call too.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_rules.h"

// rt_last_error()'s thread-local text lives in rt_api.hip; host helpers report through this
extern "C" void rt_host_set_error(const char *msg);

namespace {

int host_fail(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    rt_host_set_error(buf);
    return RT_ERR_ARG;
}

// Vec::norm, Vec.cpp:28-30: the squared length is binary32, the square root and the
// reciprocal are binary64 (unqualified sqrt on a float picks ::sqrt(double) there).
rt_vec3 host_norm(rt_vec3 v) {
    const float len2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float inv = static_cast<float>(1 / std::sqrt(static_cast<double>(len2)));
    return rt_vec3{ v.x * inv, v.y * inv, v.z * inv };
}

rt_vec3 host_cross(rt_vec3 a, rt_vec3 b) {
    return rt_vec3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x };
}

}  // namespace

extern "C" {

void rt_compute_camera(rt_camera *cam, int w, int h) {
    if (!cam) return;
    cam->dir = host_norm(rt_vec3{ cam->target.x - cam->orig.x, cam->target.y - cam->orig.y,
                                  cam->target.z - cam->orig.z });
    const rt_vec3 up{ 0.f, 1.f, 0.f };
    const float fov = static_cast<float>((3.14159265358979323846 / 180.f) * 45.f);
    rt_vec3 cx = host_norm(host_cross(cam->dir, up));
    const float sx = w * fov / h;
    cam->x = rt_vec3{ cx.x * sx, cx.y * sx, cx.z * sx };
    rt_vec3 cy = host_norm(host_cross(cam->x, cam->dir));
    cam->y = rt_vec3{ cy.x * fov, cy.y * fov, cy.z * fov };
}

// glibc's rand() with its initial state (equivalent to srand(1)): the TYPE_3 additive
// generator x[i] = x[i-31] + x[i-3] (mod 2^32) over a 31-word table that is filled by the
// Lehmer generator 16807 * s mod (2^31 - 1), run for 310 steps before the first output;
// each output is x[i] >> 1.
// The stream is a pure function of the index, so its head is generated once per process and kept
// (up to kSeedCacheWords; a 1080p context needs 4.1 M words): creating a context, which
// rt_render() does on every call, then costs a copy instead of 4 million generator steps.
namespace {
struct RandState {
    uint32_t tab[31];
    int f, r;
    void init() {
        int64_t word = 1;
        tab[0] = 1;
        for (int i = 1; i < 31; ++i) {
            word = (16807 * word) % 2147483647;
            if (word < 0) word += 2147483647;
            tab[i] = static_cast<uint32_t>(word);
        }
        // front = index of x[i-31]'s slot, rear = x[i-3]'s; glibc starts them 3 apart
        f = 3;
        r = 0;
        for (int i = 0; i < 310; ++i) (void)step();
    }
    uint32_t step() {
        tab[f] += tab[r];
        const uint32_t v = tab[f] >> 1;
        f = (f + 1 == 31) ? 0 : f + 1;
        r = (r + 1 == 31) ? 0 : r + 1;
        return v;
    }
    uint32_t seed() {                                                 // OpenCLConfig.cpp:678-679
        const uint32_t v = step();
        return v < 2 ? 2u : v;
    }
};
constexpr size_t kSeedCacheWords = size_t(1) << 23;                   // 32 MiB
std::mutex g_seed_mutex;
std::vector<uint32_t> g_seed_head;                                    // seeds [0, size)
RandState g_seed_state;                                               // generator after g_seed_head.size() outputs
bool g_seed_started = false;
}  // namespace

void rt_default_seeds(uint32_t *seeds, size_t count) {
    if (!seeds) return;
    RandState tail;
    size_t have;
    {
        std::lock_guard<std::mutex> lock(g_seed_mutex);
        if (!g_seed_started) {
            g_seed_state.init();
            g_seed_started = true;
        }
        const size_t want = count < kSeedCacheWords ? count : kSeedCacheWords;
        if (g_seed_head.size() < want) {
            const size_t old = g_seed_head.size();
            g_seed_head.resize(want);
            for (size_t i = old; i < want; ++i) g_seed_head[i] = g_seed_state.seed();
        }
        have = count < g_seed_head.size() ? count : g_seed_head.size();
        memcpy(seeds, g_seed_head.data(), have * sizeof(uint32_t));
        tail = g_seed_state;                                          // continues at g_seed_head.size()
    }
    for (size_t i = have; i < count; ++i) seeds[i] = tail.seed();
}

// Seed stream `stream_id`: 0 is the default stream above; any other id draws pair i from the splitmix64 finaliser of
// (stream_id, i), clamped like the reference's own seeds (OpenCLConfig.cpp:676-680).  rt_seed_stream_async generates the
// same words on the device (rt_state.hip rt_seed_stream_kernel).
void rt_stream_seeds(uint64_t stream_id, uint32_t *seeds, size_t count) {
    if (!seeds) return;
    if (stream_id == 0) {
        rt_default_seeds(seeds, count);
        return;
    }
    for (size_t i = 0; 2 * i < count; ++i) {
        uint64_t z = stream_id * 0x9E3779B97F4A7C15ull + (uint64_t)i + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const uint32_t lo = (uint32_t)z, hi = (uint32_t)(z >> 32);
        seeds[2 * i] = lo < 2 ? 2u : lo;
        if (2 * i + 1 < count) seeds[2 * i + 1] = hi < 2 ? 2u : hi;      // (an odd count ends on a low half)
    }
}

int rt_demo_scene(rt_sphere *out, uint32_t cap) {
    static const rt_sphere demo[6] = {
        { 1000.f, { 0.f, -1000.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.75f, 0.75f, 0.75f }, RT_DIFF },
        { 12.f, { 40.f, 20.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.9f, 0.f, 0.f }, RT_REFR },
        { 11.f, { -35.f, 20.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.9f, 0.f }, RT_REFR },
        { 10.f, { 0.f, 25.f, -10.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.9f }, RT_REFR },
        { 9.f, { 20.f, 10.f, -5.f }, { 0.f, 0.f, 0.f }, { 0.9f, 0.f, 0.9f }, RT_REFR },
        { 7.f, { 0.f, 60.f, 0.f }, { 12.f, 12.f, 12.f }, { 0.f, 0.f, 0.f }, RT_DIFF },
    };
    if (!out || cap < 6) return -6;
    memcpy(out, demo, sizeof demo);
    return 6;
}

int rt_read_scene(const char *path, rt_sphere *out, uint32_t cap, uint32_t *count, rt_vec3 *orig,
                  rt_vec3 *target, int reference_doubling) {
    if (!path || !out || !count || !orig || !target) return host_fail("rt_read_scene: null argument");
    *count = 0;
    FILE *f = fopen(path, "r");
    if (!f) return host_fail("Failed to open file: %s", path);
    int got = fscanf(f, "camera %f %f %f  %f %f %f\n", &orig->x, &orig->y, &orig->z, &target->x,
                     &target->y, &target->z);
    if (got != 6) {
        fclose(f);
        return host_fail("Failed to read 6 camera parameters: %d", got);
    }
    unsigned n = 0;
    got = fscanf(f, "size %u\n", &n);
    if (got != 1) {
        fclose(f);
        return host_fail("Failed to read sphere count: %d", got);
    }
    const uint64_t total = reference_doubling ? 2ull * n : n;
    if (total > cap) {
        fclose(f);
        return host_fail("scene has %llu spheres, capacity %u", (unsigned long long)total, cap);
    }
    uint32_t at = 0;
    if (reference_doubling) {            // Utility.cpp:120: vector built with n zeroed spheres...
        memset(out, 0, sizeof(rt_sphere) * n);
        at = n;
    }
    for (unsigned i = 0; i < n; ++i) {   // ...then n more are appended (:154)
        rt_sphere s;
        memset(&s, 0, sizeof s);
        int mat = 0;
        got = fscanf(f, "sphere %f  %f %f %f  %f %f %f  %f %f %f  %d\n", &s.rad, &s.p.x, &s.p.y, &s.p.z,
                     &s.e.x, &s.e.y, &s.e.z, &s.c.x, &s.c.y, &s.c.z, &mat);
        if (mat < 0 || mat > 2) {
            fclose(f);
            return host_fail("Failed to read material type for sphere #%u: %d", i, mat);
        }
        if (got != 11) {
            fclose(f);
            return host_fail("Failed to read sphere #%u: %d", i, got);
        }
        s.refl = mat;
        out[at++] = s;
    }
    fclose(f);
    *count = at;
    return RT_OK;
}

// ---- rt_denoise_planes: the non-local-means filter of include/rt_api.h ("denoising"), rules 1-6, as plain loops ----
// rt_denoise_async runs the same arithmetic on the device (rt_denoise.hip) and is tested against this function bit for bit.

void rt_denoise_defaults(rt_denoise_params *p) {
    if (!p) return;
    p->search_radius = 5;
    p->patch_radius = 1;
    p->alpha = 1.0f;
    p->k = 0.45f;
}

// the parameter rules both entry points share (`p` == null: the defaults); hidden, like rt_host_set_error
int rt_host_denoise_params(const rt_denoise_params *p, rt_denoise_params *out) {
    rt_denoise_defaults(out);
    if (p) *out = *p;
    if (out->search_radius < 0 || out->search_radius > 8) return host_fail("rt_denoise: search_radius %d (0 .. 8)", out->search_radius);
    if (out->patch_radius < 0 || out->patch_radius > 2) return host_fail("rt_denoise: patch_radius %d (0 .. 2)", out->patch_radius);
    if (!std::isfinite(out->alpha) || out->alpha < 0.f) return host_fail("rt_denoise: alpha %g (finite, >= 0)", (double)out->alpha);
    if (!std::isfinite(out->k) || out->k <= 0.f) return host_fail("rt_denoise: k %g (finite, > 0)", (double)out->k);
    return RT_OK;
}

void rt_guide_defaults(rt_guide_params *g) {
    if (!g) return;
    g->k_albedo = 0.15f;
    g->k_normal = 0.2f;
    g->k_depth = 0.05f;
    g->reserved = 0;
}

// the guide's parameter rules (every entry point that takes or holds one); hidden, like rt_host_denoise_params
int rt_host_guide_params(const rt_guide_params *g) {
    if (!g) return host_fail("rt_guide_params: null");
    const float k[3] = { g->k_albedo, g->k_normal, g->k_depth };
    static const char *const name[3] = { "k_albedo", "k_normal", "k_depth" };
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(k[i]) || k[i] <= 0.f) return host_fail("rt_guide_params: %s %g (finite, > 0)", name[i], (double)k[i]);
    if (g->reserved != 0) return host_fail("rt_guide_params: reserved %u (0)", g->reserved);
    return RT_OK;
}

}  // extern "C"

namespace {

inline int dn_cl(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// rules 1 and 2: the variance of the mean of the two halves, smoothed over 3x3, clamped
std::vector<float> smoothed_variance(const float *a, const float *b, int w, int h) {
    const auto at = [w](int y, int x) { return 3 * ((size_t)y * (size_t)w + (size_t)x); };
    const size_t px = (size_t)w * (size_t)h;
    std::vector<float> V(3 * px), Vs(3 * px);
    for (size_t i = 0; i < 3 * px; ++i) {
        const float d = (a[i] - b[i]) * 0.5f;
        V[i] = d * d;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                float sum = 0.f;
                for (int j = -1; j <= 1; ++j)
                    for (int i = -1; i <= 1; ++i) {
                        const float v = V[at(dn_cl(y + j, h), dn_cl(x + i, w)) + c];
                        sum = (j == -1 && i == -1) ? v : sum + v;
                    }
                Vs[at(y, x) + c] = sum * (1.0f / 9.0f);
            }
    return Vs;
}

// rules 3 to 6 with the image and the guide apart: the weights come from `guide` (rule 3's t) and the variance plane `var`, the values that are
// tested (rule 5) and averaged (rule 6) from `img`.  rt_denoise_planes: img == guide == the merged frame, var = Vs.  rt_denoise_pair_planes: img
// one half, guide the other, var = Vh.  `gd` non-null (the guided functions): rule 14, the weight never above rule 13's of the feature plane `feat`
void nlm_planes(float *out, const float *img, const float *guide, const std::vector<float> &var, int w, int h, const rt_denoise_params &q,
                const float *feat, const rt_guide_params *gd) {
    const int R = q.search_radius, P = q.patch_radius;
    const float ia = gd ? 1.0f / (gd->k_albedo * gd->k_albedo) : 0.f, in = gd ? 1.0f / (gd->k_normal * gd->k_normal) : 0.f, id = gd ? 1.0f / (gd->k_depth * gd->k_depth) : 0.f;
    const float alpha = q.alpha, kk = q.k * q.k, inv = 1.0f / (float)(3 * (2 * P + 1) * (2 * P + 1));
    const auto at = [w](int y, int x) { return 3 * ((size_t)y * (size_t)w + (size_t)x); };
    const size_t px = (size_t)w * (size_t)h;
    std::vector<float> num(3 * px, 0.0f), den(px, 0.0f), e(px);
    for (int oy = -R; oy <= R; ++oy)
        for (int ox = -R; ox <= R; ++ox) {
            if (oy == 0 && ox == 0) {                        // 5. the pixel itself: weight 1, whatever it holds
                for (size_t i = 0; i < px; ++i) {
                    for (int c = 0; c < 3; ++c) num[3 * i + c] = num[3 * i + c] + 1.0f * img[3 * i + c];
                    den[i] = den[i] + 1.0f;
                }
                continue;
            }
            // 3. e(x, o) for every pixel x: it depends on x and o only, so one evaluation serves every patch that covers x
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const size_t ip = at(y, x), iq = at(dn_cl(y + oy, h), dn_cl(x + ox, w));
                    float d[3];
                    for (int c = 0; c < 3; ++c) {
                        const float vp = var[ip + c], vq = var[iq + c];
                        d[c] = rt::nlm_term(guide[ip + c] - guide[iq + c], rt::nlm_offset(alpha, vp, vq), rt::nlm_denominator(kk, vp, vq));
                    }
                    e[(size_t)y * w + x] = (d[0] + d[1]) + d[2];
                }
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const int qy = y + oy, qx = x + ox;
                    if (qy < 0 || qy >= h || qx < 0 || qx >= w) continue;     // 5. p + o outside the image
                    float S = 0.f;                                            // 4. the patch sum, at clamped positions
                    for (int dy = -P; dy <= P; ++dy)
                        for (int dx = -P; dx <= P; ++dx) {
                            const float v = e[(size_t)dn_cl(y + dy, h) * w + dn_cl(x + dx, w)];
                            S = (dy == -P && dx == -P) ? v : S + v;
                        }
                    const float T = S * inv;
                    const float *dq = img + at(qy, qx);
                    if (std::isnan(T) || !rt::finite3(dq[0], dq[1], dq[2])) continue;
                    const float g = T > 0.f ? T : 0.f;
                    float wgt = rt::falloff(g);
                    const size_t i = (size_t)y * w + x;
                    if (gd) {                                                 // 14. (13.: words 0-6 of the two records; word 7 is not read)
                        const float wf = rt::guide_weight(feat + 8 * i, feat + 8 * ((size_t)qy * w + qx), ia, in, id);
                        wgt = wf < wgt ? wf : wgt;
                    }
                    for (int c = 0; c < 3; ++c) num[3 * i + c] = num[3 * i + c] + wgt * dq[c];
                    den[i] = den[i] + wgt;
                }
        }
    for (size_t i = 0; i < px; ++i)                                           // 6.
        for (int c = 0; c < 3; ++c) out[3 * i + c] = num[3 * i + c] / den[i];
}

}  // namespace

extern "C" {

// `g` == null: the filter without a guide; else its parameters checked and the feature plane there
static int guide_args(const char *call, const float *feat, const rt_guide_params *g) {
    if (!g) return RT_OK;
    if (!feat) return host_fail("%s: null feature plane", call);
    return rt_host_guide_params(g);
}

int rt_denoise_guided_planes(float *out, const float *merged, const float *a, const float *b, const float *feat, int w, int h, const rt_denoise_params *p,
                             const rt_guide_params *g) {
    if (!out || !merged || !a || !b) return host_fail("rt_denoise_planes: null plane");
    if (w < 1 || h < 1) return host_fail("rt_denoise_planes: %dx%d", w, h);
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    if (guide_args("rt_denoise_guided_planes", feat, g) != RT_OK) return RT_ERR_ARG;
    nlm_planes(out, merged, merged, smoothed_variance(a, b, w, h), w, h, q, feat, g);
    return RT_OK;
}

int rt_denoise_planes(float *out, const float *merged, const float *a, const float *b, int w, int h, const rt_denoise_params *p) {
    return rt_denoise_guided_planes(out, merged, a, b, nullptr, w, h, p, nullptr);
}

// ---- rt_denoise_pair_planes: the cross-filtered halves of include/rt_api.h ("the error of the filtered frame"), as plain loops ----
// rt_denoise_pair_async runs the same arithmetic on the device (rt_denoise.hip) and is tested against this function bit for bit.
int rt_denoise_pair_guided_planes(float *out_a, float *out_b, const float *a, const float *b, const float *feat, int w, int h, const rt_denoise_params *p,
                                  const rt_guide_params *g) {
    if (!out_a || !out_b || !a || !b) return host_fail("rt_denoise_pair_planes: null plane");
    if (w < 1 || h < 1) return host_fail("rt_denoise_pair_planes: %dx%d", w, h);
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    if (guide_args("rt_denoise_pair_guided_planes", feat, g) != RT_OK) return RT_ERR_ARG;
    const size_t n = 3 * (size_t)w * (size_t)h;
    if (q.search_radius == 0) {                              // the window is the pixel itself: the halves, bit for bit
        memcpy(out_a, a, n * sizeof(float));
        memcpy(out_b, b, n * sizeof(float));
        return RT_OK;
    }
    std::vector<float> Vh = smoothed_variance(a, b, w, h);
    for (size_t i = 0; i < n; ++i) Vh[i] = Vh[i] + Vh[i];    // the variance of ONE half: twice that of the mean
    nlm_planes(out_a, a, b, Vh, w, h, q, feat, g);           // FA: A's values, weights from B
    nlm_planes(out_b, b, a, Vh, w, h, q, feat, g);           // FB: B's values, weights from A
    return RT_OK;
}

int rt_denoise_pair_planes(float *out_a, float *out_b, const float *a, const float *b, int w, int h, const rt_denoise_params *p) {
    return rt_denoise_pair_guided_planes(out_a, out_b, a, b, nullptr, w, h, p, nullptr);
}

// ---- rt_features_planes: the feature plane of include/rt_api.h ("feature planes"), rules 10-12, as plain loops ----
// rt_features_async forms the same words on the device (rt_features.hip) and is tested against this function bit for bit.
int rt_features_planes(float *out, const rt_sphere *spheres, uint32_t count, const rt_camera *cam, int w, int h) {
    if (!out || !cam || (count > 0 && !spheres)) return host_fail("rt_features_planes: null argument");
    if (w < 1 || h < 1) return host_fail("rt_features_planes: %dx%d", w, h);
    const rt::PixelCamera pc = rt::pixel_camera(*cam);
    const float inv_w = 1.f / (float)w, inv_h = 1.f / (float)h;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            // 10. the ray through the pixel's centre
            const rt::PixelRay r = rt::pixel_ray(pc, x, y, inv_w, inv_h);
            // 11. the nearest record in scene order (.cl:215-232)
            float t = 1e20f;
            uint32_t id = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < count; ++i) {
                const rt_sphere &s = spheres[i];
                const float dist = rt::sphere_distance(s.p.x, s.p.y, s.p.z, s.rad * s.rad, r);
                if (dist != 0.f && dist < t) {
                    t = dist;
                    id = i;
                }
            }
            // 12. the values
            float *o = out + 8 * ((size_t)(h - 1 - y) * (size_t)w + (size_t)x);
            if (t < 1e20f) {
                const rt_sphere &s = spheres[id];
                const rt::Float3 nrm = rt::hit_normal(r, t, s.p.x, s.p.y, s.p.z);
                o[0] = s.c.x + s.e.x, o[1] = s.c.y + s.e.y, o[2] = s.c.z + s.e.z;
                o[3] = nrm.x, o[4] = nrm.y, o[5] = nrm.z;
                o[6] = t;
            } else {
                for (int k = 0; k < 7; ++k) o[k] = 0.0f;
                id = 0xFFFFFFFFu;
            }
            memcpy(o + 7, &id, sizeof id);
        }
    return RT_OK;
}

}  // extern "C"

// ---- rt_reproject_planes: temporal reprojection of include/rt_api.h ("temporal reprojection"), rules 15-19, as plain loops ----
// rt_reproject_async forms the same words on the device (rt_reproject.hip) and is tested against this function bit for bit.
namespace {

inline float rp_dot(const float *a, const float *b) { return rt::dot3(a[0], a[1], a[2], b[0], b[1], b[2]); }

}  // namespace

extern "C" {

void rt_reproject_defaults(rt_reproject_params *p) {
    if (!p) return;
    p->k_pos = 4.0f;
    p->max_history = 64.0f;
    p->reserved[0] = p->reserved[1] = 0;
}

// the parameter rules both entry points share (`p` == null: the defaults); hidden, like rt_host_denoise_params
int rt_host_reproject_params(const rt_reproject_params *p, rt_reproject_params *out) {
    rt_reproject_defaults(out);
    if (p) *out = *p;
    if (!std::isfinite(out->k_pos) || out->k_pos <= 0.f) return host_fail("rt_reproject: k_pos %g (finite, > 0)", (double)out->k_pos);
    if (!std::isfinite(out->max_history) || out->max_history <= 0.f) return host_fail("rt_reproject: max_history %g (finite, > 0)", (double)out->max_history);
    if (out->reserved[0] != 0 || out->reserved[1] != 0) return host_fail("rt_reproject: reserved %u, %u (0)", out->reserved[0], out->reserved[1]);
    return RT_OK;
}

void rt_shadow_history_defaults(rt_shadow_history_params *p) {
    if (!p) return;
    p->keep = 2.0f;                     // what the prototype measured best (include/rt_api.h, "shadow-aware history")
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

// the parameter rule rt_set_shadow_history and rt_reproject_shadow_planes share; hidden, like rt_host_moments_params
int rt_host_shadow_history_params(const rt_shadow_history_params *p, rt_shadow_history_params *out) {
    rt_shadow_history_defaults(out);
    if (p) *out = *p;
    if (!std::isfinite(out->keep) || !(out->keep >= 0.f)) return host_fail("rt_shadow_history: keep %g (finite, >= 0)", (double)out->keep);
    if (out->reserved[0] != 0 || out->reserved[1] != 0 || out->reserved[2] != 0)
        return host_fail("rt_shadow_history: reserved %u, %u, %u (0)", out->reserved[0], out->reserved[1], out->reserved[2]);
    return RT_OK;
}

// rule 29: the pair list of the records S and D, `count` each, in its order; the first `cap` pairs into `out` (rt::kShadowPairFloats floats each: S's and
// D's {centre, radius} of l, then of j, then l and j as words and two zero words), or nothing (out null).  Returns how many pairs there are.  Hidden:
// the host loops below and rt_reproject_async (rt_reproject.hip, over the two contexts' mirrors) build their lists with it
size_t rt_host_shadow_pairs(const rt_sphere *S, const rt_sphere *D, uint32_t count, float *out, size_t cap) {
    const auto changed = [&](uint32_t j) { return memcmp(&S[j], &D[j], 4 * sizeof(float)) != 0; };        // {rad, p}: the record's first four words
    const auto phantom = [&](uint32_t j) { return S[j].rad == 0.0f && D[j].rad == 0.0f; };
    const auto put = [](float *o, const rt_sphere &s) { o[0] = s.p.x, o[1] = s.p.y, o[2] = s.p.z, o[3] = s.rad; };
    size_t n = 0;
    for (uint32_t l = 0; l < count; ++l) {
        if (phantom(l) || !rt::light_record(D[l])) continue;
        const bool l_changed = changed(l);
        for (uint32_t j = 0; j < count; ++j) {
            if (j == l || phantom(j) || !(l_changed || changed(j))) continue;
            if (out && n < cap) {
                float *o = out + rt::kShadowPairFloats * n;
                put(o, S[l]), put(o + 4, D[l]), put(o + 8, S[j]), put(o + 12, D[j]);
                const uint32_t words[4] = { l, j, 0, 0 };
                memcpy(o + 16, words, sizeof words);
            }
            ++n;
        }
    }
    return n;
}

int rt_shadow_history_pairs(const rt_sphere *src_spheres, const rt_sphere *dst_spheres, uint32_t count, uint32_t *out_lj, uint32_t cap) {
    if ((count > 0 && (!src_spheres || !dst_spheres)) || (cap > 0 && !out_lj)) {
        host_fail("rt_shadow_history_pairs: null argument");
        return -1;
    }
    const size_t n = rt_host_shadow_pairs(src_spheres, dst_spheres, count, nullptr, 0);
    std::vector<float> list(rt::kShadowPairFloats * std::min<size_t>(n, cap));
    rt_host_shadow_pairs(src_spheres, dst_spheres, count, list.data(), std::min<size_t>(n, cap));
    for (size_t k = 0; k < std::min<size_t>(n, cap); ++k) memcpy(out_lj + 2 * k, list.data() + rt::kShadowPairFloats * k + 16, 2 * sizeof(uint32_t));
    return (int)n;
}

}  // extern "C"

namespace {

// rules 15-19 and, where out_m is not null, rules 25-27 beside them (src_m: S's moments plane, or null for rule 25's luminance of U): the loops of
// rt_reproject_planes and rt_reproject_moments_planes, which therefore cannot differ in a word of out_rgbn.  sp not null: rules 29-32 between the
// history and the blend (out_k, where not null: rule 31's flags; all 0 without sp)
int reproject_loops(const char *call, float *out_rgbn, float *out_m, uint8_t *out_k, const rt_reproject_view *dst, const rt_reproject_view *src, const float *src_m,
                    uint32_t count, int w, int h, const rt_reproject_params *p, const rt_shadow_history_params *sp) {
    if (!out_rgbn || !dst || !src) return host_fail("%s: null argument", call);
    if (w < 1 || h < 1) return host_fail("%s: %dx%d", call, w, h);
    for (const rt_reproject_view *v : { dst, src }) {
        const char *side = v == dst ? "dst" : "src";
        if (v->channels != 3 && v->channels != 4) return host_fail("%s: %s has %d channels (3 or 4)", call, side, v->channels);
        if (v->passes < 0) return host_fail("%s: %s holds %d passes", call, side, v->passes);
        if (!v->feat || !v->cam || (count > 0 && !v->spheres)) return host_fail("%s: %s has a null feature plane, camera or records", call, side);
    }
    if (!src->plane) return host_fail("%s: src has a null plane", call);
    if (!dst->plane && dst->passes != 0) return host_fail("%s: dst has a null plane and %d passes", call, dst->passes);
    rt_reproject_params q;
    if (rt_host_reproject_params(p, &q) != RT_OK) return RT_ERR_ARG;
    rt_shadow_history_params sq{};
    if (sp && rt_host_shadow_history_params(sp, &sq) != RT_OK) return RT_ERR_ARG;
    // 29. the lists
    std::vector<float> pairs;
    if (sp) {
        pairs.resize(rt::kShadowPairFloats * rt_host_shadow_pairs(src->spheres, dst->spheres, count, nullptr, 0));
        rt_host_shadow_pairs(src->spheres, dst->spheres, count, pairs.data(), pairs.size() / rt::kShadowPairFloats);
    }

    const rt_camera &camS = *src->cam;
    const rt::PixelCamera pcD = rt::pixel_camera(*dst->cam), pcS = rt::pixel_camera(camS);
    const float inv_w = 1.f / (float)w, inv_h = 1.f / (float)h, fw = (float)w, fh = (float)h;
    const float sdir[3] = { camS.dir.x, camS.dir.y, camS.dir.z }, sx[3] = { camS.x.x, camS.x.y, camS.x.z }, sy[3] = { camS.y.x, camS.y.y, camS.y.z };
    const float dd = rp_dot(sdir, sdir), xx = rp_dot(sx, sx), yy = rp_dot(sy, sy);
    const float foot = sqrtf(xx) * (1.f / (float)w);             // rule 17: a pixel's footprint per unit of distance
    const float nd = (float)dst->passes;
    const int cs = src->channels, cd = dst->channels;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t at = (size_t)(h - 1 - y) * (size_t)w + (size_t)x;
            float sw = 0.0f, sn = 0.0f, sc[3] = { 0.0f, 0.0f, 0.0f };
            float s1 = 0.0f, s2 = 0.0f, sk = 0.0f;                    // 26. the history's moments
            // 15. the point and where it was
            uint32_t id;
            memcpy(&id, dst->feat + 8 * at + 7, sizeof id);
            float P[3] = { 0.0f, 0.0f, 0.0f }, Pp[3] = { 0.0f, 0.0f, 0.0f };
            if (id < count) {                                         // (0xFFFFFFFF: the sky)
                const float t = dst->feat[8 * at + 6];
                float v[3];
                const rt::PixelRay r = rt::pixel_ray(pcD, x, y, inv_w, inv_h);
                const float o[3] = { r.ox, r.oy, r.oz }, d[3] = { r.dx, r.dy, r.dz };
                const rt_vec3 &pd = dst->spheres[id].p, &ps = src->spheres[id].p;
                const float m[3] = { pd.x - ps.x, pd.y - ps.y, pd.z - ps.z };
                for (int c = 0; c < 3; ++c) P[c] = o[c] + d[c] * t, Pp[c] = P[c] - m[c];
                // 16. where S saw it
                v[0] = Pp[0] - camS.orig.x, v[1] = Pp[1] - camS.orig.y, v[2] = Pp[2] - camS.orig.z;
                const float z = rp_dot(v, sdir);
                if (z > 0.0f) {
                    const float kx = (rp_dot(v, sx) * dd) / (z * xx), ky = (rp_dot(v, sy) * dd) / (z * yy);
                    const float fx = (kx + 0.5f) * fw, fy = (ky + 0.5f) * fh;
                    if (fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                        const float x0 = std::floor(fx), y0 = std::floor(fy), ax = fx - x0, ay = fy - y0;
                        // 17. the taps
                        for (int j = 0; j < 2; ++j)
                            for (int i = 0; i < 2; ++i) {
                                const int qx = (int)x0 + i, qy = (int)y0 + j;
                                const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                                const size_t aq = (size_t)(h - 1 - qy) * (size_t)w + (size_t)qx;
                                uint32_t idq;
                                memcpy(&idq, src->feat + 8 * aq + 7, sizeof idq);
                                if (idq != id) continue;
                                const float tq = src->feat[8 * aq + 6];
                                const rt::PixelRay rq = rt::pixel_ray(pcS, qx, qy, inv_w, inv_h);
                                const float oq[3] = { rq.ox, rq.oy, rq.oz }, dq[3] = { rq.dx, rq.dy, rq.dz };
                                float e[3];
                                for (int c = 0; c < 3; ++c) e[c] = (oq[c] + dq[c] * tq) - Pp[c];
                                const float rr = q.k_pos * (tq * foot);
                                if (!(rp_dot(e, e) <= rr * rr)) continue;
                                const float *u = src->plane + (size_t)cs * aq;
                                const float un = cs == 4 ? u[3] : (float)src->passes;
                                if (!rt::usable(u[0], u[1], u[2], un)) continue;
                                // 18. the history
                                sw = sw + b;
                                sn = sn + b * un;
                                for (int c = 0; c < 3; ++c) sc[c] = sc[c] + b * u[c];
                                if (!out_m) continue;
                                // 25. the tap's moments, 26. their sums
                                float m1q, m2q, kq;
                                if (src_m) m1q = src_m[4 * aq], m2q = src_m[4 * aq + 1], kq = src_m[4 * aq + 2];
                                else {
                                    const float lq = rt::luminance(u[0], u[1], u[2]);
                                    m1q = lq, m2q = lq * lq, kq = 1.0f;
                                }
                                s1 = s1 + b * m1q;
                                s2 = s2 + b * m2q;
                                sk = sk + b * kq;
                            }
                    }
                }
            }
            // 31. the flag: a pixel with history and a newer sample, under a pair whose state at it changed (sw > 0.0f implies id < count)
            bool flagged = false;
            if (sw > 0.0f && dst->passes != 0)
                for (size_t k = 0; k < pairs.size() && !flagged; k += rt::kShadowPairFloats) {
                    const float *g = pairs.data() + k;
                    uint32_t lj[2];
                    memcpy(lj, g + 16, sizeof lj);
                    if (id == lj[0] || id == lj[1]) continue;
                    const int before = rt::shadow_state(Pp[0], Pp[1], Pp[2], g[0], g[1], g[2], g[3], g[8], g[9], g[10], g[11]);          // 30.
                    const int after = rt::shadow_state(P[0], P[1], P[2], g[4], g[5], g[6], g[7], g[12], g[13], g[14], g[15]);
                    flagged = rt::shadow_changes(before, after);
                }
            if (out_k) out_k[at] = flagged ? 1 : 0;
            // 19. the blend (D's plane is not read at pass 0), with 32. the cap of a flagged pixel
            const float *CD = dst->passes != 0 ? dst->plane + (size_t)cd * at : nullptr;
            float *T = out_rgbn + 4 * at;
            rt::temporal_blend_as<true>(T[0], T[1], T[2], T[3], CD ? CD[0] : 0.0f, CD ? CD[1] : 0.0f, CD ? CD[2] : 0.0f, nd, CD != nullptr, sw, sn, sc[0], sc[1], sc[2],
                                        q.max_history, flagged, sq.keep);
            if (!out_m) continue;
            // 27. the moments' blend
            float *M = out_m + 4 * at;
            const float lD = CD ? rt::luminance(CD[0], CD[1], CD[2]) : 0.0f;
            rt::moments_blend_as<true>(M[0], M[1], M[2], M[3], lD, nd, CD != nullptr, sw, sn, s1, s2, sk, q.max_history, flagged, sq.keep);
        }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_reproject_planes(float *out_rgbn, const rt_reproject_view *dst, const rt_reproject_view *src, uint32_t count, int w, int h,
                        const rt_reproject_params *p) {
    return rt_reproject_shadow_planes(out_rgbn, nullptr, nullptr, dst, src, nullptr, count, w, h, p, nullptr);
}

int rt_reproject_moments_planes(float *out_rgbn, float *out_m, const rt_reproject_view *dst, const rt_reproject_view *src, const float *src_m, uint32_t count, int w,
                                int h, const rt_reproject_params *p) {
    if (!out_m) return host_fail("rt_reproject_moments_planes: null argument");
    return rt_reproject_shadow_planes(out_rgbn, out_m, nullptr, dst, src, src_m, count, w, h, p, nullptr);
}

int rt_reproject_shadow_planes(float *out_rgbn, float *out_m, uint8_t *out_k, const rt_reproject_view *dst, const rt_reproject_view *src, const float *src_m,
                               uint32_t count, int w, int h, const rt_reproject_params *p, const rt_shadow_history_params *sp) {
    const char *const call = sp ? "rt_reproject_shadow_planes" : out_m ? "rt_reproject_moments_planes" : "rt_reproject_planes";     // (each refusal keeps its caller's name)
    return reproject_loops(call, out_rgbn, out_m, out_k, dst, src, src_m, count, w, h, p, sp);
}

}  // extern "C"

// ---- rt_atrous_planes: the edge-avoiding wavelet filter of include/rt_api.h ("edge-avoiding wavelet filter"), rules 20-23, as plain loops ----
// rt_atrous_async forms the same words on the device (rt_atrous.hip) and is tested against this function bit for bit.
extern "C" {

void rt_atrous_defaults(rt_atrous_params *p) {
    if (!p) return;
    p->levels = 3;
    p->k_lum = 1.5f;
    p->k_normal = 0.3f;
    p->reserved = 0;
}

// the parameter rules both entry points share (`p` == null: the defaults); hidden, like rt_host_reproject_params
int rt_host_atrous_params(const rt_atrous_params *p, rt_atrous_params *out) {
    rt_atrous_defaults(out);
    if (p) *out = *p;
    if (out->levels < 0 || out->levels > 5) return host_fail("rt_atrous: levels %d (0 .. 5)", out->levels);
    if (!std::isfinite(out->k_lum) || out->k_lum <= 0.f) return host_fail("rt_atrous: k_lum %g (finite, > 0)", (double)out->k_lum);
    if (!std::isfinite(out->k_normal) || out->k_normal <= 0.f) return host_fail("rt_atrous: k_normal %g (finite, > 0)", (double)out->k_normal);
    if (out->reserved != 0) return host_fail("rt_atrous: reserved %u (0)", out->reserved);
    return RT_OK;
}

void rt_moments_defaults(rt_moments_params *p) {
    if (!p) return;
    p->k_min = 4.0f;                    // SVGF's four frames
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

// the parameter rule rt_set_temporal_moments and rt_atrous_moments_planes share (`p` == null: the defaults); hidden, like rt_host_atrous_params
int rt_host_moments_params(const rt_moments_params *p, rt_moments_params *out) {
    rt_moments_defaults(out);
    if (p) *out = *p;
    if (!std::isfinite(out->k_min) || !(out->k_min >= 1.f)) return host_fail("rt_moments: k_min %g (finite, >= 1)", (double)out->k_min);
    if (out->reserved[0] != 0 || out->reserved[1] != 0 || out->reserved[2] != 0)
        return host_fail("rt_moments: reserved %u, %u, %u (0)", out->reserved[0], out->reserved[1], out->reserved[2]);
    return RT_OK;
}

}  // extern "C"

namespace {

// rules 20-23 and, where m is not null, rule 28 in place of rule 21 (k_min from the caller's checked parameters): the loops of rt_atrous_planes and
// rt_atrous_moments_planes
int atrous_loops(const char *call, float *out_rgbv, const float *plane, int channels, int passes, const float *m, float k_min, const float *feat, int w, int h,
                 const rt_atrous_params *p) {
    if (!out_rgbv || !plane || !feat) return host_fail("%s: null argument", call);
    if (w < 1 || h < 1) return host_fail("%s: %dx%d", call, w, h);
    if (channels != 3 && channels != 4) return host_fail("%s: %d channels (3 or 4)", call, channels);
    if (passes < 0) return host_fail("%s: %d passes", call, passes);
    rt_atrous_params q;
    if (rt_host_atrous_params(p, &q) != RT_OK) return RT_ERR_ARG;

    const size_t px = (size_t)w * (size_t)h;
    std::vector<float> other(q.levels > 0 ? 4 * px : 0), n(px);
    std::vector<uint32_t> id(px);
    std::vector<unsigned char> usable(px);
    // the levels alternate between the two planes and end in the caller's
    float *cur = q.levels % 2 == 0 ? out_rgbv : other.data(), *nxt = q.levels % 2 == 0 ? other.data() : out_rgbv;
    // 20. usability, judged on U once; C0 = U's rgb
    for (size_t at = 0; at < px; ++at) {
        const float *u = plane + (size_t)channels * at;
        n[at] = channels == 4 ? u[3] : (float)passes;
        usable[at] = rt::usable(u[0], u[1], u[2], n[at]);
        memcpy(&id[at], feat + 8 * at + 7, sizeof(uint32_t));
        memcpy(cur + 4 * at, u, 3 * sizeof(float));
    }
    // 21. the variance estimate
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t at = (size_t)y * (size_t)w + (size_t)x;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                    const size_t aq = (size_t)qy * (size_t)w + (size_t)qx;
                    if (!usable[aq] || id[aq] != id[at]) continue;
                    const float *cq = cur + 4 * aq;
                    const float l = rt::luminance(cq[0], cq[1], cq[2]);
                    s0 = s0 + 1.0f;
                    s1 = s1 + l;
                    s2 = s2 + l * l;
                }
            const float v21 = rt::variance_of_sums(s0, s1, s2);
            // 28. ... or the one the pixel's history holds
            cur[4 * at + 3] = m ? rt::variance_from_history(usable[at] != 0, m[4 * at + 2], m[4 * at + 3], k_min, v21) : v21;
        }
    // 22., 23. the levels
    const float in =1.0f / (q.k_normal * q.k_normal), kl2 = q.k_lum * q.k_lum;
    for (int level = 0; level < q.levels; ++level) {
        const int s = 1 << level;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t at = (size_t)y * (size_t)w + (size_t)x;
                const float *cp = cur + 4 * at;
                if (!usable[at]) {                                   // stays what it was and spreads nowhere
                    memcpy(nxt + 4 * at, cp, 4 * sizeof(float));
                    continue;
                }
                const float lp = rt::luminance(cp[0], cp[1], cp[2]);
                const float *np = feat + 8 * at + 3;
                float acc[3] = { 0.0f, 0.0f, 0.0f }, aw = 0.0f, av = 0.0f;
                for (int j = -2; j <= 2; ++j)
                    for (int i = -2; i <= 2; ++i) {
                        const float *cq;
                        float wgt;
                        if (i == 0 && j == 0) {
                            cq = cp;
                            wgt = rt::atrous_centre_weight(n[at]);
                        } else {
                            const long qx = (long)x + (long)s * i, qy = (long)y + (long)s * j;
                            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                            const size_t aq = (size_t)qy * (size_t)w + (size_t)qx;
                            if (!usable[aq] || id[aq] != id[at]) continue;
                            cq = cur + 4 * aq;
                            const float *nq = feat + 8 * aq + 3;
                            const float g = rt::atrous_edge(np[0], np[1], np[2], nq[0], nq[1], nq[2], in, lp, rt::luminance(cq[0], cq[1], cq[2]), cp[3], cq[3], kl2);
                            wgt = rt::atrous_tap_weight(rt::atrous_tap(j), rt::atrous_tap(i), g, n[aq]);
                        }
                        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + wgt * cq[c];
                        aw = aw + wgt;
                        av = av + (wgt * wgt) * cq[3];
                    }
                float *o = nxt + 4 * at;
                for (int c = 0; c < 3; ++c) o[c] = acc[c] / aw;
                o[3] = av / (aw * aw);
            }
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_atrous_planes(float *out_rgbv, const float *plane, int channels, int passes, const float *feat, int w, int h, const rt_atrous_params *p) {
    return atrous_loops("rt_atrous_planes", out_rgbv, plane, channels, passes, nullptr, 0.0f, feat, w, h, p);
}

int rt_atrous_moments_planes(float *out_rgbv, const float *plane, int channels, int passes, const float *m, const float *feat, int w, int h,
                             const rt_atrous_params *p, const rt_moments_params *mp) {
    rt_moments_params mq;
    if (rt_host_moments_params(mp, &mq) != RT_OK) return RT_ERR_ARG;
    return atrous_loops("rt_atrous_moments_planes", out_rgbv, plane, channels, passes, m, mq.k_min, feat, w, h, p);
}

}  // extern "C"
