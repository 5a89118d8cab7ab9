#include "rt_api.h"
#include <cstdio>
#include <vector>
extern "C" void rt_host_set_error(const char *msg) { fprintf(stderr, "err: %s\n", msg); }
int main() {
    std::vector<rt_sphere> s(64);
    uint32_t n = 0; rt_vec3 o, t;
    for (const char *p : { "/tmp/rt_san/a.scn", "/tmp/rt_san/bad1.scn", "/tmp/rt_san/bad2.scn", "/tmp/rt_san/none.scn" }) {
        int rc = rt_read_scene(p, s.data(), 64, &n, &o, &t, 1);
        printf("%s rc %d n %u\n", p, rc, n);
        rc = rt_read_scene(p, s.data(), 3, &n, &o, &t, 0);
        printf("  small cap rc %d n %u\n", rc, n);
    }
    std::vector<uint32_t> seeds(100000);
    rt_default_seeds(seeds.data(), seeds.size());
    rt_default_seeds(seeds.data(), 10);
    rt_camera c{}; c.orig = {20, 100, 120}; c.target = {0, 25, 0};
    rt_compute_camera(&c, 800, 600);
    rt_sphere d[6]; printf("demo %d %d\n", rt_demo_scene(d, 6), rt_demo_scene(d, 2));
    printf("seed0 %u cam %g\n", seeds[0], c.x.x);
    // temporal reprojection's host statement on planes of exactly the sizes it may touch: the Demo scene from two origins at sizes with partial
    // tiles and 1x1, the source with 3 and with 4 floats a texel, the destination with and without a pass (a null colour plane)
    for (int size = 0; size < 3; ++size) {
        const int w = size == 0 ? 41 : size == 1 ? 70 : 1, h = size == 0 ? 23 : size == 1 ? 19 : 1;
        rt_camera cs{}, cd{};
        cs.orig = {20, 100, 120}; cs.target = {0, 25, 0};
        cd.orig = {23, 100, 119}; cd.target = {0, 25, 0};
        rt_compute_camera(&cs, w, h);
        rt_compute_camera(&cd, w, h);
        const size_t px = (size_t)w * h;
        std::vector<float> fs(8 * px), fd(8 * px), u3(3 * px, 0.5f), u4(4 * px, 2.0f), cdp(3 * px, 0.25f), out(4 * px);
        rt_features_planes(fs.data(), d, 6, &cs, w, h);
        rt_features_planes(fd.data(), d, 6, &cd, w, h);
        int ok = 0;
        for (int ch = 3; ch <= 4; ++ch)
            for (int nd = 0; nd <= 2; nd += 2) {
                const rt_reproject_view dst{ nd ? cdp.data() : nullptr, 3, nd, fd.data(), &cd, d };
                const rt_reproject_view src{ ch == 3 ? u3.data() : u4.data(), ch, 16, fs.data(), &cs, d };
                ok += rt_reproject_planes(out.data(), &dst, &src, 6, w, h, nullptr) == RT_OK;
            }
        printf("reproject %dx%d: %d of 4 ok, n %g\n", w, h, ok, out[3]);
        // the wavelet filter's host statement on the same planes: five levels put steps 8 and 16 beyond all three sizes in one direction or both
        rt_atrous_params at;
        rt_atrous_defaults(&at);
        at.levels = 5;
        int filtered = 0;
        filtered += rt_atrous_planes(out.data(), u3.data(), 3, 16, fd.data(), w, h, &at) == RT_OK;
        filtered += rt_atrous_planes(out.data(), u4.data(), 4, 0, fd.data(), w, h, &at) == RT_OK;
        printf("atrous %dx%d: %d of 2 ok, v %g\n", w, h, filtered, out[3]);
        // the temporal moments' host statements on the same planes (all three sizes are odd one way or both): a first frame from the luminance of a
        // 3-float source, a second from that frame's moments plane with the cap running (max_history 3 < 16), a pure warp; then the filter with rule 28
        // on both sides of k_min, and without a moments plane
        {
            std::vector<float> t1(4 * px), m1(4 * px), t2(4 * px), m2(4 * px);
            rt_reproject_params rp;
            rt_reproject_defaults(&rp);
            rp.max_history = 3.0f;
            rt_moments_params mp;
            rt_moments_defaults(&mp);
            mp.k_min = 2.0f;
            const rt_reproject_view dst{ cdp.data(), 3, 2, fd.data(), &cd, d }, dst0{ nullptr, 3, 0, fd.data(), &cd, d };
            const rt_reproject_view src3{ u3.data(), 3, 16, fs.data(), &cs, d }, src4{ t1.data(), 4, 0, fd.data(), &cd, d };
            int moments = 0;
            moments += rt_reproject_moments_planes(t1.data(), m1.data(), &dst, &src3, nullptr, 6, w, h, &rp) == RT_OK;
            moments += rt_reproject_moments_planes(t2.data(), m2.data(), &dst, &src4, m1.data(), 6, w, h, &rp) == RT_OK;
            moments += rt_reproject_moments_planes(out.data(), m1.data(), &dst0, &src4, m2.data(), 6, w, h, nullptr) == RT_OK;
            moments += rt_atrous_moments_planes(out.data(), t2.data(), 4, 0, m2.data(), fd.data(), w, h, &at, &mp) == RT_OK;
            moments += rt_atrous_moments_planes(out.data(), u3.data(), 3, 16, m2.data(), fd.data(), w, h, nullptr, nullptr) == RT_OK;
            moments += rt_atrous_moments_planes(out.data(), t2.data(), 4, 0, nullptr, fd.data(), w, h, &at, &mp) == RT_OK;
            printf("moments %dx%d: %d of 6 ok, k %g v %g\n", w, h, moments, m2[2], m2[3]);
        }
        // shadow-aware history's host statement on the same planes: record 3 moved (one pair), then the light moved too (every record pairs with it),
        // with and without a moments plane and a flag plane, keep 0 and the default, a pure warp; and the pair list, counted and filled short
        {
            rt_sphere moved[6];
            for (int i = 0; i < 6; ++i) moved[i] = d[i];
            moved[3].p.x += 7.0f;
            std::vector<float> t1(4 * px), m1(4 * px);
            std::vector<uint8_t> k(px);
            rt_shadow_history_params sp;
            rt_shadow_history_defaults(&sp);
            const rt_reproject_view src3{ u3.data(), 3, 16, fs.data(), &cs, d }, src4{ u4.data(), 4, 0, fs.data(), &cs, d };
            int shadow = 0, flagged = 0;
            for (int lights = 0; lights <= 1; ++lights) {
                if (lights) moved[5].p.z -= 4.0f;
                std::vector<float> fm(8 * px);
                rt_features_planes(fm.data(), moved, 6, &cd, w, h);
                const rt_reproject_view dst{ cdp.data(), 3, 2, fm.data(), &cd, moved }, dst0{ nullptr, 3, 0, fm.data(), &cd, moved };
                shadow += rt_reproject_shadow_planes(t1.data(), m1.data(), k.data(), &dst, &src3, nullptr, 6, w, h, nullptr, &sp) == RT_OK;
                for (uint8_t v : k) flagged += v;
                sp.keep = 0.0f;
                shadow += rt_reproject_shadow_planes(t1.data(), nullptr, k.data(), &dst, &src4, nullptr, 6, w, h, nullptr, &sp) == RT_OK;
                shadow += rt_reproject_shadow_planes(t1.data(), m1.data(), nullptr, &dst, &src4, u4.data(), 6, w, h, nullptr, &sp) == RT_OK;
                shadow += rt_reproject_shadow_planes(t1.data(), nullptr, k.data(), &dst0, &src3, nullptr, 6, w, h, nullptr, nullptr) == RT_OK;
                uint32_t lj[4];
                shadow += rt_shadow_history_pairs(d, moved, 6, lj, 2) == (lights ? 5 : 1);
                shadow += rt_shadow_history_pairs(d, moved, 6, nullptr, 0) == (lights ? 5 : 1);
            }
            printf("shadow history %dx%d: %d of 12 ok, %d flagged\n", w, h, shadow, flagged);
        }
        // the NL-means host statements on halves of the same sizes, with and without the guide (the feature plane above), search radius 0 and 2, patch
        // radius 0 and 2: with the calls above, every function of rt_rules.h has run
        std::vector<float> ha(3 * px), hb(3 * px), merged(3 * px), fa(3 * px), fb(3 * px);
        for (size_t i = 0; i < 3 * px; ++i) {
            ha[i] = 0.25f + 0.001f * (float)(i % 97);
            hb[i] = 0.30f - 0.002f * (float)(i % 53);
            merged[i] = (ha[i] + hb[i]) * 0.5f;
        }
        rt_guide_params gp;
        rt_guide_defaults(&gp);
        int denoised = 0;
        for (int guided = 0; guided <= 1; ++guided)
            for (int R = 0; R <= 2; R += 2)
                for (int P = 0; P <= 2; P += 2) {
                    rt_denoise_params dp;
                    rt_denoise_defaults(&dp);
                    dp.search_radius = R;
                    dp.patch_radius = P;
                    denoised += rt_denoise_guided_planes(fa.data(), merged.data(), ha.data(), hb.data(), guided ? fd.data() : nullptr, w, h, &dp, guided ? &gp : nullptr) == RT_OK;
                    denoised += rt_denoise_pair_guided_planes(fa.data(), fb.data(), ha.data(), hb.data(), guided ? fd.data() : nullptr, w, h, &dp, guided ? &gp : nullptr) == RT_OK;
                }
        printf("denoise %dx%d: %d of 16 ok, f %g\n", w, h, denoised, fa[0]);
    }
}
