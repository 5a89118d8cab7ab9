// rt_features.hip -- feature planes from camera rays (include/rt_api.h, "feature planes"): what lies under every pixel --
//   rt_features_async        albedo, normal, distance and scene index of the pixel-centre ray's first hit, into a plane the context owns
//   rt_read_features         that plane (read_plane, rt_internal.h)
//   rt_set_denoise_guide     the per-context setting that lets the filters of rt_denoise.hip restrict their weights by it
// and the kernel behind the first.  rt_features_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 10-12, and
// the comments below name the rule a line implements.  The reference hands out no such plane: this is the library's own extension.
// This unit is compiled with parity's flags (-ffp-contract=off, correctly rounded division and square root): every multiply, add, division and square
// root below is an operation of its own, in the written order -- whatever rt_set_mode says.
// Two ways to the same words (rt_instance.h features_form says which a call takes; rt_last_features_kernel names it): the PLAIN SWEEP below, pixels x
// records tests, whose answer is the reference's Intersect by construction -- scenes without a hierarchy, or of fewer than kFeaturesWalkMin records --
// and ONE closest-hit query per pixel THROUGH THE HIERARCHY (rt_walk.inc.h rt_features_pairs / _pairs_m / _pairs_g, parity's unit), which an interactive
// host that forms the plane every frame needs on large scenes.  The hierarchy only selects candidates: every test made is the same arithmetic.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_internal.h"
#include "rt_plane.inc.h"

using rt::fail;

extern "C" int rt_host_guide_params(const rt_guide_params *g);     // rt_host.cpp: the guide's parameter rules

namespace {

constexpr uint32_t kFtChunk = 1024;                                             // records staged at a time: 16 KiB of LDS

}  // namespace

// One lane per pixel.  The geometry table {centre, radius^2} (rt_scene.hip: the reference's own rad * rad) goes through LDS in chunks of kFtChunk
// records, a barrier either side of a chunk's tests, and is read back at wave-uniform addresses.  EVERY lane stays in the chunk loop until its last
// barrier -- a lane outside the image traces the ray of a pixel that does not exist and stores nothing.
// Bounds: a chunk stages records [base, min(base + kFtChunk, n)) of a table of n and tests exactly those; the hit's records are read at id < n; the
// store is guarded by x < w && y < h.
__global__ void __launch_bounds__(kPlaneLanes) rt_features_kernel(float4 *__restrict__ out, const float4 *__restrict__ geom, const float4 *__restrict__ emis,
                                                                  const float4 *__restrict__ colr, uint32_t n, rt::PixelCamera cam, int w, int h) {
    __shared__ float4 s_geom[kFtChunk];
    const int tid = (int)threadIdx.x;
    const auto [x, y] = plane_pixel();

    // rule 10: the ray through the pixel's centre
    const rt::PixelRay r = rt::pixel_ray(cam, x, y, 1.f / (float)w, 1.f / (float)h);

    // rule 11: the nearest record in scene order
    float t = 1e20f;
    uint32_t id = 0xFFFFFFFFu;
    for (uint32_t base = 0; base < n; base += kFtChunk) {
        const uint32_t m = min(kFtChunk, n - base);
        for (uint32_t i = (uint32_t)tid; i < m; i += (uint32_t)kPlaneLanes) s_geom[i] = geom[base + i];
        __syncthreads();
        for (uint32_t i = 0; i < m; ++i) {
            const float4 g = s_geom[i];
            const float dist = rt::sphere_distance(g.x, g.y, g.z, g.w, r);
            if (dist != 0.f && dist < t) {
                t = dist;
                id = base + i;
            }
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;

    // rule 12: the values
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (t < 1e20f) {
        const float4 g = geom[id], e = emis[id], c = colr[id];
        const rt::Float3 nrm = rt::hit_normal(r, t, g.x, g.y, g.z);
        lo = make_float4(c.x + e.x, c.y + e.y, c.z + e.z, nrm.x);
        hi = make_float4(nrm.y, nrm.z, t, __uint_as_float(id));
    }
    const size_t at = (size_t)(h - 1 - y) * (size_t)w + (size_t)x;
    out[2 * at] = lo;
    out[2 * at + 1] = hi;
}

namespace rt {

int features_refuse(const rt_ctx *c, const char *call, const char *lead, const char *of_whom) {
    if (features_current(c)) return RT_OK;
    return fail(RT_ERR_STATE, "%s: %sthe feature plane%s is not current (rt_features_async forms it; rt_set_scene, rt_update_spheres_async and rt_set_camera end it)", call,
                lead, of_whom);
}

int guide_refuse(const rt_ctx *a, const rt_ctx *b, const char *call, bool *guided) {
    if (guided) *guided = false;
    const auto &ga = a->planes.guide_set, &gb = b->planes.guide_set;
    if (ga.on != gb.on || (ga.on && memcmp(&ga.params, &gb.params, sizeof ga.params) != 0))
        return fail(RT_ERR_STATE, "%s: the halves differ in their guide (rt_set_denoise_guide: both off, or both on with the same parameters)", call);
    if (!ga.on) return RT_OK;
    // (a plane is current only after rt_features_async has acquired its block: SceneState::features_formed)
    RT_TRY(features_refuse(a, call, "a guide is set and ", " of the first half"));
    RT_TRY(features_refuse(b, call, "a guide is set and ", " of the second half"));
    if (guided) *guided = true;
    return RT_OK;
}

}  // namespace rt

using namespace rt;

extern "C" {

RT_API int rt_features_async(rt_ctx *c, void *hip_stream) {
    int rc = tiles_refuse(c, "rt_features_async");
    if (rc != RT_OK) return rc;
    if (!c->scene.state.renderable()) return fail(RT_ERR_STATE, "rt_features_async: rt_set_scene and rt_set_camera come first");
    // (the hierarchy forced on a scene that has none: refused here, before anything is queued, where the tables say so already; a scene whose
    // tables an update left stale is asked again behind their rebuild, below)
    const char *no_hierarchy = "rt_features_async: the hierarchy is forced (rt_debug_set_features_form) and the scene has none (fewer than %d small spheres?)";
    if (c->knobs.features_form == 2 && !c->scene.state.needs_refresh() && !c->scene.state.has_hierarchy()) return fail(RT_ERR_STATE, no_hierarchy, c->knobs.bvh_min);
    rc = select_device(c);
    if (rc != RT_OK) return rc;
    RT_TRY(ensure_device(c->owned, &c->scene.d_features, 8 * image_pixels(c)));
    // behind everything the context has queued; the tables from the records as they are now
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(c, stream);
    if (rc == RT_OK) rc = refresh_tables(c, stream);
    if (rc != RT_OK) return rc;
    // which kernel: the rule, of the scene as the refresh left it
    const SceneFacts facts = scene_facts(c);
    const int form = features_form(c->knobs, facts);
    if (c->knobs.features_form == 2 && !features_walks(form)) return fail(RT_ERR_STATE, no_hierarchy, c->knobs.bvh_min);
    if (features_walks(form)) {
        const FeaturesWalkParams p{ reinterpret_cast<float4 *>(c->scene.d_features), c->scene.tables.geom, c->scene.tables.emis, c->scene.tables.colr, c->scene.bvh,
                                    pixel_camera(c->cam), c->w, c->h };
        const size_t lds = features_lds(form, facts);
        if (lds > kLdsMax) return fail(RT_ERR_ARG, "rt_features_async: %s needs %zu B of LDS for this scene (limit %zu)", features_walk_name(form), lds, kLdsMax);
        HIP_TRY(launch_features_walk(form, p, plane_grid(c->w, c->h), lds, stream));
        c->last_features_kernel = features_walk_name(form);
    } else {
        hipLaunchKernelGGL(rt_features_kernel, plane_grid(c->w, c->h), dim3(kPlaneLanes), 0, stream, reinterpret_cast<float4 *>(c->scene.d_features), c->scene.tables.geom,
                           c->scene.tables.emis, c->scene.tables.colr, c->scene.tables.n_spheres, pixel_camera(c->cam), c->w, c->h);
        HIP_TRY(hipGetLastError());
        c->last_features_kernel = "rt_features_kernel";
    }
    if (!c->scene.state.features_current) c->frame.features_reformed();     // (a temporal plane formed under the plane that ended stays ended)
    c->scene.state.features_formed();
    return RT_OK;
}

RT_API const char *rt_last_features_kernel(const rt_ctx *c) { return c ? c->last_features_kernel : ""; }

RT_API int rt_read_features(rt_ctx *c, float *out_host) { return read_plane(c, "rt_read_features", Plane::Features, out_host); }

RT_API int rt_set_denoise_guide(rt_ctx *c, const rt_guide_params *g) {
    RT_TRY(tiles_refuse(c, "rt_set_denoise_guide"));
    if (g && rt_host_guide_params(g) != RT_OK) return RT_ERR_ARG;
    c->planes.guide_set = { g ? *g : rt_guide_params{}, g != nullptr };
    return RT_OK;
}

}  // extern "C"
