// rt_denoise.hip -- denoising (include/rt_api.h, "denoising"): a non-local-means filter of a merged frame, steered by the difference of the two
// halves it was merged from (Rousselle, Knaus, Zwicker 2012) --
//   rt_denoise_async         dst's colour plane filtered on the device, the colour planes of a and b as the variance estimate
// and the kernels behind it.  rt_denoise_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 1-6, and the
// comments below name the rule a line implements.  The reference filters nothing: this is the library's own extension.
// "The error of the filtered frame" of the same header lives here too --
//   rt_denoise_pair_async    each half filtered with weights taken from the OTHER half, into planes of their own beside the colour planes
//   rt_denoise_pair_tiles_async   ... of the groups in the current selection alone (adaptive sampling's groups: rt_tiles.hip), the rest kept
//   rt_read_filtered         that plane of one context (read_plane, rt_internal.h)
// (rt_denoise_pair_planes is the host statement; rt_compare.hip compares the packed planes).
// As rt_host.cpp filters through one nlm_planes(out, img, guide, ...), the device filters through ONE body, dn_body<P, N, kAnyRow, kGuided>: N = 1 is the
// frame filtered with its own weights, N = 2 the two halves, each with the other's; kGuided adds the guide of rules 13-14 ("feature planes").  Three
// kernel templates give it an origin -- the frame, the frame's halves, a list of groups -- and ONE function launches them.
// The render kernels are not touched, and nothing here reads or writes anything but colour planes.
// This unit is compiled with -ffp-contract=off: every multiply, add and IEEE division below is an operation of its own, in the written order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include <atomic>

#include "rt_denoise.inc.h"
#include "rt_detmath.h"
#include "rt_internal.h"

using rt::fail;

extern "C" int rt_host_denoise_params(const rt_denoise_params *p, rt_denoise_params *out);     // rt_host.cpp: the parameter rules (null = defaults)


// Rules 1 and 2: one thread per float of a plane row (blockIdx.y walks the rows, so that no index is divided in 64 bits).  V = ((A - B) * 0.5)^2 is
// formed nine times per float rather than stored: the planes of a frame sit in L2, and a pass of its own over V would cost a plane's traffic more.
__global__ void __launch_bounds__(256) rt_denoise_variance_kernel(float *__restrict__ vs, const float *__restrict__ a, const float *__restrict__ b, int w, int h) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;     // float of the row: pixel f / 3, channel f % 3
    if (f >= 3u * (uint32_t)w) return;
    const int x = (int)(f / 3u), c = (int)(f - 3u * (uint32_t)x);
    for (int y = (int)blockIdx.y; y < h; y += (int)gridDim.y) {
        float sum = 0.f;
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int k = -1; k <= 1; ++k) {
                const size_t at = 3 * ((size_t)dn_clamp(y + j, h) * (size_t)w + (size_t)dn_clamp(x + k, w)) + (size_t)c;
                const float d = (a[at] - b[at]) * 0.5f;
                const float v = d * d;
                sum = (j == -1 && k == -1) ? v : sum + v;
            }
        vs[3 * ((size_t)y * (size_t)w + (size_t)x) + (size_t)c] = sum * (1.0f / 9.0f);
    }
}

// The three kernels.  kGuided (rules 13-14; rt_denoise_guided_planes / rt_denoise_pair_guided_planes are the host statements): the feature plane of the
// first half beside the colour planes, in `gd`; without it `gd` is passed empty and not touched.
// ... over the frame: the plane tiled from its row 0, a workgroup per 32x8 pixels -- the merged frame with its own weights,
template <int P, bool kGuided>
__global__ void __launch_bounds__(kPlaneLanes) rt_denoise_kernel(DnPlanes<1> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, DnGuide gd) {
    extern __shared__ float dn_lds[];
    dn_body<P, 1, false, kGuided>(dn_lds, (int)blockIdx.x * kPlaneTileW, (int)blockIdx.y * kPlaneTileH, k, vs, w, h, R, alpha, kk, gd);
}

// ... the two halves.  (waves_per_eu: at the default radii, R 5 and P 1 -- the only ones it was measured at -- LDS admits four workgroups a CU, a
// wavefront of each per SIMD.  Told so, the compiler keeps rule 3's independent divisions interleaved; left to aim for a seventh wavefront, it
// serialises them in this instance to save two registers, which measured 1.9 % slower at 1920x1080 -- profiles/HISTORY.md.  The hint bounds nothing
// at run time and the register counts are the same with it, 60 / 74 / 93.  It ALLOWS the compiler 128 registers, though: at small radii (R 1, P 0:
// nine workgroups a CU by LDS) occupancy is bound by registers, so a body that grows must be looked at again with the hint taken off.
// Looked at again for the body grown by the guide: the guided pair instances take 83 / 91 / 109 vector registers for P = 0 / 1 / 2, no scratch.  At the
// defaults, R 5 and P 1, the 58 KiB of LDS admit two workgroups a CU, a wavefront of each on every SIMD, and 91 registers would admit five; at R 8, P 2
// one workgroup fits.  Only at R 1, P 0 does LDS -- 26 KiB, six workgroups -- ask for more wavefronts than the hint's four, and that instance's 83
// registers admit six.  So the hint is kept for what it was measured to do in the unguided body, keeping rule 3's divisions interleaved, and bounds
// nothing under the guide.)
template <int P, bool kGuided>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kPlaneLanes)
rt_denoise_pair_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, DnGuide gd) {
    extern __shared__ float dn_lds[];
    dn_body<P, 2, false, kGuided>(dn_lds, (int)blockIdx.x * kPlaneTileW, (int)blockIdx.y * kPlaneTileH, k, vs, w, h, R, alpha, kk, gd);
}

// ... and the halves over the groups of a selection (rt_tiles.hip): workgroup i takes group list[i] -- g = gy * groups_x + gx in the PIXEL BUFFER's tile
// rows, row 0 at the bottom -- and covers its pixel rows 8 gy .. 8 gy + 7, which are the plane's rows h - 8 (gy + 1) .. h - 1 - 8 gy: the origin is
// negative for the top, partial, group row.  Every other pixel of the four output planes keeps its words.  A list entry that names no group is skipped
// by the whole workgroup, ahead of the first barrier.
template <int P, bool kGuided>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kPlaneLanes)
rt_denoise_pair_tiles_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, const uint32_t *__restrict__ list,
                             uint32_t groups_x, uint32_t n_groups, DnGuide gd) {
    extern __shared__ float dn_lds[];
    const uint32_t g = list[blockIdx.x];
    if (g >= n_groups) return;
    const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
    dn_body<P, 2, true, kGuided>(dn_lds, (int)gx * kPlaneTileW, h - kPlaneTileH * ((int)gy + 1), k, vs, w, h, R, alpha, kk, gd);
}

using namespace rt;

namespace {

std::atomic<uint64_t> g_pair_calls{0};                     // numbers the calls that make cross-filtered planes (FrameState::filtered_pair)

int launch_variance(float *var, const float *a, const float *b, int w, int h, hipStream_t stream) {
    hipLaunchKernelGGL(rt_denoise_variance_kernel, dim3((unsigned)((3 * (size_t)w + 255) / 256), (unsigned)std::min(h, 65535)), dim3(256), 0, stream, var, a, b, w, h);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// the guide of a pair of halves whose first is `a` (guide_refuse has passed: both hold the same setting, both feature planes are current; the plane is a's)
DnGuide guide_of(const rt_ctx *a) {
    const rt_guide_params &g = a->planes.guide_set.params;
    return DnGuide{ reinterpret_cast<const float4 *>(a->scene.d_features), 1.0f / (g.k_albedo * g.k_albedo), 1.0f / (g.k_normal * g.k_normal), 1.0f / (g.k_depth * g.k_depth) };
}

// THE launch of the filter, on c's device (selected) and in c's geometry.  N = 1: rt_denoise_async's frame; 2: the halves, over the frame or (`groups`) over a
// list of `n_selected` groups.  `guide` null: by colour alone.  Dynamic LDS beyond the 64 KiB every kernel may ask for: the limit is raised for that
// kernel on the selected device (each kernel by its symbol, as every launch of the library: the limit, then the launch).
template <int N>
int launch_filter(const rt_ctx *c, const DnPlanes<N> &k, const float *var, const rt_denoise_params &q, hipStream_t stream, const DnGuide *guide = nullptr,
                  const uint32_t *groups = nullptr, uint32_t n_selected = 0) {
    const DnGuide gd = guide ? *guide : DnGuide{};
    const size_t lds = dn_lds_bytes(N, q.search_radius, q.patch_radius, guide != nullptr);
    const dim3 grid = plane_grid(c->w, c->h);
    const float kk = q.k * q.k;
    hipError_t e = hipSuccess;
    const auto go = [&](auto kernel, dim3 blocks, auto... list) {       // (list: what the tiles kernel takes between kk and the guide)
        if (lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(kPlaneLanes), lds, stream, k, var, c->w, c->h, q.search_radius, q.alpha, kk, list..., gd);
    };
    with_patch_radius(q.patch_radius, [&](auto P) {
        constexpr int kP = decltype(P)::value;
        if constexpr (N == 1) go(guide ? rt_denoise_kernel<kP, true> : rt_denoise_kernel<kP, false>, grid);
        else if (groups)
            go(guide ? rt_denoise_pair_tiles_kernel<kP, true> : rt_denoise_pair_tiles_kernel<kP, false>, dim3(n_selected), groups, groups_per_row(c), group_count(c));
        else go(guide ? rt_denoise_pair_kernel<kP, true> : rt_denoise_pair_kernel<kP, false>, grid);
    });
    if (e != hipSuccess) return fail(RT_ERR_HIP, "the guided filter's LDS limit: %s", hipGetErrorString(e));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// two halves hold the same number of passes, and at least one
int halves_refuse(const rt_ctx *a, const rt_ctx *b, const char *call) {
    if (a->frame.current_sample != b->frame.current_sample)
        return fail(RT_ERR_STATE, "%s: the halves hold %d and %d passes", call, a->frame.current_sample, b->frame.current_sample);
    if (a->frame.current_sample <= 0) return fail(RT_ERR_STATE, "%s: the halves hold no pass", call);
    return RT_OK;
}

int check_three(const rt_ctx *dst, const rt_ctx *a, const rt_ctx *b) {
    if (!dst || !a || !b) return fail(RT_ERR_ARG, "rt_denoise_async: ctx is null");
    int rc = tiles_refuse(dst, "rt_denoise_async");
    if (rc == RT_OK) rc = tiles_refuse(a, "rt_denoise_async");
    if (rc == RT_OK) rc = tiles_refuse(b, "rt_denoise_async");
    // (no context is sharded by now: rows per tile say nothing about an unsharded frame)
    if (rc == RT_OK) rc = same_frame(a, dst, "rt_denoise_async", "the first half", "the destination", false);
    if (rc == RT_OK) rc = same_frame(b, dst, "rt_denoise_async", "the second half", "the destination", false);
    if (rc == RT_OK) rc = same_frame(a, b, "rt_denoise_async", "the first half", "the second half", false);
    return rc;
}

// The halves of a checked pair filtered on `stream`, a's device selected: over the frame, or (`tiles`) over the groups `a` has selected -- rule 2's
// plane is formed for the whole frame either way: it is bandwidth-bound and small beside the filter, and the selected groups' halos reach into groups
// that are not selected.  The list of groups is built once per selection (FrameState::group_list_built).
int filter_pair(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream, bool tiles) {
    const size_t n_floats = color_floats(a), n_words = image_pixels(a);
    for (rt_ctx *c : { a, b }) {
        RT_TRY(ensure_device(c->owned, &c->planes.filtered, n_floats));
        RT_TRY(ensure_device(c->owned, &c->planes.filtered_px, n_words));
    }
    RT_TRY(ensure_device(a->owned, &a->planes.var, n_floats));
    // behind everything the two contexts have queued; their later work behind the filter
    int rc = chain_all(stream, { a, b });
    if (rc == RT_OK && tiles && a->frame.group_list_is_stale()) rc = tiles_build_group_list(a, stream);
    if (rc == RT_OK) rc = launch_variance(a->planes.var, a->d_colors, b->d_colors, a->w, a->h, stream);
    if (rc != RT_OK) return rc;
    const Planes &pa = a->planes, &pb = b->planes;
    const DnPlanes<2> k{ { a->d_colors, b->d_colors }, { pa.filtered, pb.filtered }, { pa.filtered_px, pb.filtered_px }, { a->knobs.fast(), b->knobs.fast() } };
    const DnGuide gd = guide_of(a);
    RT_TRY(launch_filter<2>(a, k, pa.var, q, stream, pa.guide_set.on ? &gd : nullptr, tiles ? a->tiles.d_groups : nullptr, tiles ? a->frame.counts[0] : 0u));
    const uint64_t call = g_pair_calls.fetch_add(1) + 1;
    for (rt_ctx *c : { a, b }) tiles ? c->frame.pair_tiles_refreshed(call) : c->frame.pair_filtered(call);
    return RT_OK;
}

}  // namespace

namespace rt {

int denoise_pair_refuse(const rt_ctx *a, const rt_ctx *b, const char *call) {
    if (!a || !b) return fail(RT_ERR_ARG, "%s: ctx is null", call);
    int rc = tiles_refuse(a, call);
    if (rc == RT_OK) rc = tiles_refuse(b, call);
    if (rc == RT_OK) rc = same_frame(a, b, call, "the first half", "the second half", false);
    if (rc == RT_OK) rc = halves_refuse(a, b, call);
    if (rc == RT_OK) rc = guide_refuse(a, b, call);
    return rc;
}

int denoise_pair(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream) {
    const int rc = select_device(a);
    return rc != RT_OK ? rc : filter_pair(a, b, q, stream, false);
}

int denoise_pair_tiles(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream, const char *call) {
    const FrameState &fa = a->frame, &fb = b->frame;
    if (!fa.have_selection || !fb.have_selection) return fail(RT_ERR_STATE, "%s: no selection (rt_select_tiles on both contexts comes first)", call);
    if (fa.counts[0] != fb.counts[0] || fa.counts[1] != fb.counts[1])
        return fail(RT_ERR_STATE, "%s: the contexts hold selections of %u and %u groups", call, fa.counts[0], fb.counts[0]);
    if (fa.filtered_with(fb)) return RT_OK;                 // nothing has moved a colour plane since the planes were made
    if (!fa.filtered_behind_with(fb))
        return fail(RT_ERR_STATE, "%s: the cross-filtered planes are not one selection behind -- they were never made, were made by different calls, or something "
                                  "else than rt_render_tiles_async of the selection in hand has moved a colour plane since (rt_denoise_pair_async makes them whole)", call);
    if (!a->planes.filtered || !b->planes.filtered || !a->planes.filtered_px || !b->planes.filtered_px || !a->planes.var || !a->tiles.d_selected)
        return fail(RT_ERR_STATE, "%s: a plane that the frame record calls made does not exist", call);
    const int rc = select_device(a);
    if (rc != RT_OK) return rc;
    const uint32_t n_groups = group_count(a), m = fa.counts[0];
    if (m == 0 || m > n_groups) return fail(RT_ERR_STATE, "%s: a selection of %u of %u groups has been rendered", call, m, n_groups);
    return filter_pair(a, b, q, stream, true);
}

}  // namespace rt

extern "C" {

RT_API int rt_denoise_async(rt_ctx *dst, rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream) {
    int rc = check_three(dst, a, b);
    if (rc != RT_OK) return rc;
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    rc = halves_refuse(a, b, "rt_denoise_async");
    if (rc != RT_OK) return rc;
    if ((long long)dst->frame.current_sample != 2ll * a->frame.current_sample)
        return fail(RT_ERR_STATE, "rt_denoise_async: the destination holds %d passes, the halves %d each: it is not their merge", dst->frame.current_sample,
                    a->frame.current_sample);
    bool guided = false;
    rc = guide_refuse(a, b, "rt_denoise_async", &guided);
    if (rc != RT_OK) return rc;
    if (q.search_radius == 0) return RT_OK;                 // the window is the pixel itself: the image, bit for bit
    rc = select_device(dst);
    if (rc != RT_OK) return rc;
    const size_t n_floats = color_floats(dst);
    RT_TRY(ensure_device(dst->owned, &dst->planes.denoise, n_floats));
    RT_TRY(ensure_device(dst->owned, &dst->planes.var, n_floats));
    // behind everything the three contexts have queued; their later work behind the filter
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain_all(stream, { dst, a, b });
    if (rc == RT_OK) rc = launch_variance(dst->planes.var, a->d_colors, b->d_colors, dst->w, dst->h, stream);
    if (rc != RT_OK) return rc;
    const DnPlanes<1> k{ { dst->d_colors }, { dst->planes.denoise }, { nullptr }, { 0 } };      // (nothing is packed: rt_read_pixels packs the colour plane)
    const DnGuide gd = guide_of(a);                         // (the feature plane is a's)
    RT_TRY(launch_filter<1>(dst, k, dst->planes.var, q, stream, guided ? &gd : nullptr));
    std::swap(dst->d_colors, dst->planes.denoise);          // the filtered plane IS the colour plane now; the old one is the next call's scratch
    dst->frame.colours_replaced();                          // rt_read_pixels packs the filtered plane
    return RT_OK;
}

RT_API int rt_denoise_pair_async(rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream) {
    int rc = denoise_pair_refuse(a, b, "rt_denoise_pair_async");
    if (rc != RT_OK) return rc;
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    return denoise_pair(a, b, q, (hipStream_t)hip_stream);
}

RT_API int rt_denoise_pair_tiles_async(rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream) {
    int rc = denoise_pair_refuse(a, b, "rt_denoise_pair_tiles_async");
    if (rc != RT_OK) return rc;
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    return denoise_pair_tiles(a, b, q, (hipStream_t)hip_stream, "rt_denoise_pair_tiles_async");
}

RT_API int rt_read_filtered(rt_ctx *c, float *out_host) { return read_plane(c, "rt_read_filtered", Plane::Filtered, out_host); }

}  // extern "C"
