// rt_denoise_guided.hip -- the filter kernels of rt_denoise.hip under a guide (include/rt_api.h, "feature planes", rules 13-14): the same body,
// dn_body<P, N, kAnyRow, true>, with the feature plane of the first half beside the colour planes, and the one function that launches them.  A unit of
// its own: the unguided kernels' code object stays what it was.  rt_denoise_guided_planes / rt_denoise_pair_guided_planes (rt_host.cpp) are the host
// statements.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "rt_denoise.inc.h"

using rt::fail;

// The three kernels of rt_denoise.hip under a guide: the same origins, the feature plane beside the colour planes.  (waves_per_eu, looked at again for the
// grown body: the pair instances take 83 / 91 / 109 vector registers for P = 0 / 1 / 2, no scratch.  At the defaults, R 5 and P 1, the 58 KiB of LDS admit two
// workgroups a CU, a wavefront of each on every SIMD, and 91 registers would admit five; at R 8, P 2 one workgroup fits.  Only at R 1, P 0 does LDS -- 26 KiB,
// six workgroups -- ask for more wavefronts than the hint's four, and that instance's 83 registers admit six.  So the hint is kept for what it was measured
// to do in the unguided body, keeping rule 3's divisions interleaved, and bounds nothing here.)
template <int P>
__global__ void __launch_bounds__(kPlaneLanes) rt_denoise_guided_kernel(DnPlanes<1> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, DnGuide gd) {
    extern __shared__ float dn_lds[];
    dn_body<P, 1, false, true>(dn_lds, (int)blockIdx.x * kPlaneTileW, (int)blockIdx.y * kPlaneTileH, k, vs, w, h, R, alpha, kk, gd);
}

template <int P>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kPlaneLanes)
rt_denoise_pair_guided_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, DnGuide gd) {
    extern __shared__ float dn_lds[];
    dn_body<P, 2, false, true>(dn_lds, (int)blockIdx.x * kPlaneTileW, (int)blockIdx.y * kPlaneTileH, k, vs, w, h, R, alpha, kk, gd);
}

template <int P>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kPlaneLanes)
rt_denoise_pair_tiles_guided_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, const uint32_t *__restrict__ list,
                                    uint32_t groups_x, uint32_t n_groups, DnGuide gd) {
    extern __shared__ float dn_lds[];
    const uint32_t g = list[blockIdx.x];
    if (g >= n_groups) return;
    const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
    dn_body<P, 2, true, true>(dn_lds, (int)gx * kPlaneTileW, h - kPlaneTileH * ((int)gy + 1), k, vs, w, h, R, alpha, kk, gd);
}

namespace rt {

// `n_images` = 1: rt_denoise_async's frame; 2: the halves, over the frame or (f.groups) over a list of groups.  The guide and the feature plane are `a`'s.
// Dynamic LDS beyond the 64 KiB every kernel may ask for: the limit is raised for that kernel on the selected device.
int launch_guided_filter(int n_images, const GuidedFilter &f, const rt_ctx *a, const rt_denoise_params &q, hipStream_t stream) {
    const rt_guide_params &g = a->planes.guide_set.params;
    const DnGuide gd{ reinterpret_cast<const float4 *>(a->scene.d_features), 1.0f / (g.k_albedo * g.k_albedo), 1.0f / (g.k_normal * g.k_normal), 1.0f / (g.k_depth * g.k_depth) };
    const size_t lds = dn_lds_bytes(n_images, q.search_radius, q.patch_radius, true);
    const dim3 grid = plane_grid(a->w, a->h);
    const float kk = q.k * q.k;
    hipError_t e = hipSuccess;
    // (each kernel by its symbol, as every launch of the library: the limit, then the launch)
#define DN_LAUNCH_GUIDED(kernel, blocks, ...)                                                                                                        \
    do {                                                                                                                                             \
        if (lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax); \
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(kPlaneLanes), lds, stream, __VA_ARGS__);                                           \
    } while (0)
    with_patch_radius(q.patch_radius, [&](auto P) {
        constexpr int kP = decltype(P)::value;
        if (n_images == 1) {
            const DnPlanes<1> k{ { f.img[0] }, { f.out[0] }, { nullptr }, { 0 } };
            DN_LAUNCH_GUIDED(rt_denoise_guided_kernel<kP>, grid, k, f.var, a->w, a->h, q.search_radius, q.alpha, kk, gd);
        } else {
            const DnPlanes<2> k{ { f.img[0], f.img[1] }, { f.out[0], f.out[1] }, { f.px[0], f.px[1] }, { f.fast[0], f.fast[1] } };
            if (f.groups)
                DN_LAUNCH_GUIDED(rt_denoise_pair_tiles_guided_kernel<kP>, dim3(f.n_selected), k, f.var, a->w, a->h, q.search_radius, q.alpha, kk, f.groups,
                                 groups_per_row(a), group_count(a), gd);
            else
                DN_LAUNCH_GUIDED(rt_denoise_pair_guided_kernel<kP>, grid, k, f.var, a->w, a->h, q.search_radius, q.alpha, kk, gd);
        }
    });
#undef DN_LAUNCH_GUIDED
    if (e != hipSuccess) return fail(RT_ERR_HIP, "the guided filter's LDS limit: %s", hipGetErrorString(e));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // namespace rt
