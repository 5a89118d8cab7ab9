// walk_probe.hip -- the hierarchy walk's own rays kernel (csrc/rt_walk.inc.h, the kernel behind rt_debug_walk_rays: arbitrary rays
// through the walk AND through the plain sweep, one lane per ray) built under the FAST flags, for tests/test_gpu_fast_walk.py.
//
// The library instantiates that kernel once, in the diagnostics build and with parity's flags (rt_walk_rays_parity); the derivation of
// the walk's pad is written for parity's roundings.  Here the same text -- csrc/rt_trace.inc.h and rt_walk.inc.h included unchanged, as
// rt_kernel_parity.hip includes them for its pairs instance -- is built twice by tests/_fast_reference.py build_probe:
//   fast arm     -DRT_FAST=1, the flags of rt_kernel_fast.hip (-ffp-contract=fast)
//   control arm  -DRT_FAST=0, -ffp-contract=off: must equal rt_debug_walk_rays of the diagnostics library bit for bit on the same
//                tables -- that is what says the probe is wired correctly
// The host entry fills LaunchParams from the table {centre, radius^2} of the scene and the hierarchy's blob and counts as the diagnostics
// library hands them out (rt_debug_read_bvh); the LDS size is the one rt_debug_walk_rays computes.  The instantiation also carries the
// walk's render kernel (rt_trace_walk_probe), which nothing launches.
#ifndef RT_FAST
#error "define RT_FAST to 0 or 1"
#endif
#define RT_DIAGNOSTICS 1
#define RT_NS walk_probe
#define RT_KERNEL_NAME rt_trace_walk_probe
#define RT_WALK_RAYS_KERNEL_NAME rt_walk_rays_probe
#define RT_VARIANT_KERNEL 1
#define RT_OPT_WALK 1
#define RT_OPT_MINWAVES 5
#include "rt_trace.inc.h"

namespace {

struct DeviceBuffer {
    void *p = nullptr;
    hipError_t e = hipSuccess;
    DeviceBuffer(const void *host, size_t bytes, size_t spare = 0) {
        e = hipMalloc(&p, bytes + spare + 16);
        if (e == hipSuccess) e = hipMemset(p, 0, bytes + spare + 16);
        if (e == hipSuccess && host) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    }
    ~DeviceBuffer() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

#define PROBE_TRY(x)                       \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)
#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int walk_probe_is_fast(void) { return RT_FAST; }

// table: n records {centre, radius^2}; blob: the hierarchy's blob, blob_float4 float4s; rays8[i] = { o.xyz, t_max, d.xyz, bits(shadow) };
// out4[i] as rt_debug_walk_rays: the walk's answer, then the sweep's.  0 on success, a hipError_t, or -1 (arguments) / -2 (LDS).
PROBE_API int walk_probe_rays(const float *table, unsigned n, const float *blob, size_t blob_float4, unsigned n_always, unsigned n_leaves,
                              unsigned stack_depth, const float *rays8, unsigned n_rays, unsigned *out4) {
    if (!table || !blob || !rays8 || !out4 || n == 0 || n_rays == 0 || n_leaves == 0 || stack_depth == 0) return -1;
    const unsigned n_slots = n_always + (unsigned)rt::kBvhLeaf * n_leaves;
    if (blob_float4 < rt::bvh_blob_float4s(n_leaves, n_slots)) return -1;
    const size_t lds = rt::lds_bytes_pairs(0, 0, false, 0, n_leaves, n_slots, stack_depth, 256);
    if (lds > 152 * 1024) return -2;
    DeviceBuffer d_table(table, (size_t)n * 16), d_blob(blob, blob_float4 * 16), d_rays(rays8, (size_t)n_rays * 32, 32), d_out(nullptr, (size_t)n_rays * 16);
    PROBE_TRY(d_table.e); PROBE_TRY(d_blob.e); PROBE_TRY(d_rays.e); PROBE_TRY(d_out.e);
    rt::LaunchParams p{};
    p.scene.geom = (const float4 *)d_table.p;
    p.scene.n_spheres = n;
    p.bvh.blob = (const float4 *)d_blob.p;
    p.bvh.n_always = n_always;
    p.bvh.n_leaves = n_leaves;
    p.bvh.n_slots = n_slots;
    p.bvh.stack_depth = stack_depth;
    p.bvh.emis_at = rt::bvh_emis_at(n_leaves, n_slots);
    PROBE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(rt::walk_probe::rt_walk_rays_probe), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    const unsigned blocks = (n_rays + 255) / 256 < 512 ? (n_rays + 255) / 256 : 512;
    hipLaunchKernelGGL(rt::walk_probe::rt_walk_rays_probe, dim3(blocks), dim3(256), lds, 0, p, (const float4 *)d_rays.p, n_rays, (uint4 *)d_out.p);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out4, d_out.p, (size_t)n_rays * 16, hipMemcpyDeviceToHost));
    return 0;
}
