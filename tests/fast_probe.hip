// fast_probe.hip -- the inline building blocks of the path-trace kernels, one lane per input, for tests/test_gpu_fast_*.py.
//
// Built by the tests (tests/_fast_reference.py build_probe) twice from this text:
//   fast arm     -DRT_FAST=1, the flags of rt_kernel_fast.hip (-ffp-contract=fast)
//   control arm  -DRT_FAST=0, -ffp-contract=off: the parity arithmetic, which must equal the oracle / the binary32
//                restatement bit for bit -- that is what says the probe is wired correctly
// csrc/rt_trace.inc.h is included unchanged, as rt_kernel_fast.hip includes it for an instance without a render kernel;
// the kernels below CALL its inline functions.  What that holds is the source functions under the fast flags, not the
// shipped machine code: contraction depends on the surrounding code (see the docstring of tests/_fast_reference.py).
//
// Every library function that uses a wave ballot is called by ALL lanes of a wavefront: grids are whole wavefronts,
// a lane beyond the input works on the last valid record again and stores nothing.
#ifndef RT_FAST
#error "define RT_FAST to 0 or 1"
#endif
#define RT_DIAGNOSTICS 0
#define RT_NS probe
#define RT_KERNEL_NAME rt_trace_probe
#define RT_VARIANT_KERNEL 1
#define RT_NO_RENDER_KERNEL 1
#include "rt_trace.inc.h"

namespace rt {
namespace RT_NS {

RT_DEV size_t lane_index(size_t n, bool &live) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    live = i < n;
    return live ? i : n - 1;
}

// The sine and cosine a bounce or a light sample uses for the draw u, as the kernel bodies form them.
RT_DEV void sincos_of_draw(float u, float &sn, float &cs) {
#if RT_FAST
    fm_sincos_turns(u, sn, cs);
#else
    dm_sincosf_pos((2.f * RT_PI) * u, sn, cs);
#endif
}

// Scalar blocks.  a, b: inputs (b for op 4 only); r0, r1: results (r1 for ops 0 and 8).  Op 9 reads and writes triples.
extern "C" __global__ void probe_eval_kernel(int op, const float *a, const float *b, float *r0, float *r1, size_t n) {
    bool live;
    const size_t i = lane_index(n, live);
    float x = 0.f, y = 0.f, p = 0.f, q = 0.f;
    V3 v = mk(0.f, 0.f, 0.f), w = mk(0.f, 0.f, 0.f);
    if (op == 9) v = mk(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
    else x = a[i];
    if (op == 4) y = b[i];
    switch (op) {
        case 0: sincos_of_draw(x, p, q); break;
#if RT_FAST
        case 1: p = fm_powf(x, 1.f / 2.2f); break;
#else
        case 1: p = dm_powf(x, 1.f / 2.2f); break;
#endif
        case 2: p = __int_as_float(to_int(x)); break;
        case 3: p = rt_rcp(x); break;
        case 4: p = rt_div(x, y); break;
        case 5: p = rt_sqrt(x); break;
        case 6: p = rt_sqrt_unit(x); break;
        case 7: p = rt_sqrt_det(x); break;
        case 8: q = sqrt_and_rcp(x, p); break;
        case 9: w = unit(v); break;
        default: break;
    }
    if (!live) return;
    if (op == 9) {
        r0[3 * i] = w.x;
        r0[3 * i + 1] = w.y;
        r0[3 * i + 2] = w.z;
        return;
    }
    r0[i] = p;
    if (op == 0 || op == 8) r1[i] = q;
}

// Every (ray, sphere) pair: rays {o, d} (6 floats), spheres {centre, radius^2}.  out: 5 floats per pair, ray-major:
// b, det, hit_roots' t, hit_roots' hit (0 / 1), hit_post's distance.
extern "C" __global__ void probe_pairs_kernel(const float *rays, size_t n_rays, const float4 *spheres, size_t n_spheres, float *out) {
    bool live;
    const size_t k = lane_index(n_rays * n_spheres, live);
    const size_t r = k / n_spheres, s = k - r * n_spheres;
    const V3 o = mk(rays[6 * r], rays[6 * r + 1], rays[6 * r + 2]), d = mk(rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]);
    const HitPre p = hit_pre(spheres[s], o, d);
    const HitRoots h = hit_roots(p);
    const float t = hit_post(p);
    if (!live) return;
    out[5 * k] = p.b;
    out[5 * k + 1] = p.det;
    out[5 * k + 2] = h.t;
    out[5 * k + 3] = h.hit ? 1.f : 0.f;
    out[5 * k + 4] = t;
}

// The two sweeps over a table staged in LDS as the sweep kernels stage it.  rays: {o, d, max_t} (7 floats).
// out: 3 words per ray: bits of the closest distance (1e20f: none), its index, the first blocker closer than max_t (n: none).
extern "C" __global__ void probe_scene_kernel(const float *rays, size_t n_rays, const float4 *table, uint32_t n, uint32_t *out) {
    extern __shared__ float4 lds[];
    float4 *s_geom = lds;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) s_geom[i] = table[i];
    __syncthreads();
    bool live;
    const size_t r = lane_index(n_rays, live);
    const V3 o = mk(rays[7 * r], rays[7 * r + 1], rays[7 * r + 2]), d = mk(rays[7 * r + 3], rays[7 * r + 4], rays[7 * r + 5]);
    float t = 1e20f;
    uint32_t id = 0;
    unsigned long long roots = 0;
    sweep_closest(s_geom, n, o, d, t, id, roots);
    const uint32_t first = sweep_any(s_geom, n, o, d, rays[7 * r + 6], roots);
    if (!live) return;
    out[3 * r] = __float_as_uint(t);
    out[3 * r + 1] = id;
    out[3 * r + 2] = first;
}

// The continuous steps of shading that are functions of their arguments.  in: 16 words per lane, out: 12 floats per lane.
//   what 0  camera ray     in  s0, s1 (generator state), x | y << 16;  cam: o, d, x, y, 1/w, 1/h (14 floats)
//                          out rd (camera_direction), o (camera_origin), d (unit)
//   what 1  diffuse bounce in  nl[3], u, r2           out uu[3], vv[3] (basis_around), nd[3] (cosine_direction)
//   what 2  hit record     in  nrm[3], d[3]           out dp, nl[3] (facing_normal), the reflected direction d - nrm * 2 dp [3]
//   what 3  glass          in  nnt, ddn, Re           out cos2t_of, roulette_p
//   what 4  light sample   in  la[4], lb.w, s0, s1, hp[3], nl[3]     out wanted (0 / 1), sd[3], len, numer
extern "C" __global__ void probe_shade_kernel(int what, const float *in, const float *cam, float *out, size_t n) {
    bool live;
    const size_t i = lane_index(n, live);
    const float *f = in + 16 * i;
    float r[12] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (what == 0) {
        uint32_t s0 = __float_as_uint(f[0]), s1 = __float_as_uint(f[1]);
        const V3 cam_o = mk(cam[0], cam[1], cam[2]);
        const CameraArgs c = { cam_o, mk(cam[3], cam[4], cam[5]), mk(cam[6], cam[7], cam[8]), mk(cam[9], cam[10], cam[11]), cam[12], cam[13] };
        const V3 rd = camera_direction(c, __float_as_uint(f[2]), s0, s1);
        const V3 o = camera_origin(rd, cam_o);
        const V3 d = unit(rd);
        r[0] = rd.x, r[1] = rd.y, r[2] = rd.z, r[3] = o.x, r[4] = o.y, r[5] = o.z, r[6] = d.x, r[7] = d.y, r[8] = d.z;
    } else if (what == 1) {
        const float u = f[3], r2 = f[4];
        const float r2s = rt_sqrt_unit(r2);
        const Basis around = basis_around(mk(f[0], f[1], f[2]));
        float sn, cs;
        sincos_of_draw(u, sn, cs);
        const V3 nd = cosine_direction(around, sn, cs, r2s, r2);
        r[0] = around.uu.x, r[1] = around.uu.y, r[2] = around.uu.z, r[3] = around.vv.x, r[4] = around.vv.y, r[5] = around.vv.z;
        r[6] = nd.x, r[7] = nd.y, r[8] = nd.z;
    } else if (what == 2) {
        const V3 nrm = mk(f[0], f[1], f[2]), d = mk(f[3], f[4], f[5]);
        const float dp = dot(nrm, d);
        const V3 nl = facing_normal(nrm, dp);
        const V3 rfl = sub(d, scale(nrm, 2.f * dp));
        r[0] = dp, r[1] = nl.x, r[2] = nl.y, r[3] = nl.z, r[4] = rfl.x, r[5] = rfl.y, r[6] = rfl.z;
    } else if (what == 3) {
        r[0] = cos2t_of(f[0], f[1]);
        r[1] = roulette_p(f[2]);
    } else {
        uint32_t s0 = __float_as_uint(f[5]), s1 = __float_as_uint(f[6]), draws = 0;
        V3 sd = mk(0.f, 0.f, 0.f);
        float len = 0.f, numer = 0.f;
        const bool want = sample_light(make_float4(f[0], f[1], f[2], f[3]), make_float4(0.f, 0.f, 0.f, f[4]), s0, s1, draws,
                                       mk(f[7], f[8], f[9]), mk(f[10], f[11], f[12]), sd, len, numer);
        r[0] = want ? 1.f : 0.f, r[1] = sd.x, r[2] = sd.y, r[3] = sd.z, r[4] = len, r[5] = numer;
    }
    if (!live) return;
    for (int k = 0; k < 12; ++k) out[12 * i + k] = r[k];
}

}  // namespace RT_NS
}  // namespace rt

// ---- C entry points: allocate, copy, launch, synchronise, free.  0 on success, a hipError_t otherwise. ----------
namespace {

struct DeviceBuffer {
    void *p = nullptr;
    hipError_t e = hipSuccess;
    DeviceBuffer(const void *host, size_t bytes) {
        if (bytes == 0) bytes = 4;
        e = hipMalloc(&p, bytes);
        if (e == hipSuccess && host) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && !host) e = hipMemset(p, 0, bytes);
    }
    ~DeviceBuffer() {
        if (p) (void)hipFree(p);
    }
    hipError_t back(void *host, size_t bytes) const { return hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost); }
};

unsigned blocks_of(size_t lanes) { return (unsigned)((lanes + 255) / 256); }

hipError_t finish() {
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipDeviceSynchronize();
}

}  // namespace

#define PROBE_TRY(x)                       \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)
#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int probe_is_fast(void) { return RT_FAST; }

PROBE_API int probe_eval(int op, const float *a, const float *b, float *r0, float *r1, size_t n) {
    if (n == 0 || op < 0 || op > 9) return -1;
    const size_t w = op == 9 ? 3 : 1;
    DeviceBuffer da(a, w * n * 4), db(op == 4 ? b : nullptr, n * 4), d0(nullptr, w * n * 4), d1(nullptr, n * 4);
    PROBE_TRY(da.e); PROBE_TRY(db.e); PROBE_TRY(d0.e); PROBE_TRY(d1.e);
    hipLaunchKernelGGL(rt::probe::probe_eval_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, op, (const float *)da.p, (const float *)db.p,
                       (float *)d0.p, (float *)d1.p, n);
    PROBE_TRY(finish());
    PROBE_TRY(d0.back(r0, w * n * 4));
    if (op == 0 || op == 8) PROBE_TRY(d1.back(r1, n * 4));
    return 0;
}

PROBE_API int probe_pairs(const float *rays, size_t n_rays, const float *spheres, size_t n_spheres, float *out) {
    if (n_rays == 0 || n_spheres == 0) return -1;
    const size_t pairs = n_rays * n_spheres;
    DeviceBuffer dr(rays, n_rays * 24), ds(spheres, n_spheres * 16), dout(nullptr, pairs * 20);
    PROBE_TRY(dr.e); PROBE_TRY(ds.e); PROBE_TRY(dout.e);
    hipLaunchKernelGGL(rt::probe::probe_pairs_kernel, dim3(blocks_of(pairs)), dim3(256), 0, 0, (const float *)dr.p, n_rays,
                       (const float4 *)ds.p, n_spheres, (float *)dout.p);
    PROBE_TRY(finish());
    PROBE_TRY(dout.back(out, pairs * 20));
    return 0;
}

PROBE_API int probe_scene(const float *rays, size_t n_rays, const float *table, unsigned n, unsigned *out) {
    if (n_rays == 0 || n == 0 || n > 2048) return -1;            // (2048 records = 32 KB of LDS, below the 64 KB a launch gets by default)
    DeviceBuffer dr(rays, n_rays * 28), dt(table, (size_t)n * 16), dout(nullptr, n_rays * 12);
    PROBE_TRY(dr.e); PROBE_TRY(dt.e); PROBE_TRY(dout.e);
    hipLaunchKernelGGL(rt::probe::probe_scene_kernel, dim3(blocks_of(n_rays)), dim3(256), (size_t)n * 16, 0, (const float *)dr.p, n_rays,
                       (const float4 *)dt.p, n, (uint32_t *)dout.p);
    PROBE_TRY(finish());
    PROBE_TRY(dout.back(out, n_rays * 12));
    return 0;
}

PROBE_API int probe_shade(int what, const float *in, const float *cam, float *out, size_t n) {
    if (n == 0 || what < 0 || what > 4) return -1;
    const float no_cam[14] = { 0 };
    DeviceBuffer di(in, n * 64), dc(cam ? cam : no_cam, 56), dout(nullptr, n * 48);
    PROBE_TRY(di.e); PROBE_TRY(dc.e); PROBE_TRY(dout.e);
    hipLaunchKernelGGL(rt::probe::probe_shade_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, what, (const float *)di.p, (const float *)dc.p,
                       (float *)dout.p, n);
    PROBE_TRY(finish());
    PROBE_TRY(dout.back(out, n * 48));
    return 0;
}
