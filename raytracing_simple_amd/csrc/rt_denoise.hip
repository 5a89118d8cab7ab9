// rt_denoise.hip -- denoising (include/rt_api.h, "denoising"): a non-local-means filter of a merged frame, steered by the difference of the two
// halves it was merged from (Rousselle, Knaus, Zwicker 2012) --
//   rt_denoise_async         dst's colour plane filtered on the device, the colour planes of a and b as the variance estimate
// and the two kernels behind it.  rt_denoise_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 1-6, and the
// comments below name the rule a line implements.  The reference filters nothing: this is the library's own extension.
// The render kernels are not touched, and nothing here reads or writes anything but colour planes.
// This unit is compiled with -ffp-contract=off: every multiply, add and IEEE division below is an operation of its own, in the written order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "rt_internal.h"

using rt::fail;

extern "C" int rt_host_denoise_params(const rt_denoise_params *p, rt_denoise_params *out);     // rt_host.cpp: the parameter rules (null = defaults)

namespace {

constexpr int kDnTileW = 32, kDnTileH = 8, kDnLanes = kDnTileW * kDnTileH;      // a workgroup's output pixels: four wavefronts, a row of 32 per half-wave

__device__ __forceinline__ int dn_clamp(int v, int n) { return min(max(v, 0), n - 1); }

}  // namespace

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

// Rules 3 to 6.  A workgroup owns the 32x8 output pixels at (x0, y0); H = R + P.
//   LDS: six planes (D and Vs, three channels each) of LW x LH = (32 + 2H) x (8 + 2H) floats, entry (ly, lx) = the plane at cl(y0 - H + ly, x0 - H + lx) --
//   one float per lane and read, consecutive lanes on consecutive banks -- then two buffers of EW x EH = (32 + 2P) x (8 + 2P) floats for e(., o).
//   Per offset o: every lane forms e(x, o) for its one or two positions x of the tile and its P-halo (x = the CLAMPED position, its partner cl(x + o):
//   rule 4's double clamp; x's own D and Vs stay in registers for all offsets), one barrier, then every pixel sums its (2P + 1)^2 patch from the buffer.
//   Two buffers make one barrier per offset enough: offset n + 1 writes the other buffer while slower lanes still read this one, and the barrier of
//   offset n + 1 lies between those reads and the writes of offset n + 2.
//   Every coordinate that indexes LDS or the planes is clamped to the image first, and a clamped coordinate lies inside the staged window: the tile holds
//   at least one image pixel, so 0 <= x0 <= w - 1 and the window [x0 - H, x0 + 31 + H] cut to the image is what positions and partners can reach.
template <int P>
__global__ void __launch_bounds__(kDnLanes) rt_denoise_kernel(float *__restrict__ out, const float *__restrict__ img, const float *__restrict__ vs, int w, int h,
                                                              int R, float alpha, float kk) {
    extern __shared__ float dn_lds[];
    constexpr int EW = kDnTileW + 2 * P, EH = kDnTileH + 2 * P, EN = EW * EH;      // 256 / 340 / 432 positions: at most two per lane
    const int H = R + P, LW = kDnTileW + 2 * H, LH = kDnTileH + 2 * H, LN = LW * LH;
    float *const sD = dn_lds, *const sV = dn_lds + 3 * LN, *const sE = dn_lds + 6 * LN;
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
    const int wx0 = x0 - H, wy0 = y0 - H;                   // the window's origin in the plane

    for (int l = tid; l < LN; l += kDnLanes) {
        const int ly = l / LW, lx = l - ly * LW;
        const size_t at = 3 * ((size_t)dn_clamp(wy0 + ly, h) * (size_t)w + (size_t)dn_clamp(wx0 + lx, w));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sD[c * LN + l] = img[at + c];
            sV[c * LN + l] = vs[at + c];
        }
    }
    __syncthreads();

    // this lane's positions of the tile and its P-halo: plane coordinates (clamped), and what rule 3 reads of the position itself
    int ex[2], ey[2];
    float pd[2][3], pv[2][3];
    bool have[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        have[s] = tid + s * kDnLanes < EN;
        const int idx = have[s] ? tid + s * kDnLanes : 0, iy = idx / EW, ix = idx - iy * EW;
        ex[s] = dn_clamp(x0 - P + ix, w);
        ey[s] = dn_clamp(y0 - P + iy, h);
        const int l = (ey[s] - wy0) * LW + (ex[s] - wx0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pd[s][c] = sD[c * LN + l];
            pv[s][c] = sV[c * LN + l];
        }
    }

    const int tx = tid & (kDnTileW - 1), ty = tid / kDnTileW, px = x0 + tx, py = y0 + ty;
    const bool inside = px < w && py < h;
    const float inv = 1.0f / (float)(3 * (2 * P + 1) * (2 * P + 1));
    float num0 = 0.0f, num1 = 0.0f, num2 = 0.0f, den = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; ++oy)
        for (int ox = -R; ox <= R; ++ox) {
            const bool centre = oy == 0 && ox == 0;
            float *const e = sE + buf * EN;
            if (!centre) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!have[s]) continue;
                    const int l = (dn_clamp(ey[s] + oy, h) - wy0) * LW + (dn_clamp(ex[s] + ox, w) - wx0);    // q' = cl(x + o)
                    float d[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {           // rule 3
                        const float qd = sD[c * LN + l], qv = sV[c * LN + l];
                        const float t = pd[s][c] - qd;
                        const float m = qv < pv[s][c] ? qv : pv[s][c];
                        d[c] = (t * t - alpha * (pv[s][c] + m)) / (1e-10f + kk * (pv[s][c] + qv));
                    }
                    e[tid + s * kDnLanes] = (d[0] + d[1]) + d[2];
                }
            }
            __syncthreads();
            buf ^= 1;
            const int qx = px + ox, qy = py + oy;
            if (inside && qx >= 0 && qx < w && qy >= 0 && qy < h) {   // rule 5: p + o outside the image is skipped
                const int l = (qy - wy0) * LW + (qx - wx0);
                const float q0 = sD[l], q1 = sD[LN + l], q2 = sD[2 * LN + l];
                float wgt = 1.0f;
                bool take = true;
                if (!centre) {
                    float S = 0.f;                          // rule 4: the entries of the tile's P-halo ARE the clamped positions
#pragma unroll
                    for (int dy = 0; dy <= 2 * P; ++dy)
#pragma unroll
                        for (int dx = 0; dx <= 2 * P; ++dx) {
                            const float v = e[(ty + dy) * EW + tx + dx];
                            S = (dy == 0 && dx == 0) ? v : S + v;
                        }
                    const float T = S * inv;
                    take = T == T && fabsf(q0) <= FLT_MAX && fabsf(q1) <= FLT_MAX && fabsf(q2) <= FLT_MAX;
                    const float g = T > 0.f ? T : 0.f;
                    wgt = 1.0f / (1.0f + g * (1.0f + g * 0.5f));
                }
                if (take) {                                 // rule 6
                    num0 = num0 + wgt * q0;
                    num1 = num1 + wgt * q1;
                    num2 = num2 + wgt * q2;
                    den = den + wgt;
                }
            }
        }
    if (!inside) return;
    const size_t at = 3 * ((size_t)py * (size_t)w + (size_t)px);
    out[at] = num0 / den;
    out[at + 1] = num1 / den;
    out[at + 2] = num2 / den;
}

using namespace rt;

namespace {

size_t denoise_lds_bytes(int R, int P) {
    const int H = R + P;
    return ((size_t)6 * (kDnTileW + 2 * H) * (kDnTileH + 2 * H) + (size_t)2 * (kDnTileW + 2 * P) * (kDnTileH + 2 * P)) * sizeof(float);
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

}  // namespace

extern "C" {

RT_API int rt_denoise_async(rt_ctx *dst, rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream) {
    int rc = check_three(dst, a, b);
    if (rc != RT_OK) return rc;
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;
    if (a->frame.current_sample != b->frame.current_sample)
        return fail(RT_ERR_STATE, "rt_denoise_async: the halves hold %d and %d passes", a->frame.current_sample, b->frame.current_sample);
    if (a->frame.current_sample <= 0) return fail(RT_ERR_STATE, "rt_denoise_async: the halves hold no pass");
    if ((long long)dst->frame.current_sample != 2ll * a->frame.current_sample)
        return fail(RT_ERR_STATE, "rt_denoise_async: the destination holds %d passes, the halves %d each: it is not their merge", dst->frame.current_sample,
                    a->frame.current_sample);
    if (q.search_radius == 0) return RT_OK;                 // the window is the pixel itself: the image, bit for bit
    rc = select_device(dst);
    if (rc != RT_OK) return rc;
    const size_t n_floats = color_floats(dst);
    if (!dst->d_denoise) HIP_TRY(hipMalloc(&dst->d_denoise, n_floats * sizeof(float)));
    if (!dst->d_denoise_var) HIP_TRY(hipMalloc(&dst->d_denoise_var, n_floats * sizeof(float)));
    // behind everything the three contexts have queued; their later work behind the filter
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(dst, stream);
    if (rc == RT_OK) rc = chain(a, stream);
    if (rc == RT_OK) rc = chain(b, stream);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(rt_denoise_variance_kernel, dim3((unsigned)((3 * (size_t)dst->w + 255) / 256), (unsigned)std::min(dst->h, 65535)), dim3(256), 0, stream,
                       dst->d_denoise_var, a->d_colors, b->d_colors, dst->w, dst->h);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((dst->w + kDnTileW - 1) / kDnTileW), (unsigned)((dst->h + kDnTileH - 1) / kDnTileH));
    const size_t lds = denoise_lds_bytes(q.search_radius, q.patch_radius);
    const float kk = q.k * q.k;
    switch (q.patch_radius) {
    case 0: hipLaunchKernelGGL(rt_denoise_kernel<0>, grid, dim3(kDnLanes), lds, stream, dst->d_denoise, dst->d_colors, dst->d_denoise_var, dst->w, dst->h, q.search_radius, q.alpha, kk); break;
    case 1: hipLaunchKernelGGL(rt_denoise_kernel<1>, grid, dim3(kDnLanes), lds, stream, dst->d_denoise, dst->d_colors, dst->d_denoise_var, dst->w, dst->h, q.search_radius, q.alpha, kk); break;
    default: hipLaunchKernelGGL(rt_denoise_kernel<2>, grid, dim3(kDnLanes), lds, stream, dst->d_denoise, dst->d_colors, dst->d_denoise_var, dst->w, dst->h, q.search_radius, q.alpha, kk); break;
    }
    HIP_TRY(hipGetLastError());
    std::swap(dst->d_colors, dst->d_denoise);               // the filtered plane IS the colour plane now; the old one is the next call's scratch
    dst->frame.colours_replaced();                          // rt_read_pixels packs the filtered plane
    return RT_OK;
}

}  // extern "C"
