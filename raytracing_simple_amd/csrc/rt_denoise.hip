// rt_denoise.hip -- denoising (include/rt_api.h, "denoising"): a non-local-means filter of a merged frame, steered by the difference of the two
// halves it was merged from (Rousselle, Knaus, Zwicker 2012) --
//   rt_denoise_async         dst's colour plane filtered on the device, the colour planes of a and b as the variance estimate
// and the kernels behind it.  rt_denoise_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 1-6, and the
// comments below name the rule a line implements.  The reference filters nothing: this is the library's own extension.
// "The error of the filtered frame" of the same header lives here too --
//   rt_denoise_pair_async    each half filtered with weights taken from the OTHER half, into planes of their own beside the colour planes
//   rt_denoise_pair_tiles_async   ... of the groups in the current selection alone (adaptive sampling's groups: rt_tiles.hip), the rest kept
//   rt_read_filtered         that plane of one context
// (rt_denoise_pair_planes is the host statement; rt_compare.hip compares the packed planes).
// As rt_host.cpp filters through one nlm_planes(out, img, guide, ...), the device filters through ONE body, dn_body<P, N, kAnyRow>: N = 1 is the frame
// filtered with its own weights, N = 2 the two halves, each with the other's.  Three kernels give it an origin: the frame, the frame's halves, a list
// of groups.
// The render kernels are not touched, and nothing here reads or writes anything but colour planes.
// This unit is compiled with -ffp-contract=off: every multiply, add and IEEE division below is an operation of its own, in the written order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include <atomic>
#include <type_traits>

#include "rt_detmath.h"
#include "rt_internal.h"

using rt::fail;

extern "C" int rt_host_denoise_params(const rt_denoise_params *p, rt_denoise_params *out);     // rt_host.cpp: the parameter rules (null = defaults)

namespace {

constexpr int kDnTileW = 32, kDnTileH = 8, kDnLanes = kDnTileW * kDnTileH;      // a workgroup's output pixels: four wavefronts, a row of 32 per half-wave

__device__ __forceinline__ int dn_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// .cl:34, the pack kernel's toInt (rt_trace.inc.h to_int): parity's restated powf, or fast mode's exp2 / log2 with the fused multiply-add that
// unit's contraction makes of g * 255 + .5 (this unit contracts nothing, so it is written out)
__device__ __forceinline__ uint32_t dn_to_int(float v, bool fast) {
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    if (fast) return (uint32_t)(int)__builtin_fmaf(rt::fm_powf(c, 1.f / 2.2f), 255.f, .5f);
    return (uint32_t)(int)(rt::dm_powf(c, 1.f / 2.2f) * 255.f + .5f);
}

__device__ __forceinline__ bool dn_finite3(float a, float b, float c) { return fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX && fabsf(c) <= FLT_MAX; }

// What a filter kernel reads and writes per image: the plane, the filtered plane, and -- the halves only -- the filtered plane packed by the toInt
// of that context's mode
template <int N>
struct DnPlanes {
    const float *img[N];
    float *out[N];
    uint32_t *px[N];
    int fast[N];
};

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

// Rules 3 to 6 for N images at once: image i takes its weights from guide N - 1 - i -- itself (N = 1: rt_denoise_planes) or the other half (N = 2:
// rt_denoise_pair_planes, the header's three substitutions).  A workgroup owns the 32x8 output pixels at (x0, y0) of the plane; H = R + P.
//   LDS: 3 N image planes and three variance planes (Vs; N = 2: Vh = Vs + Vs, the variance of one half) of LW x LH = (32 + 2H) x (8 + 2H) floats,
//   entry (ly, lx) = the plane at cl(y0 - H + ly, x0 - H + lx) -- one float per lane and read, consecutive lanes on consecutive banks -- then 2 N
//   buffers of EW x EH = (32 + 2P) x (8 + 2P) floats: e(., o) of every guide, twice.  48 (N + 1)(R + P + 16)(R + P + 4) + 32 N (P + 16)(P + 4) bytes,
//   59 328 for N = 2 at R 8, P 2: below 64 KiB, no attribute call.
//   Per offset o: every lane forms e(x, o) for its one or two positions x of the tile and its P-halo (x = the CLAMPED position, its partner cl(x + o):
//   rule 4's double clamp; x's own planes stay in registers for all offsets; rule 3's alpha * (V[x] + m) and 1e-10f + kk * (V[x] + V[q']) serve every
//   guide, t, the square and the division are per guide), one barrier, then every pixel sums its (2P + 1)^2 patch from the buffers.  Two sets of
//   buffers make one barrier per offset enough: offset n + 1 writes the other set while slower lanes still read this one, and the barrier of offset
//   n + 1 lies between those reads and the writes of offset n + 2.
//   Bounds: every coordinate that indexes LDS or a plane is clamped to the image first, and a clamped coordinate lies inside the staged window: the
//   32x8 pixels hold at least one image pixel, so positions clamp into [max(0, x0 - P), min(w - 1, x0 + 31 + P)] (rows alike) and their partners within
//   R of that, all inside the window [x0 - H, x0 + 31 + H] cut to the image.  kAnyRow: y0 may be NEGATIVE, -7 at the least, with y0 + 7 >= 0 -- the
//   top group row of an image whose height is no multiple of 8 (rt_denoise_pair_tiles_kernel).  The argument holds as it stands; what is added is that
//   a lane above the plane's row 0 is outside the image and stores nothing.
// N = 2 also packs: the words go to the pixel buffer's row (row 0 = bottom: plane row h - 1 - y).
template <int P, int N, bool kAnyRow>
__device__ __forceinline__ void dn_body(float *dn_lds, const int x0, const int y0, const DnPlanes<N> &k, const float *__restrict__ vs, int w, int h, int R,
                                        float alpha, float kk) {
    constexpr int EW = kDnTileW + 2 * P, EH = kDnTileH + 2 * P, EN = EW * EH;      // 256 / 340 / 432 positions: at most two per lane
    const int H = R + P, LW = kDnTileW + 2 * H, LH = kDnTileH + 2 * H, LN = LW * LH;
    float *const sI = dn_lds, *const sV = dn_lds + 3 * N * LN, *const sE = dn_lds + 3 * (N + 1) * LN;     // image i, channel c: sI + (3 i + c) LN
    const int tid = (int)threadIdx.x;
    const int wx0 = x0 - H, wy0 = y0 - H;                   // the window's origin in the plane

    for (int l = tid; l < LN; l += kDnLanes) {
        const int ly = l / LW, lx = l - ly * LW;
        const size_t at = 3 * ((size_t)dn_clamp(wy0 + ly, h) * (size_t)w + (size_t)dn_clamp(wx0 + lx, w));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = vs[at + c];
#pragma unroll
            for (int i = 0; i < N; ++i) sI[(3 * i + c) * LN + l] = k.img[i][at + c];
            sV[c * LN + l] = N == 2 ? v + v : v;
        }
    }
    __syncthreads();

    // this lane's positions of the tile and its P-halo: plane coordinates (clamped), and what rule 3 reads of the position itself
    int ex[2], ey[2];
    float pi[2][N][3], pv[2][3];
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
#pragma unroll
            for (int i = 0; i < N; ++i) pi[s][i][c] = sI[(3 * i + c) * LN + l];
            pv[s][c] = sV[c * LN + l];
        }
    }

    const int tx = tid & (kDnTileW - 1), ty = tid / kDnTileW, px = x0 + tx, py = y0 + ty;
    const bool inside = px < w && py < h && (!kAnyRow || py >= 0);
    const float inv = 1.0f / (float)(3 * (2 * P + 1) * (2 * P + 1));
    float num[N][3], den[N];
#pragma unroll
    for (int i = 0; i < N; ++i) num[i][0] = num[i][1] = num[i][2] = den[i] = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; ++oy)
        for (int ox = -R; ox <= R; ++ox) {
            const bool centre = oy == 0 && ox == 0;
            float *const e = sE + (N * buf) * EN;           // e(., o) of guide g: e + g * EN
            if (!centre) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!have[s]) continue;
                    const int l = (dn_clamp(ey[s] + oy, h) - wy0) * LW + (dn_clamp(ex[s] + ox, w) - wx0);    // q' = cl(x + o)
                    float d[N][3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {           // rule 3, for every guide
                        const float qv = sV[c * LN + l];
                        const float m = qv < pv[s][c] ? qv : pv[s][c];
                        const float off = alpha * (pv[s][c] + m), dnm = 1e-10f + kk * (pv[s][c] + qv);
#pragma unroll
                        for (int g = 0; g < N; ++g) {
                            const float t = pi[s][g][c] - sI[(3 * g + c) * LN + l];
                            d[g][c] = (t * t - off) / dnm;
                        }
                    }
#pragma unroll
                    for (int g = 0; g < N; ++g) e[g * EN + tid + s * kDnLanes] = (d[g][0] + d[g][1]) + d[g][2];
                }
            }
            __syncthreads();
            buf ^= 1;
            const int qx = px + ox, qy = py + oy;
            if (inside && qx >= 0 && qx < w && qy >= 0 && qy < h) {   // rule 5: p + o outside the image is skipped
                const int l = (qy - wy0) * LW + (qx - wx0);
                float q[N][3], wgt[N];
                bool take[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[i][c] = sI[(3 * i + c) * LN + l];
                    wgt[i] = 1.0f;
                    take[i] = true;
                }
                if (!centre) {
                    float S[N];                             // rule 4: the entries of the tile's P-halo ARE the clamped positions
#pragma unroll
                    for (int g = 0; g < N; ++g) S[g] = 0.f;
#pragma unroll
                    for (int dy = 0; dy <= 2 * P; ++dy)
#pragma unroll
                        for (int dx = 0; dx <= 2 * P; ++dx)
#pragma unroll
                            for (int g = 0; g < N; ++g) {
                                const float v = e[g * EN + (ty + dy) * EW + tx + dx];
                                S[g] = (dy == 0 && dx == 0) ? v : S[g] + v;
                            }
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const float T = S[N - 1 - i] * inv;
                        take[i] = T == T && dn_finite3(q[i][0], q[i][1], q[i][2]);
                        const float g = T > 0.f ? T : 0.f;
                        wgt[i] = 1.0f / (1.0f + g * (1.0f + g * 0.5f));
                    }
                }
#pragma unroll
                for (int i = 0; i < N; ++i)
                    if (take[i]) {                          // rule 6
#pragma unroll
                        for (int c = 0; c < 3; ++c) num[i][c] = num[i][c] + wgt[i] * q[i][c];
                        den[i] = den[i] + wgt[i];
                    }
            }
        }
    if (!inside) return;
    const size_t at = 3 * ((size_t)py * (size_t)w + (size_t)px);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float f0 = num[i][0] / den[i], f1 = num[i][1] / den[i], f2 = num[i][2] / den[i];
        if constexpr (N == 2) {
            if (R == 0) {                                   // the window is the pixel itself: the halves, bit for bit
                const int l = (py - wy0) * LW + (px - wx0);
                f0 = sI[(3 * i) * LN + l], f1 = sI[(3 * i + 1) * LN + l], f2 = sI[(3 * i + 2) * LN + l];
            }
        }
        k.out[i][at] = f0;
        k.out[i][at + 1] = f1;
        k.out[i][at + 2] = f2;
        if constexpr (N == 2) {
            const bool fast = k.fast[i] != 0;
            k.px[i][(size_t)(h - 1 - py) * (size_t)w + (size_t)px] = dn_to_int(f0, fast) | (dn_to_int(f1, fast) << 8) | (dn_to_int(f2, fast) << 16);
        }
    }
}

// ... over the frame: the plane tiled from its row 0, a workgroup per 32x8 pixels -- the merged frame with its own weights,
template <int P>
__global__ void __launch_bounds__(kDnLanes) rt_denoise_kernel(DnPlanes<1> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk) {
    extern __shared__ float dn_lds[];
    dn_body<P, 1, false>(dn_lds, (int)blockIdx.x * kDnTileW, (int)blockIdx.y * kDnTileH, k, vs, w, h, R, alpha, kk);
}

// ... the two halves.  (waves_per_eu: at the default radii, R 5 and P 1 -- the only ones it was measured at -- LDS admits four workgroups a CU, a
// wavefront of each per SIMD.  Told so, the compiler keeps rule 3's independent divisions interleaved; left to aim for a seventh wavefront, it
// serialises them in this instance to save two registers, which measured 1.9 % slower at 1920x1080 -- profiles/HISTORY.md.  The hint bounds nothing
// at run time and the register counts are the same with it, 60 / 74 / 93.  It ALLOWS the compiler 128 registers, though: at small radii (R 1, P 0:
// nine workgroups a CU by LDS) occupancy is bound by registers, so a body that grows must be looked at again with the hint taken off.)
template <int P>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kDnLanes)
rt_denoise_pair_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk) {
    extern __shared__ float dn_lds[];
    dn_body<P, 2, false>(dn_lds, (int)blockIdx.x * kDnTileW, (int)blockIdx.y * kDnTileH, k, vs, w, h, R, alpha, kk);
}

// ... and the halves over the groups of a selection (rt_tiles.hip): workgroup i takes group list[i] -- g = gy * groups_x + gx in the PIXEL BUFFER's tile
// rows, row 0 at the bottom -- and covers its pixel rows 8 gy .. 8 gy + 7, which are the plane's rows h - 8 (gy + 1) .. h - 1 - 8 gy: the origin is
// negative for the top, partial, group row.  Every other pixel of the four output planes keeps its words.  A list entry that names no group is skipped
// by the whole workgroup, ahead of the first barrier.
template <int P>
__global__ void __attribute__((amdgpu_waves_per_eu(1, 4))) __launch_bounds__(kDnLanes)
rt_denoise_pair_tiles_kernel(DnPlanes<2> k, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, const uint32_t *__restrict__ list,
                             uint32_t groups_x, uint32_t n_groups) {
    extern __shared__ float dn_lds[];
    const uint32_t g = list[blockIdx.x];
    if (g >= n_groups) return;
    const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
    dn_body<P, 2, true>(dn_lds, (int)gx * kDnTileW, h - kDnTileH * ((int)gy + 1), k, vs, w, h, R, alpha, kk);
}

using namespace rt;

namespace {

std::atomic<uint64_t> g_pair_calls{0};                     // numbers the calls that make cross-filtered planes (FrameState::filtered_pair)

size_t lds_bytes(int N, int R, int P) {                    // dn_body's layout
    const int H = R + P;
    return ((size_t)3 * (N + 1) * (kDnTileW + 2 * H) * (kDnTileH + 2 * H) + (size_t)2 * N * (kDnTileW + 2 * P) * (kDnTileH + 2 * P)) * sizeof(float);
}

bool packs_fast(const rt_ctx *c) { return c->mode == RT_MODE_FAST || c->mode >= 200; }     // which pack kernel refresh_pixels launches (rt_api.hip)

dim3 frame_grid(const rt_ctx *c) { return dim3((unsigned)((c->w + kDnTileW - 1) / kDnTileW), (unsigned)((c->h + kDnTileH - 1) / kDnTileH)); }

int launch_variance(float *var, const float *a, const float *b, int w, int h, hipStream_t stream) {
    hipLaunchKernelGGL(rt_denoise_variance_kernel, dim3((unsigned)((3 * (size_t)w + 255) / 256), (unsigned)std::min(h, 65535)), dim3(256), 0, stream, var, a, b, w, h);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// f(std::integral_constant<int, P>) for the instantiated patch radius (rt_host_denoise_params allows 0, 1, 2)
template <class F>
void with_patch_radius(int patch_radius, F &&f) {
    switch (patch_radius) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    default: f(std::integral_constant<int, 2>{}); break;
    }
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
        if (!c->d_filtered) HIP_TRY(hipMalloc(&c->d_filtered, n_floats * sizeof(float)));
        if (!c->d_filtered_px) HIP_TRY(hipMalloc(&c->d_filtered_px, n_words * sizeof(uint32_t)));
    }
    if (!a->d_denoise_var) HIP_TRY(hipMalloc(&a->d_denoise_var, n_floats * sizeof(float)));
    // behind everything the two contexts have queued; their later work behind the filter
    int rc = chain(a, stream);
    if (rc == RT_OK) rc = chain(b, stream);
    if (rc == RT_OK && tiles && a->frame.group_list_is_stale()) rc = tiles_build_group_list(a, stream);
    if (rc == RT_OK) rc = launch_variance(a->d_denoise_var, a->d_colors, b->d_colors, a->w, a->h, stream);
    if (rc != RT_OK) return rc;
    const DnPlanes<2> k{ { a->d_colors, b->d_colors }, { a->d_filtered, b->d_filtered }, { a->d_filtered_px, b->d_filtered_px }, { packs_fast(a), packs_fast(b) } };
    const size_t lds = lds_bytes(2, q.search_radius, q.patch_radius);
    const float kk = q.k * q.k;
    with_patch_radius(q.patch_radius, [&](auto P) {
        if (tiles)
            hipLaunchKernelGGL(rt_denoise_pair_tiles_kernel<decltype(P)::value>, dim3(a->frame.counts[0]), dim3(kDnLanes), lds, stream, k, a->d_denoise_var, a->w,
                               a->h, q.search_radius, q.alpha, kk, a->tiles.d_groups, groups_per_row(a), group_count(a));
        else
            hipLaunchKernelGGL(rt_denoise_pair_kernel<decltype(P)::value>, frame_grid(a), dim3(kDnLanes), lds, stream, k, a->d_denoise_var, a->w, a->h,
                               q.search_radius, q.alpha, kk);
    });
    HIP_TRY(hipGetLastError());
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
    if (!a->d_filtered || !b->d_filtered || !a->d_filtered_px || !b->d_filtered_px || !a->d_denoise_var || !a->tiles.d_selected)
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
    if (rc == RT_OK) rc = launch_variance(dst->d_denoise_var, a->d_colors, b->d_colors, dst->w, dst->h, stream);
    if (rc != RT_OK) return rc;
    const DnPlanes<1> k{ { dst->d_colors }, { dst->d_denoise }, { nullptr }, { 0 } };       // (nothing is packed: rt_read_pixels packs the colour plane)
    with_patch_radius(q.patch_radius, [&](auto P) {
        hipLaunchKernelGGL(rt_denoise_kernel<decltype(P)::value>, frame_grid(dst), dim3(kDnLanes), lds_bytes(1, q.search_radius, q.patch_radius), stream, k,
                           dst->d_denoise_var, dst->w, dst->h, q.search_radius, q.alpha, q.k * q.k);
    });
    HIP_TRY(hipGetLastError());
    std::swap(dst->d_colors, dst->d_denoise);               // the filtered plane IS the colour plane now; the old one is the next call's scratch
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

RT_API int rt_read_filtered(rt_ctx *c, float *out_host) {
    int rc = tiles_refuse(c, "rt_read_filtered");
    if (rc != RT_OK) return rc;
    if (!out_host) return fail(RT_ERR_ARG, "rt_read_filtered: out_host is null");
    if (c->frame.filtered_pair == 0)
        return fail(RT_ERR_STATE, "rt_read_filtered: the context holds no current cross-filtered plane (rt_denoise_pair_async makes one; whatever moves the colour plane ends it)");
    return read_back(c, out_host, c->d_filtered, color_floats(c) * sizeof(float));
}

}  // extern "C"
