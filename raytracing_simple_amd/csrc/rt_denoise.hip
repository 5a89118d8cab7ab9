// rt_denoise.hip -- denoising (include/rt_api.h, "denoising"): a non-local-means filter of a merged frame, steered by the difference of the two
// halves it was merged from (Rousselle, Knaus, Zwicker 2012) --
//   rt_denoise_async         dst's colour plane filtered on the device, the colour planes of a and b as the variance estimate
// and the two kernels behind it.  rt_denoise_planes (rt_host.cpp) is the same arithmetic as plain loops; the header states it as rules 1-6, and the
// comments below name the rule a line implements.  The reference filters nothing: this is the library's own extension.
// "The error of the filtered frame" of the same header lives here too --
//   rt_denoise_pair_async    each half filtered with weights taken from the OTHER half, into planes of their own beside the colour planes
//   rt_denoise_pair_tiles_async   ... of the groups in the current selection alone (adaptive sampling's groups: rt_tiles.hip), the rest kept
//   rt_read_filtered         that plane of one context
// and one kernel body that forms both planes together, instantiated over the frame and over a list of groups (rt_denoise_pair_planes is its host
// statement).  rt_compare.hip compares the packed planes.
// The render kernels are not touched, and nothing here reads or writes anything but colour planes.
// This unit is compiled with -ffp-contract=off: every multiply, add and IEEE division below is an operation of its own, in the written order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include <atomic>

#include "rt_detmath.h"
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

namespace {

// .cl:34, the pack kernel's toInt (rt_trace.inc.h to_int): parity's restated powf, or fast mode's exp2 / log2 with the fused multiply-add that
// unit's contraction makes of g * 255 + .5 (this unit contracts nothing, so it is written out)
__device__ __forceinline__ uint32_t dn_to_int(float v, bool fast) {
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    if (fast) return (uint32_t)(int)__builtin_fmaf(rt::fm_powf(c, 1.f / 2.2f), 255.f, .5f);
    return (uint32_t)(int)(rt::dm_powf(c, 1.f / 2.2f) * 255.f + .5f);
}

__device__ __forceinline__ bool dn_finite3(float a, float b, float c) { return fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX && fabsf(c) <= FLT_MAX; }

}  // namespace

// The cross-filtered halves: FA = A filtered with weights from B, FB = B with weights from A, rules 3 to 6 with the header's three substitutions,
// both in one pass.  The shape is rt_denoise_kernel's -- a workgroup per 32x8 pixels, H = R + P, one barrier per offset -- with
//   LDS: NINE planes (A, B and Vh = Vs + Vs, three channels each) of LW x LH floats, then FOUR buffers of EW x EH floats: e(., o) of guide A and of
//   guide B, each twice, so that offset n + 1 writes the other pair while slower lanes still read this one (as the two buffers there).
//   (9 * 52 * 28 + 4 * 36 * 12) * 4 = 59 328 bytes at R 8, P 2: below 64 KiB, no attribute call.
//   Rule 3's alpha * (Vh[p] + m) and 1e-10f + kk * (Vh[p] + Vh[q']) are formed once per position and offset and serve both directions; t, the
//   square and the division are per direction.
// The index arithmetic and its bounds are that kernel's, line for line: every coordinate that indexes LDS or a plane is clamped to the image first,
// and a clamped coordinate lies inside the staged window.  The packed words go to the pixel buffer's row (row 0 = bottom: plane row h - 1 - y).
// The body takes the workgroup's origin (x0, y0) in the plane from its kernel.  kAnyRow: y0 may be NEGATIVE, -7 at the least, and y0 + 7 >= 0 -- the
// top group row of an image whose height is no multiple of 8 (rt_denoise_pair_tiles_kernel below).  The bounds hold as they stand: the 32x8 pixels
// still hold an image pixel, so positions clamp into [max(0, y0 - P), min(h - 1, y0 + 7 + P)] and their partners within R of that, all inside the
// window's rows [y0 - H, y0 + 7 + H] cut to the image; what is added is that a lane above the plane's row 0 is outside the image and stores nothing.
template <int P, bool kAnyRow>
__device__ __forceinline__ void dn_pair_body(float *dn_lds, const int x0, const int y0, float *__restrict__ out_a, float *__restrict__ out_b,
                                             uint32_t *__restrict__ px_a, uint32_t *__restrict__ px_b, const float *__restrict__ a,
                                             const float *__restrict__ b, const float *__restrict__ vs, int w, int h, int R, float alpha, float kk,
                                             int fast_a, int fast_b) {
    constexpr int EW = kDnTileW + 2 * P, EH = kDnTileH + 2 * P, EN = EW * EH;
    const int H = R + P, LW = kDnTileW + 2 * H, LH = kDnTileH + 2 * H, LN = LW * LH;
    float *const sA = dn_lds, *const sB = dn_lds + 3 * LN, *const sV = dn_lds + 6 * LN, *const sE = dn_lds + 9 * LN;
    const int tid = (int)threadIdx.x;
    const int wx0 = x0 - H, wy0 = y0 - H;

    for (int l = tid; l < LN; l += kDnLanes) {
        const int ly = l / LW, lx = l - ly * LW;
        const size_t at = 3 * ((size_t)dn_clamp(wy0 + ly, h) * (size_t)w + (size_t)dn_clamp(wx0 + lx, w));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = vs[at + c];
            sA[c * LN + l] = a[at + c];
            sB[c * LN + l] = b[at + c];
            sV[c * LN + l] = v + v;                         // Vh: the variance of one half
        }
    }
    __syncthreads();

    int ex[2], ey[2];
    float pa[2][3], pb[2][3], pv[2][3];
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
            pa[s][c] = sA[c * LN + l];
            pb[s][c] = sB[c * LN + l];
            pv[s][c] = sV[c * LN + l];
        }
    }

    const int tx = tid & (kDnTileW - 1), ty = tid / kDnTileW, px = x0 + tx, py = y0 + ty;
    const bool inside = px < w && py < h && (!kAnyRow || py >= 0);
    const float inv = 1.0f / (float)(3 * (2 * P + 1) * (2 * P + 1));
    float na0 = 0.0f, na1 = 0.0f, na2 = 0.0f, da = 0.0f, nb0 = 0.0f, nb1 = 0.0f, nb2 = 0.0f, db = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; ++oy)
        for (int ox = -R; ox <= R; ++ox) {
            const bool centre = oy == 0 && ox == 0;
            float *const e_ga = sE + (2 * buf) * EN, *const e_gb = e_ga + EN;      // e(., o) of guide A (it weights FB), of guide B (it weights FA)
            if (!centre) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!have[s]) continue;
                    const int l = (dn_clamp(ey[s] + oy, h) - wy0) * LW + (dn_clamp(ex[s] + ox, w) - wx0);    // q' = cl(x + o)
                    float d_ga[3], d_gb[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {           // rule 3, G = A and G = B
                        const float qv = sV[c * LN + l];
                        const float m = qv < pv[s][c] ? qv : pv[s][c];
                        const float off = alpha * (pv[s][c] + m), dnm = 1e-10f + kk * (pv[s][c] + qv);
                        const float t_a = pa[s][c] - sA[c * LN + l], t_b = pb[s][c] - sB[c * LN + l];
                        d_ga[c] = (t_a * t_a - off) / dnm;
                        d_gb[c] = (t_b * t_b - off) / dnm;
                    }
                    e_ga[tid + s * kDnLanes] = (d_ga[0] + d_ga[1]) + d_ga[2];
                    e_gb[tid + s * kDnLanes] = (d_gb[0] + d_gb[1]) + d_gb[2];
                }
            }
            __syncthreads();
            buf ^= 1;
            const int qx = px + ox, qy = py + oy;
            if (inside && qx >= 0 && qx < w && qy >= 0 && qy < h) {   // rule 5: p + o outside the image is skipped
                const int l = (qy - wy0) * LW + (qx - wx0);
                const float a0 = sA[l], a1 = sA[LN + l], a2 = sA[2 * LN + l], b0 = sB[l], b1 = sB[LN + l], b2 = sB[2 * LN + l];
                float w_a = 1.0f, w_b = 1.0f;               // the weight FA's sum takes (from guide B), FB's (from guide A)
                bool take_a = true, take_b = true;
                if (!centre) {
                    float s_ga = 0.f, s_gb = 0.f;           // rule 4
#pragma unroll
                    for (int dy = 0; dy <= 2 * P; ++dy)
#pragma unroll
                        for (int dx = 0; dx <= 2 * P; ++dx) {
                            const float v_ga = e_ga[(ty + dy) * EW + tx + dx], v_gb = e_gb[(ty + dy) * EW + tx + dx];
                            s_ga = (dy == 0 && dx == 0) ? v_ga : s_ga + v_ga;
                            s_gb = (dy == 0 && dx == 0) ? v_gb : s_gb + v_gb;
                        }
                    const float t_ga = s_ga * inv, t_gb = s_gb * inv;
                    take_a = t_gb == t_gb && dn_finite3(a0, a1, a2);
                    take_b = t_ga == t_ga && dn_finite3(b0, b1, b2);
                    const float g_a = t_gb > 0.f ? t_gb : 0.f, g_b = t_ga > 0.f ? t_ga : 0.f;
                    w_a = 1.0f / (1.0f + g_a * (1.0f + g_a * 0.5f));
                    w_b = 1.0f / (1.0f + g_b * (1.0f + g_b * 0.5f));
                }
                if (take_a) {                               // rule 6
                    na0 = na0 + w_a * a0;
                    na1 = na1 + w_a * a1;
                    na2 = na2 + w_a * a2;
                    da = da + w_a;
                }
                if (take_b) {
                    nb0 = nb0 + w_b * b0;
                    nb1 = nb1 + w_b * b1;
                    nb2 = nb2 + w_b * b2;
                    db = db + w_b;
                }
            }
        }
    if (!inside) return;
    float fa0 = na0 / da, fa1 = na1 / da, fa2 = na2 / da, fb0 = nb0 / db, fb1 = nb1 / db, fb2 = nb2 / db;
    if (R == 0) {                                           // the window is the pixel itself: the halves, bit for bit
        const int l = (py - wy0) * LW + (px - wx0);
        fa0 = sA[l], fa1 = sA[LN + l], fa2 = sA[2 * LN + l];
        fb0 = sB[l], fb1 = sB[LN + l], fb2 = sB[2 * LN + l];
    }
    const size_t at = 3 * ((size_t)py * (size_t)w + (size_t)px), word = (size_t)(h - 1 - py) * (size_t)w + (size_t)px;
    out_a[at] = fa0;
    out_a[at + 1] = fa1;
    out_a[at + 2] = fa2;
    out_b[at] = fb0;
    out_b[at + 1] = fb1;
    out_b[at + 2] = fb2;
    px_a[word] = dn_to_int(fa0, fast_a != 0) | (dn_to_int(fa1, fast_a != 0) << 8) | (dn_to_int(fa2, fast_a != 0) << 16);
    px_b[word] = dn_to_int(fb0, fast_b != 0) | (dn_to_int(fb1, fast_b != 0) << 8) | (dn_to_int(fb2, fast_b != 0) << 16);
}

// ... over the frame: the plane tiled from its row 0, a workgroup per 32x8 pixels
template <int P>
__global__ void __launch_bounds__(kDnLanes) rt_denoise_pair_kernel(float *__restrict__ out_a, float *__restrict__ out_b, uint32_t *__restrict__ px_a,
                                                                   uint32_t *__restrict__ px_b, const float *__restrict__ a, const float *__restrict__ b,
                                                                   const float *__restrict__ vs, int w, int h, int R, float alpha, float kk, int fast_a,
                                                                   int fast_b) {
    extern __shared__ float dn_lds[];
    dn_pair_body<P, false>(dn_lds, (int)blockIdx.x * kDnTileW, (int)blockIdx.y * kDnTileH, out_a, out_b, px_a, px_b, a, b, vs, w, h, R, alpha, kk, fast_a,
                           fast_b);
}

// ... over the groups of a selection (rt_tiles.hip): workgroup i takes group list[i] -- g = gy * groups_x + gx in the PIXEL BUFFER's tile rows, row 0 at
// the bottom -- and covers its pixel rows 8 gy .. 8 gy + 7, which are the plane's rows h - 8 (gy + 1) .. h - 1 - 8 gy: the origin is negative for the
// top, partial, group row.  Every other pixel of the four output planes keeps its words.  A list entry that names no group is skipped by the whole
// workgroup, ahead of the first barrier.
template <int P>
__global__ void __launch_bounds__(kDnLanes) rt_denoise_pair_tiles_kernel(float *__restrict__ out_a, float *__restrict__ out_b, uint32_t *__restrict__ px_a,
                                                                         uint32_t *__restrict__ px_b, const float *__restrict__ a,
                                                                         const float *__restrict__ b, const float *__restrict__ vs, int w, int h, int R,
                                                                         float alpha, float kk, int fast_a, int fast_b, const uint32_t *__restrict__ list,
                                                                         uint32_t groups_x, uint32_t n_groups) {
    extern __shared__ float dn_lds[];
    const uint32_t g = list[blockIdx.x];
    if (g >= n_groups) return;
    const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
    dn_pair_body<P, true>(dn_lds, (int)gx * kDnTileW, h - kDnTileH * ((int)gy + 1), out_a, out_b, px_a, px_b, a, b, vs, w, h, R, alpha, kk, fast_a, fast_b);
}

// The groups of a selection as a list: the indices g with selected[g] != 0 in ascending order -- a stable compaction by ONE workgroup, chunk by chunk,
// as rt_tile_list_kernel builds the render's tile list (rt_tiles.hip): wave ballot + mbcnt inside the wavefront, the sixteen wave totals through LDS,
// a running base.  Entries from the count up to `slots` get the sentinel n (no group).
__global__ void __launch_bounds__(1024) rt_group_list_kernel(const uint32_t *__restrict__ selected, uint32_t n, uint32_t *__restrict__ list, uint32_t slots) {
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    uint32_t base = 0;                                      // (the same in every lane)
    for (uint32_t first = 0; first < n; first += 1024u) {
        const uint32_t g = first + tid;
        const bool keep = g < n && selected[g] != 0u;
        const unsigned long long mask = __ballot(keep);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if ((tid & 63u) == 0u) s_wave[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t at = base, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) {
            const uint32_t c_ = s_wave[v];
            at += v < wave ? c_ : 0u;
            total += c_;
        }
        if (keep && at + before < slots) list[at + before] = g;
        base += total;
        __syncthreads();                                    // (s_wave is written again by the next chunk)
    }
    for (uint32_t k = base + tid; k < slots; k += 1024u) list[k] = n;
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

namespace {

std::atomic<uint64_t> g_pair_calls{0};                     // numbers the rt_denoise_pair_async calls of the process (FrameState::filtered_pair)

size_t denoise_pair_lds_bytes(int R, int P) {
    const int H = R + P;
    return ((size_t)9 * (kDnTileW + 2 * H) * (kDnTileH + 2 * H) + (size_t)4 * (kDnTileW + 2 * P) * (kDnTileH + 2 * P)) * sizeof(float);
}

bool packs_fast(const rt_ctx *c) { return c->mode == RT_MODE_FAST || c->mode >= 200; }     // which pack kernel refresh_pixels launches (rt_api.hip)

}  // namespace

namespace rt {

int denoise_pair_refuse(const rt_ctx *a, const rt_ctx *b, const char *call) {
    if (!a || !b) return fail(RT_ERR_ARG, "%s: ctx is null", call);
    int rc = tiles_refuse(a, call);
    if (rc == RT_OK) rc = tiles_refuse(b, call);
    if (rc == RT_OK) rc = same_frame(a, b, call, "the first half", "the second half", false);
    if (rc != RT_OK) return rc;
    if (a->frame.current_sample != b->frame.current_sample)
        return fail(RT_ERR_STATE, "%s: the halves hold %d and %d passes", call, a->frame.current_sample, b->frame.current_sample);
    if (a->frame.current_sample <= 0) return fail(RT_ERR_STATE, "%s: the halves hold no pass", call);
    return RT_OK;
}

int denoise_pair(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream) {
    int rc = select_device(a);
    if (rc != RT_OK) return rc;
    const size_t n_floats = color_floats(a), n_words = image_pixels(a);
    for (rt_ctx *c : { a, b }) {
        if (!c->d_filtered) HIP_TRY(hipMalloc(&c->d_filtered, n_floats * sizeof(float)));
        if (!c->d_filtered_px) HIP_TRY(hipMalloc(&c->d_filtered_px, n_words * sizeof(uint32_t)));
    }
    if (!a->d_denoise_var) HIP_TRY(hipMalloc(&a->d_denoise_var, n_floats * sizeof(float)));
    // behind everything the two contexts have queued; their later work behind the filter
    rc = chain(a, stream);
    if (rc == RT_OK) rc = chain(b, stream);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(rt_denoise_variance_kernel, dim3((unsigned)((3 * (size_t)a->w + 255) / 256), (unsigned)std::min(a->h, 65535)), dim3(256), 0, stream,
                       a->d_denoise_var, a->d_colors, b->d_colors, a->w, a->h);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((a->w + kDnTileW - 1) / kDnTileW), (unsigned)((a->h + kDnTileH - 1) / kDnTileH));
    const size_t lds = denoise_pair_lds_bytes(q.search_radius, q.patch_radius);
    const float kk = q.k * q.k;
    const int fast_a = packs_fast(a), fast_b = packs_fast(b);
#define RT_PAIR_LAUNCH(P)                                                                                                                                     \
    hipLaunchKernelGGL(rt_denoise_pair_kernel<P>, grid, dim3(kDnLanes), lds, stream, a->d_filtered, b->d_filtered, a->d_filtered_px, b->d_filtered_px,          \
                       a->d_colors, b->d_colors, a->d_denoise_var, a->w, a->h, q.search_radius, q.alpha, kk, fast_a, fast_b)
    switch (q.patch_radius) {
    case 0: RT_PAIR_LAUNCH(0); break;
    case 1: RT_PAIR_LAUNCH(1); break;
    default: RT_PAIR_LAUNCH(2); break;
    }
#undef RT_PAIR_LAUNCH
    HIP_TRY(hipGetLastError());
    const uint64_t call = g_pair_calls.fetch_add(1) + 1;
    a->frame.pair_filtered(call);
    b->frame.pair_filtered(call);
    return RT_OK;
}

// The pair kernel over the groups `a` has selected.  Rule 2's plane is formed for the whole frame: it is bandwidth-bound and small beside the filter, and
// the selected groups' halos reach into groups that are not selected.  The list of groups is built once per selection (FrameState::group_list_built).
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
    int rc = select_device(a);
    if (rc != RT_OK) return rc;
    const uint32_t n_groups = group_count(a), m = fa.counts[0];
    if (m == 0 || m > n_groups) return fail(RT_ERR_STATE, "%s: a selection of %u of %u groups has been rendered", call, m, n_groups);
    if (!a->tiles.d_groups) HIP_TRY(hipMalloc(&a->tiles.d_groups, (size_t)n_groups * sizeof(uint32_t)));
    rc = chain(a, stream);
    if (rc == RT_OK) rc = chain(b, stream);
    if (rc != RT_OK) return rc;
    if (fa.group_list_is_stale()) {
        hipLaunchKernelGGL(rt_group_list_kernel, dim3(1), dim3(1024), 0, stream, a->tiles.d_selected, n_groups, a->tiles.d_groups, n_groups);
        HIP_TRY(hipGetLastError());
        a->frame.group_list_built();
    }
    hipLaunchKernelGGL(rt_denoise_variance_kernel, dim3((unsigned)((3 * (size_t)a->w + 255) / 256), (unsigned)std::min(a->h, 65535)), dim3(256), 0, stream,
                       a->d_denoise_var, a->d_colors, b->d_colors, a->w, a->h);
    HIP_TRY(hipGetLastError());
    const size_t lds = denoise_pair_lds_bytes(q.search_radius, q.patch_radius);
    const float kk = q.k * q.k;
    const int fast_a = packs_fast(a), fast_b = packs_fast(b);
#define RT_PAIR_TILES_LAUNCH(P)                                                                                                                               \
    hipLaunchKernelGGL(rt_denoise_pair_tiles_kernel<P>, dim3(m), dim3(kDnLanes), lds, stream, a->d_filtered, b->d_filtered, a->d_filtered_px,                  \
                       b->d_filtered_px, a->d_colors, b->d_colors, a->d_denoise_var, a->w, a->h, q.search_radius, q.alpha, kk, fast_a, fast_b,                  \
                       a->tiles.d_groups, groups_per_row(a), n_groups)
    switch (q.patch_radius) {
    case 0: RT_PAIR_TILES_LAUNCH(0); break;
    case 1: RT_PAIR_TILES_LAUNCH(1); break;
    default: RT_PAIR_TILES_LAUNCH(2); break;
    }
#undef RT_PAIR_TILES_LAUNCH
    HIP_TRY(hipGetLastError());
    const uint64_t id = g_pair_calls.fetch_add(1) + 1;
    a->frame.pair_tiles_refreshed(id);
    b->frame.pair_tiles_refreshed(id);
    return RT_OK;
}

}  // namespace rt

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
