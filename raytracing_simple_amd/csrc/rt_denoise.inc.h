// rt_denoise.inc.h -- the NL-means device body the filter kernels share (include/rt_api.h, "denoising", "the error of the filtered frame", "feature
// planes"): included by rt_denoise.hip, whose kernels filter by colour alone or, kGuided, add the guide of rules 13-14.
// The workgroup's shape and the pack are rt_plane.inc.h's (a workgroup's 32x8 output pixels: a row of 32 per half-wave here); the arithmetic of rules
// 3, 5 and 13 is rt_rules.h's.
// The unit is compiled with -ffp-contract=off: every multiply, add and IEEE division below is an operation of its own, in the written order.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt_internal.h"
#include "rt_plane.inc.h"

namespace {

__device__ __forceinline__ int dn_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// What a filter kernel reads and writes per image: the plane, the filtered plane, and -- the halves only -- the filtered plane packed by the toInt
// of that context's mode
template <int N>
struct DnPlanes {
    const float *img[N];
    float *out[N];
    uint32_t *px[N];
    int fast[N];
};

// What a GUIDED filter kernel reads besides ("feature planes", rules 13-14): the feature plane of the first half, 8 words per pixel as two float4, and
// 1 / k^2 of the three features
struct DnGuide {
    const float4 *feat;
    float ia, in, id;
};

}  // namespace

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
// kGuided (rules 13-14): behind the buffers, words 0-6 of the feature plane for the tile and its R-halo -- rule 13 is per pixel, the patch halo is not
//   needed -- as seven planes of FW x FH = (32 + 2R) x (8 + 2R) floats, entry (fy, fx) = F at cl(y0 - R + fy, x0 - R + fx): 28 (32 + 2R)(8 + 2R) bytes
//   more, 91 584 in all for N = 2 at R 8, P 2 (the host raises the dynamic limit beyond 64 KiB).  The output pixel's own seven values stay in registers;
//   a partner q = p + o that rule 5 has not skipped lies inside the image and within R of the tile, so inside that window.  ONE wf per offset serves
//   every image.  The instances without it compile to the instructions they had before the parameter existed (tools/isa_compare.py).
template <int P, int N, bool kAnyRow, bool kGuided = false>
__device__ __forceinline__ void dn_body(float *dn_lds, const int x0, const int y0, const DnPlanes<N> &k, const float *__restrict__ vs, int w, int h, int R,
                                        float alpha, float kk, const DnGuide gd = DnGuide{}) {
    constexpr int EW = kPlaneTileW + 2 * P, EH = kPlaneTileH + 2 * P, EN = EW * EH;      // 256 / 340 / 432 positions: at most two per lane
    const int H = R + P, LW = kPlaneTileW + 2 * H, LH = kPlaneTileH + 2 * H, LN = LW * LH;
    float *const sI = dn_lds, *const sV = dn_lds + 3 * N * LN, *const sE = dn_lds + 3 * (N + 1) * LN;     // image i, channel c: sI + (3 i + c) LN
    const int tid = (int)threadIdx.x;
    const int wx0 = x0 - H, wy0 = y0 - H;                   // the window's origin in the plane
    const int FW = kPlaneTileW + 2 * R, FN = FW * (kPlaneTileH + 2 * R), fx0 = x0 - R, fy0 = y0 - R;        // kGuided: the feature window
    float *const sF = sE + 2 * N * EN;                      // feature word c: sF + c * FN

    for (int l = tid; l < LN; l += kPlaneLanes) {
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
    if constexpr (kGuided) {
        for (int l = tid; l < FN; l += kPlaneLanes) {
            const int fy = l / FW, fx = l - fy * FW;
            const size_t at = (size_t)dn_clamp(fy0 + fy, h) * (size_t)w + (size_t)dn_clamp(fx0 + fx, w);
            const float4 lo = gd.feat[2 * at], hi = gd.feat[2 * at + 1];
            sF[l] = lo.x, sF[FN + l] = lo.y, sF[2 * FN + l] = lo.z, sF[3 * FN + l] = lo.w;
            sF[4 * FN + l] = hi.x, sF[5 * FN + l] = hi.y, sF[6 * FN + l] = hi.z;
        }
    }
    __syncthreads();

    // this lane's positions of the tile and its P-halo: plane coordinates (clamped), and what rule 3 reads of the position itself
    int ex[2], ey[2];
    float pi[2][N][3], pv[2][3];
    bool have[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        have[s] = tid + s * kPlaneLanes < EN;
        const int idx = have[s] ? tid + s * kPlaneLanes : 0, iy = idx / EW, ix = idx - iy * EW;
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

    const int tx = tid & (kPlaneTileW - 1), ty = tid / kPlaneTileW, px = x0 + tx, py = y0 + ty;
    const bool inside = px < w && py < h && (!kAnyRow || py >= 0);
    const float inv = 1.0f / (float)(3 * (2 * P + 1) * (2 * P + 1));
    float pf[7];                                            // kGuided: the pixel's own feature words (a lane outside the image: those of the clamped pixel)
    if constexpr (kGuided) {
        const int l = (dn_clamp(py, h) - fy0) * FW + (dn_clamp(px, w) - fx0);
#pragma unroll
        for (int c = 0; c < 7; ++c) pf[c] = sF[c * FN + l];
    }
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
                        const float off = rt::nlm_offset(alpha, pv[s][c], qv), dnm = rt::nlm_denominator(kk, pv[s][c], qv);
#pragma unroll
                        for (int g = 0; g < N; ++g) d[g][c] = rt::nlm_term(pi[s][g][c] - sI[(3 * g + c) * LN + l], off, dnm);
                    }
#pragma unroll
                    for (int g = 0; g < N; ++g) e[g * EN + tid + s * kPlaneLanes] = (d[g][0] + d[g][1]) + d[g][2];
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
                        take[i] = T == T && rt::finite3(q[i][0], q[i][1], q[i][2]);
                        const float g = T > 0.f ? T : 0.f;
                        wgt[i] = rt::falloff(g);
                    }
                    if constexpr (kGuided) {
                        const int fl = (qy - fy0) * FW + (qx - fx0);
                        float df[7];
#pragma unroll
                        for (int c = 0; c < 7; ++c) df[c] = sF[c * FN + fl];
                        const float wf = rt::guide_weight(pf, df, gd.ia, gd.in, gd.id);      // rule 13
#pragma unroll
                        for (int i = 0; i < N; ++i) wgt[i] = wf < wgt[i] ? wf : wgt[i];      // rule 14
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
            // (pack_rgb, written out: called here, the pair kernels' stores and the other image's divisions are scheduled differently -- profiles/HISTORY.md)
            k.px[i][(size_t)(h - 1 - py) * (size_t)w + (size_t)px] = dn_to_int(f0, fast) | (dn_to_int(f1, fast) << 8) | (dn_to_int(f2, fast) << 16);
        }
    }
}

namespace {

size_t dn_lds_bytes(int N, int R, int P, bool guided = false) {      // dn_body's layout (its own name: rt::lds_bytes is the sweep's, rt_device.h)
    const int H = R + P;
    return ((size_t)3 * (N + 1) * (kPlaneTileW + 2 * H) * (kPlaneTileH + 2 * H) + (size_t)2 * N * (kPlaneTileW + 2 * P) * (kPlaneTileH + 2 * P) +
            (guided ? (size_t)7 * (kPlaneTileW + 2 * R) * (kPlaneTileH + 2 * R) : 0)) * sizeof(float);
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

}  // namespace
