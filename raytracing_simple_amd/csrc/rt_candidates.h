// rt_candidates.h -- which spheres the camera rays of one 8x8 pixel tile can reach: the certificate behind
// RT_OPT_DIRECT_CAMERA (rt_trace.inc.h).  Plain host / device functions of binary32 arithmetic and sqrtf: the same
// text runs in the kernels' prologue (lane i classifies sphere i, one wave ballot makes the tile's candidate mask)
// and on the CPU (rt_debug_tile_candidates, tests/test_tile_candidates.py).  Stateless: nothing is stored between
// launches, so scene updates, camera changes, resumed or merged frames and sharded contexts need no invalidation.
//
// Geometry.  A sample of pixel (px, py) has the direction rd = cam.d + cam.x * kcx + cam.y * kcy with
// kcx = (px + j1) / w - 0.5, kcy = (py + j2) / h - 0.5 and jitters in [-0.5, 0.5) (rt_shade.inc.h camera_coord), its
// origin is cam.o + 0.1 * rd.  So every ray of the tile lies on a line through cam.o, and the lines' directions are
// axis + cam.x * dx + cam.y * dy with axis the direction through the centre of the tile's coordinate rectangle and
// |dx| <= hx, |dy| <= hy its half edges: they lie inside the (double) cone of apex cam.o around the axis with
// half-angle alpha, sin alpha <= (hx |cam.x| + hy |cam.y|) / |axis|.  A sphere of radius r at distance L from cam.o
// is seen under the half-angle beta = asin(r / L).  With theta the angle between the axis and the centre, a line of
// the cone passes the centre at an angle phi in [theta - alpha, theta + alpha], and it misses the sphere iff
// sin phi > sin beta.  The rule: the sphere is a MISS only if
//        gamma < theta < pi - gamma,   gamma = alpha + beta + margin < pi / 2,
// evaluated without inverse trigonometric functions as  S cos(gamma) - |C| sin(gamma) > 0  with S = |axis x oc| and
// C = axis . oc (sin(theta -+ gamma) > 0; sin and cos of gamma from the addition theorems).  Everything else is a
// CANDIDATE -- a non-finite record or camera, a camera inside or near the surface of the sphere, a radius^2 that is
// not positive, a wide tile (sin alpha >= 0.5), a comparison that fails on NaN -- and a candidate is always correct
// to test: the kernel applies the reference's own test to it.
//
// The margin.  For a MISS every line of the tile passes the centre at phi with beta + m <= phi <= pi - beta - m, so the
// exact discriminant of the kernel's test, det = r^2 - L^2 sin^2(phi), is at most
//        L^2 (sin^2(beta) - sin^2(beta + m)) = -L^2 sin(2 beta + m) sin(m) <= -L^2 sin^2(m)       (2 beta + m <= pi - m).
// What the kernel computes is det = b * b - op . op + r^2 in binary32 with op = centre - o, b = op . d:
//   - the products and sums: at most about 12 * 2^-24 (b^2 + |op|^2) <= 2^-20 L'^2 with L' = |op| <= L + 0.1 |rd|;
//     the rule demands L >= 0.15 |axis| >= 0.1 |rd|, so L' <= 2 L and this part is below 4e-6 L^2;
//   - the rounding of o = cam.o + 0.1 rd, of op's differences and of d's unit length: op is off by at most about
//     5 * 2^-24 M with M the largest coordinate involved, which moves det by at most 2 L' times that; the rule demands
//     M <= 16 L, which keeps this part below 2e-5 L^2;
//   - the certificate's own binary32 rounding (a few 1e-6 rad, covered by a slack of 1e-5 |axis| L in the comparison and by
//     the widened coordinate rectangle) and the rounding of camera_coord (below 2^-22, the rectangle is widened by 2^-20).
// Together below 2.5e-5 L^2, against sin^2(m) L^2: m = 1e-3 rad gives 1e-6 L^2 -- NOT enough; m = 0.01 rad gives 1e-4 L^2,
// four times the error bound.  (Measured on the kernels' own arithmetic: tests/test_tile_candidates.py prints the
// smallest -det / L^2 it sees.)
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_CAND_HD __host__ __device__ inline
#else
#define RT_CAND_HD inline
#endif

namespace rt {

constexpr float kCandSinMargin = 0.0099998333f;     // sin and cos of the margin, 0.01 rad
constexpr float kCandCosMargin = 0.99995000f;
constexpr uint32_t kCandMaxSpheres = 64;            // one lane, one mask bit per sphere: larger scenes run without the certificate
constexpr uint32_t kCandPacked = 4;                 // candidate indices a wavefront keeps (rt_trace.inc.h): tiles with more run the old loop, camera rays through the sweep

struct CandCamera {
    float o[3], d[3], x[3], y[3];                   // rt_camera's orig, dir, x, y
    float inv_w, inv_h;
};

RT_CAND_HD bool cand_finite(float v) { return fabsf(v) <= 3.4028234e38f; }      // (false for NaN)

// true unless NO camera ray of the pixels [x0, x1] x [y0, y1] (image coordinates, inclusive) can have a non-negative
// discriminant against the sphere g = { centre, radius^2 }
RT_CAND_HD bool tile_sphere_candidate(const CandCamera &c, int x0, int x1, int y0, int y1, float gx, float gy, float gz, float r2) {
    // the tile's rectangle of image-plane coordinates, widened for the rounding of camera_coord
    const float kx_lo = ((float)x0 - 0.5f) * c.inv_w - 0.5f, kx_hi = ((float)x1 + 0.5f) * c.inv_w - 0.5f;
    const float ky_lo = ((float)y0 - 0.5f) * c.inv_h - 0.5f, ky_hi = ((float)y1 + 0.5f) * c.inv_h - 0.5f;
    const float kcx = 0.5f * (kx_lo + kx_hi), kcy = 0.5f * (ky_lo + ky_hi);
    const float hx = 0.5f * (kx_hi - kx_lo) + 0x1p-20f, hy = 0.5f * (ky_hi - ky_lo) + 0x1p-20f;
    const float ax = c.d[0] + c.x[0] * kcx + c.y[0] * kcy;
    const float ay = c.d[1] + c.x[1] * kcx + c.y[1] * kcy;
    const float az = c.d[2] + c.x[2] * kcx + c.y[2] * kcy;
    const float A = sqrtf(ax * ax + ay * ay + az * az);
    const float ex = sqrtf(c.x[0] * c.x[0] + c.x[1] * c.x[1] + c.x[2] * c.x[2]);
    const float ey = sqrtf(c.y[0] * c.y[0] + c.y[1] * c.y[1] + c.y[2] * c.y[2]);
    const float E = hx * ex + hy * ey;
    const float ox = gx - c.o[0], oy = gy - c.o[1], oz = gz - c.o[2];
    const float L2 = ox * ox + oy * oy + oz * oz;
    const float L = sqrtf(L2);
    // every input finite (sums of finite values that overflowed count as non-finite too)
    if (!(cand_finite(A) && cand_finite(E) && cand_finite(L2) && cand_finite(r2) && cand_finite(c.o[0]) && cand_finite(c.o[1]) &&
          cand_finite(c.o[2])))
        return true;
    if (!(A > 0.f && r2 > 0.f)) return true;
    const float sa = E / A;
    if (!(sa < 0.5f)) return true;                                  // a narrow cone only
    if (!(L2 > r2 * 1.001f)) return true;                           // the camera provably outside the sphere
    if (!(L >= 0.15f * A)) return true;                             // |op| <= 2 L for every ray origin (the margin's derivation)
    const float M = fmaxf(fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz)),
                          fmaxf(fmaxf(fabsf(c.o[0]), fabsf(c.o[1])), fabsf(c.o[2])) + 0.15f * A);
    if (!(M <= 16.f * L)) return true;                              // coordinates no larger than the rounding bound assumes
    const float ca = sqrtf(1.f - sa * sa);
    const float sb = sqrtf(r2) / L;
    const float cb = sqrtf(L2 - r2) / L;
    const float s_ab = sa * cb + ca * sb, c_ab = ca * cb - sa * sb;
    const float sg = s_ab * kCandCosMargin + c_ab * kCandSinMargin;
    const float cg = c_ab * kCandCosMargin - s_ab * kCandSinMargin;
    if (!(cg > 0.f)) return true;                                   // gamma below a right angle
    const float qx = ay * oz - az * oy, qy = az * ox - ax * oz, qz = ax * oy - ay * ox;
    const float S = sqrtf(qx * qx + qy * qy + qz * qz);
    const float C = ax * ox + ay * oy + az * oz;
    const bool miss = S * cg - fabsf(C) * sg > 1e-5f * A * L;        // (false on NaN)
    return !miss;
}

// Local row -> image row of a rank's row tiles (rt_shade.inc.h pixel_at)
RT_CAND_HD int cand_image_row(int lrow, int rank, int nranks, int tile_rows) {
    const int tile = lrow / tile_rows;
    return (tile * nranks + rank) * tile_rows + (lrow - tile * tile_rows);
}

}  // namespace rt
