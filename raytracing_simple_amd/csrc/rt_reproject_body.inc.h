// rt_reproject_body.inc.h -- the STATEMENTS of the reprojection kernel (rules 15-19, and rules 25-27 in the moments arm), included between the braces of
// rt_reproject_kernel<kCh> (rt_reproject.hip) and of rt_reproject_moments_kernel<kCh, kFromPlane> (rt_moments.hip): one text, and -- because it is text
// and no function that a kernel inlines -- the kernels without the arm compile to the machine code they had before the arm existed.  The including
// function provides the kernel's arguments under the names used below and a constant kMom (rt_plane.inc.h): kNoMoments discards the arm (out_m and m_s
// are then null constants nobody reads), kMomentsOfLuminance takes a tap's moments from the luminance of U (rule 25's fallback), kMomentsOfPlane from
// S's moments plane m_s -- one more float4 load per counted tap beside U's; both store the lane's texel of dst's moments plane as ONE float4.
// Bounds: rt_reproject.hip states those of rules 15-19.  The arm reads m_s only at `aq`, a tap position that passed the in-image test above it (and
// every later test), and writes out_m at `at`, the lane's own pixel, x < w && y < h.  Without kShadow: no LDS, no barrier; never any scratch.
// THE SHADOW ARM (rules 29-32; rt_shadow_history.hip): the including function also provides a constant kShadow and, under it, the pair list `pairs` of
// `n_pairs` records of five float4 (rt_rules.h kShadowPairFloats), `keep`, the flag plane out_k and the LDS block s_pairs of kShadowChunk records;
// without it these are constants nobody reads.  Under kShadow NO LANE LEAVES at the top: a lane outside the image takes the nearest pixel inside it
// -- every load below is then in bounds as stated -- computes what that pixel's lane computes and stores nothing, so that every lane of the workgroup
// reaches both barriers of every chunk.  Only the pair arithmetic and the stores are predicated.
    const auto [lane_x, lane_y] = plane_pixel();
    if constexpr (!kShadow) {
        if (lane_x >= w || lane_y >= h) return;
    }
    [[maybe_unused]] const bool inside = lane_x < w && lane_y < h;
    const int x = kShadow ? min(lane_x, w - 1) : lane_x, y = kShadow ? min(lane_y, h - 1) : lane_y;
    const size_t at = (size_t)(h - 1 - y) * (size_t)w + (size_t)x;
    const float inv_w = 1.f / (float)w, inv_h = 1.f / (float)h, fw = (float)w, fh = (float)h;

    float sw = 0.0f, sn = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f;
    [[maybe_unused]] float s1 = 0.0f, s2 = 0.0f, sk = 0.0f;           // rule 26
    [[maybe_unused]] float px = 0.0f, py = 0.0f, pz = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;       // rule 31: P and Pp, kept for the pairs
    // rule 15: the point and where it was
    const float4 fd_hi = feat_d[2 * at + 1];                 // (words 4-7; words 0-3 of FD are not needed)
    const uint32_t id = __float_as_uint(fd_hi.w);
    if (id < n) {
        const float t = fd_hi.z;
        const rt::PixelRay r = rt::pixel_ray(cam_d, x, y, inv_w, inv_h);       // rule 10
        const float4 gd = geom_d[id], gs = geom_s[id];
        const float ppx = (r.ox + r.dx * t) - (gd.x - gs.x), ppy = (r.oy + r.dy * t) - (gd.y - gs.y), ppz = (r.oz + r.dz * t) - (gd.z - gs.z);
        // rule 16: where S saw it
        if constexpr (kShadow) px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t, wx = ppx, wy = ppy, wz = ppz;
        const float vx = ppx - cam_s.ox, vy = ppy - cam_s.oy, vz = ppz - cam_s.oz;
        const float z = dot3(vx, vy, vz, cam_s.dx, cam_s.dy, cam_s.dz);
        if (z > 0.0f) {
            const float dd = dot3(cam_s.dx, cam_s.dy, cam_s.dz, cam_s.dx, cam_s.dy, cam_s.dz);
            const float xx = dot3(cam_s.xx, cam_s.xy, cam_s.xz, cam_s.xx, cam_s.xy, cam_s.xz);
            const float yy = dot3(cam_s.yx, cam_s.yy, cam_s.yz, cam_s.yx, cam_s.yy, cam_s.yz);
            const float kx = (dot3(vx, vy, vz, cam_s.xx, cam_s.xy, cam_s.xz) * dd) / (z * xx);
            const float ky = (dot3(vx, vy, vz, cam_s.yx, cam_s.yy, cam_s.yz) * dd) / (z * yy);
            const float fx = (kx + 0.5f) * fw, fy = (ky + 0.5f) * fh;
            if (fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                const float x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0;
                const float foot = sqrtf(xx) * (1.f / (float)w);
                // rule 17: the taps
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = (int)x0 + i, qy = (int)y0 + j;
                        const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const size_t aq = (size_t)(h - 1 - qy) * (size_t)w + (size_t)qx;
                        const float4 fs_hi = feat_s[2 * aq + 1];
                        if (__float_as_uint(fs_hi.w) != id) continue;
                        const float tq = fs_hi.z;
                        const rt::PixelRay rq = rt::pixel_ray(cam_s, qx, qy, inv_w, inv_h);
                        const float ex = (rq.ox + rq.dx * tq) - ppx, ey = (rq.oy + rq.dy * tq) - ppy, ez = (rq.oz + rq.dz * tq) - ppz;
                        const float rr = k_pos * (tq * foot);
                        if (!(dot3(ex, ey, ez, ex, ey, ez) <= rr * rr)) continue;
                        const float4 u = plane_texel<kCh>(u_s, aq, ns);
                        if (!rt::usable(u.x, u.y, u.z, u.w)) continue;
                        // rule 18: the history
                        sw = sw + b;
                        sn = sn + b * u.w;
                        sc0 = sc0 + b * u.x;
                        sc1 = sc1 + b * u.y;
                        sc2 = sc2 + b * u.z;
                        if constexpr (kMom != kNoMoments) {
                            // rule 25: the tap's moments; rule 26: their sums
                            float m1q, m2q, kq;
                            if constexpr (kMom == kMomentsOfPlane) {
                                const float4 mq = m_s[aq];
                                m1q = mq.x, m2q = mq.y, kq = mq.z;
                            } else {
                                const float lq = rt::luminance(u.x, u.y, u.z);
                                m1q = lq, m2q = lq * lq, kq = 1.0f;
                            }
                            s1 = s1 + b * m1q;
                            s2 = s2 + b * m2q;
                            sk = sk + b * kq;
                        }
                    }
            }
        }
    }
    const bool have_d = nd != 0.0f;
    [[maybe_unused]] bool flagged = false;
    if constexpr (kShadow) {
        // rule 31: the pairs go through LDS in chunks of kShadowChunk, a barrier either side of a chunk, and are read back at wave-uniform addresses.
        // Bounds: a chunk stages texels [5 * base, 5 * min(base + kShadowChunk, n_pairs)) of a list of 5 * n_pairs and tests exactly those records
        const bool candidate = inside && sw > 0.0f && have_d;         // (history implies a record under the pixel)
        for (uint32_t base = 0; base < n_pairs; base += kShadowChunk) {
            const uint32_t m = min((uint32_t)kShadowChunk, n_pairs - base);
            for (uint32_t i = threadIdx.x; i < 5 * m; i += (uint32_t)kPlaneLanes) s_pairs[i] = pairs[5 * (size_t)base + i];
            __syncthreads();
            if (candidate && !flagged)                                // (a flagged lane skips the arithmetic, never a barrier)
                for (uint32_t i = 0; i < m; ++i) {
                    const float4 lj = s_pairs[5 * i + 4];
                    if (__float_as_uint(lj.x) == id || __float_as_uint(lj.y) == id) continue;
                    const float4 ls = s_pairs[5 * i], ld = s_pairs[5 * i + 1], js = s_pairs[5 * i + 2], jd = s_pairs[5 * i + 3];
                    const int before = rt::shadow_state(wx, wy, wz, ls.x, ls.y, ls.z, ls.w, js.x, js.y, js.z, js.w);      // rule 30
                    const int after = rt::shadow_state(px, py, pz, ld.x, ld.y, ld.z, ld.w, jd.x, jd.y, jd.z, jd.w);
                    flagged = flagged || rt::shadow_changes(before, after);
                }
            __syncthreads();
        }
        if (!inside) return;                                          // (behind the last barrier)
        out_k[at] = flagged ? 1 : 0;
    }
    // rule 19: the blend (D's colour plane is not read at pass 0), with rule 32's cap under kShadow
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (have_d) c0 = col_d[3 * at], c1 = col_d[3 * at + 1], c2 = col_d[3 * at + 2];
    float t0, t1, t2, tn;
    if constexpr (kShadow) rt::temporal_blend_as<true>(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history, flagged, keep);
    else rt::temporal_blend(t0, t1, t2, tn, c0, c1, c2, nd, have_d, sw, sn, sc0, sc1, sc2, max_history);
    out[at] = make_float4(t0, t1, t2, tn);
    out_px[(size_t)y * (size_t)w + (size_t)x] = pack_rgb(t0, t1, t2, fast != 0);
    if constexpr (kMom != kNoMoments) {
        // rule 27: the moments' blend
        float m1, m2, k, v;
        if constexpr (kShadow)
            rt::moments_blend_as<true>(m1, m2, k, v, have_d ? rt::luminance(c0, c1, c2) : 0.0f, nd, have_d, sw, sn, s1, s2, sk, max_history, flagged, keep);
        else rt::moments_blend(m1, m2, k, v, have_d ? rt::luminance(c0, c1, c2) : 0.0f, nd, have_d, sw, sn, s1, s2, sk, max_history);
        out_m[at] = make_float4(m1, m2, k, v);
    }
