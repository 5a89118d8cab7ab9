// rt_atrous_prepare_body.inc.h -- the STATEMENTS of the a-trous preparation kernel (rules 20-21, and rule 28 in the moments arm), included between the
// braces of rt_atrous_prepare_kernel<kCh> (rt_atrous.hip) and of rt_atrous_prepare_moments_kernel (rt_moments.hip): one text, and -- because it is text
// and no function that a kernel inlines -- the kernels without the arm compile to the machine code they had before the arm existed.  The including
// function provides the kernel's arguments under the names used below, kCh, and a constant kMom: false discards the arm (m and k_min are then constants
// nobody reads); true reads words 2-3 of the lane's own texel of the moments plane and selects between its v and rule 21's result.
// Bounds: rt_atrous.hip states those of rules 20-21.  The arm reads m at `at`, the lane's own pixel, x < w && y < h: ONE 8-byte load.
    const auto [x, y] = plane_pixel();
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const float4 up = plane_texel<kCh>(u, at, n_all);
    const float4 f_lo = feat[2 * at], f_hi = feat[2 * at + 1];
    const uint32_t id = __float_as_uint(f_hi.w);
    // rule 21
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const size_t aq = (size_t)qy * (size_t)w + (size_t)qx;
            if (__float_as_uint(feat[2 * aq + 1].w) != id) continue;
            const float4 uq = plane_texel<kCh>(u, aq, n_all);
            if (!rt::usable(uq.x, uq.y, uq.z, uq.w)) continue;
            const float l = rt::luminance(uq.x, uq.y, uq.z);
            s0 = s0 + 1.0f;
            s1 = s1 + l;
            s2 = s2 + l * l;
        }
    float v0 = rt::variance_of_sums(s0, s1, s2);
    const bool usable = rt::usable(up.x, up.y, up.z, up.w);      // rule 20
    if constexpr (kMom) {
        const float2 kv = m[2 * at + 1];                         // (k, v): words 2-3 of M[p]
        v0 = rt::variance_from_history(usable, kv.x, kv.y, k_min, v0);      // rule 28
    }
    out[at] = make_float4(up.x, up.y, up.z, v0);
    guide[at] = make_float4(f_lo.w, f_hi.x, f_hi.y, f_hi.w);
    n_out[at] = usable ? up.w : 0.0f;
    if (px) px[(size_t)(h - 1 - y) * (size_t)w + (size_t)x] = pack_rgb(up.x, up.y, up.z, fast != 0);
