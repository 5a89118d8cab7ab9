// rt_compare.hip -- frame error on the device (include/rt_api.h, "frame error"): how far apart the packed frames of two contexts are,
// as exact integer sums over the 8-bit channels, without a read-back --
//   rt_compare_async / rt_compare   per-channel squared error, differing pixels, largest difference, and a map of the error per 8x8 tile
//   rt_compare_tiles                the shape of that map
//   rt_error_psnr                   the PSNR those sums stand for (host arithmetic, no device)
//   rt_render_converged             two contexts rendered in step until the PSNR between them reaches a target
//   rt_compare_filtered(_async)     the same metric and map over the packed cross-filtered planes of rt_denoise_pair_async (rt_denoise.hip)
//   rt_render_converged_filtered    ... and the same loop (and rt_render_adaptive's, rt_tiles.hip's calls) with that figure as the check
//   rt_render_adaptive_filtered_tiles   ... the adaptive one with every check after the first filtering only the groups that were just rendered
// The difference between two independent N-pass renders of one scene is the standard estimate of an N-pass render's noise.  The reference
// has one seed stream and compares nothing: this is the library's own extension and reproduces no reference frame.
// The render kernels are not touched: the call reads the buffers their launches write (after the pack kernel, if the pixel store was off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "rt_internal.h"

using rt::fail;

extern "C" int rt_host_denoise_params(const rt_denoise_params *p, rt_denoise_params *out);     // rt_host.cpp: the parameter rules (null = defaults)

namespace rt {
constexpr int kCmpLanes = 128;                  // a workgroup: two wavefronts
constexpr int kCmpCols = 4;                     // adjacent columns a lane owns: 16 bytes of either frame per row
constexpr int kCmpRun = kCmpLanes * kCmpCols;   // columns a workgroup covers at a time (a multiple of the tile width)
static_assert(kCmpRun % 8 == 0 && 8 % kCmpCols == 0, "a tile's columns belong to whole lanes of one wavefront");
}  // namespace rt

// What one pixel adds: squared differences per channel, the count of differing pixels, the largest difference.
struct rt_cmp_sums {
    uint32_t s0 = 0, s1 = 0, s2 = 0, cnt = 0, max_abs = 0;
    __device__ __forceinline__ void add(uint32_t p, uint32_t q) {
        const int d0 = (int)(p & 255u) - (int)(q & 255u);
        const int d1 = (int)((p >> 8) & 255u) - (int)((q >> 8) & 255u);
        const int d2 = (int)((p >> 16) & 255u) - (int)((q >> 16) & 255u);
        s0 += (uint32_t)(d0 * d0);
        s1 += (uint32_t)(d1 * d1);
        s2 += (uint32_t)(d2 * d2);
        cnt += ((p ^ q) & 0x00ffffffu) != 0u ? 1u : 0u;
        max_abs = max(max_abs, (uint32_t)max(max(abs(d0), abs(d1)), abs(d2)));
    }
};

// One pass over both frames.  A workgroup takes a strip of 8 local rows by kCmpRun columns at a time (grid-stride over the strips); a lane owns
// kCmpCols adjacent columns and walks the 8 rows, so every row read of a wavefront is one contiguous segment.  The two lanes of a tile add up
// by a shuffle and one of them stores the tile's word; the frame's totals stay in registers over all strips of the workgroup, are added up
// across the wavefront by shuffles and across the workgroup through LDS, and leave as one 64-bit atomic add per channel, one for the count and
// one atomic maximum: integer atomics, so the result does not depend on the order.  `result` was cleared on the stream before the launch.
__global__ void __launch_bounds__(rt::kCmpLanes) rt_compare_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int w, int rows,
                                                                 unsigned long long *result, uint32_t *tiles) {
    const int lane = threadIdx.x;
    const int runs = (w + rt::kCmpRun - 1) / rt::kCmpRun, strips = (rows + 7) / 8, tiles_x = (w + 7) / 8;
    unsigned long long sq0 = 0, sq1 = 0, sq2 = 0, differing = 0;
    uint32_t max_abs = 0;
    for (int item = blockIdx.x; item < strips * runs; item += gridDim.x) {
        const int strip = item / runs, x0 = (item - strip * runs) * rt::kCmpRun + lane * rt::kCmpCols;
        const int n = min(w - x0, rt::kCmpCols);                // columns of this lane inside the image (<= 0: none)
        const int y0 = strip * 8, ny = min(rows - y0, 8);
        // Rows start at any multiple of 4 bytes (w = 41: row 1 at byte 164), so the 16-byte loads are of 4-byte alignment -- gfx950's global
        // loads take that.  A lane that reaches over the row's end reads its one to three pixels word by word: nothing past a row is touched.
        rt_cmp_sums t;                                          // this strip: at most 8 * 4 * 255^2 per channel
        const size_t at = (size_t)y0 * (size_t)w + (size_t)x0;
        if (n == rt::kCmpCols) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (r >= ny) break;
                uint4 p, q;
                __builtin_memcpy(&p, a + at + (size_t)r * (size_t)w, sizeof p);
                __builtin_memcpy(&q, b + at + (size_t)r * (size_t)w, sizeof q);
                t.add(p.x, q.x);
                t.add(p.y, q.y);
                t.add(p.z, q.z);
                t.add(p.w, q.w);
            }
        } else if (n > 0) {
            for (int r = 0; r < ny; ++r)
                for (int k = 0; k < n; ++k) t.add(a[at + (size_t)r * (size_t)w + k], b[at + (size_t)r * (size_t)w + k]);
        }
        max_abs = max(max_abs, t.max_abs);
        if (tiles) {                                            // (wave-uniform; every lane takes part in the shuffle)
            uint32_t sum = t.s0 + t.s1 + t.s2;                  // at most 8 * 4 * 3 * 255^2
            sum += __shfl_xor(sum, 1);
            if ((lane & 1) == 0 && n > 0) tiles[(size_t)strip * (size_t)tiles_x + (size_t)(x0 >> 3)] = sum;
        }
        sq0 += t.s0;
        sq1 += t.s1;
        sq2 += t.s2;
        differing += t.cnt;
    }
    // the frame's totals: across the wavefront by shuffles ...
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sq0 += __shfl_xor(sq0, m);
        sq1 += __shfl_xor(sq1, m);
        sq2 += __shfl_xor(sq2, m);
        differing += __shfl_xor(differing, m);
        max_abs = max(max_abs, (uint32_t)__shfl_xor((int)max_abs, m));
    }
    // ... across the workgroup through LDS, and one set of atomics per workgroup
    __shared__ unsigned long long part[rt::kCmpLanes / 64][5];
    if ((lane & 63) == 0) {
        unsigned long long *mine = part[lane >> 6];
        mine[0] = sq0;
        mine[1] = sq1;
        mine[2] = sq2;
        mine[3] = differing;
        mine[4] = max_abs;
    }
    __syncthreads();
    if (lane == 0) {
        unsigned long long tot[5] = { 0, 0, 0, 0, 0 };
        for (int v = 0; v < rt::kCmpLanes / 64; ++v) {
            for (int k = 0; k < 4; ++k) tot[k] += part[v][k];
            tot[4] = max(tot[4], part[v][4]);
        }
        for (int k = 0; k < 4; ++k)
            if (tot[k]) atomicAdd(result + k, tot[k]);          // rt_frame_error: sq_err[0..2], differing
        if (tot[4]) atomicMax(reinterpret_cast<uint32_t *>(result + 5), (uint32_t)tot[4]);     // max_abs
        if (blockIdx.x == 0) result[4] = (unsigned long long)rows * (unsigned long long)w;     // pixels (a plain store: nothing else writes it)
    }
}

using namespace rt;

namespace {

static_assert(sizeof(rt_frame_error) == 48, "rt_frame_error is 48 bytes, no padding");


// What a comparison reads: the packed frames of the two contexts, or the packed cross-filtered planes rt_denoise_pair_async left beside them.
enum class Of { Frames, FilteredPlanes };

// the pair is checked: queue the comparison on `stream`, behind everything both contexts have queued, their later work behind it
int compare_on(rt_ctx *a, rt_ctx *b, rt_frame_error *result_dev, uint32_t *tiles_dev, hipStream_t stream, Of what = Of::Frames) {
    int rc = select_device(a);
    if (rc != RT_OK) return rc;
    RT_TRY(chain_all(stream, { a, b }));
    HIP_TRY(hipMemsetAsync(result_dev, 0, sizeof(rt_frame_error), stream));     // the accumulators; the whole answer of a context without rows
    if (a->local_rows == 0) return RT_OK;
    if (what == Of::Frames) {
        rc = refresh_pixels(a, stream);
        if (rc == RT_OK) rc = refresh_pixels(b, stream);
        if (rc != RT_OK) return rc;
    }
    const uint32_t *pa = what == Of::Frames ? frame_pixels(a) : a->planes.filtered_px, *pb = what == Of::Frames ? frame_pixels(b) : b->planes.filtered_px;
    const size_t items = (size_t)tile_row_count(a) * (size_t)((a->w + kCmpRun - 1) / kCmpRun);
    const size_t blocks = std::min(items, (size_t)a->knobs.n_cus * 8);
    hipLaunchKernelGGL(rt_compare_kernel, dim3((unsigned)blocks), dim3(kCmpLanes), 0, stream, pa, pb, a->w, a->local_rows, reinterpret_cast<unsigned long long *>(result_dev), tiles_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// the blocking calls' scratch on a's device: one rt_frame_error, then the tile map
int ensure_scratch(rt_ctx *a) {
    return ensure_device(a->owned, reinterpret_cast<unsigned char **>(&a->d_compare), sizeof(rt_frame_error) + std::max<size_t>(tile_count(a), 1) * sizeof(uint32_t));
}

// rt_compare: on a's own stream through a's scratch, then the wait
int compare_blocking(rt_ctx *a, rt_ctx *b, rt_frame_error *out_host, uint32_t *tiles_host, Of what = Of::Frames) {
    int rc = select_device(a);
    if (rc == RT_OK) rc = ensure_scratch(a);
    if (rc != RT_OK) return rc;
    rt_frame_error *res = static_cast<rt_frame_error *>(a->d_compare);
    uint32_t *tiles = reinterpret_cast<uint32_t *>(res + 1);
    const bool want_tiles = tiles_host && tile_count(a) > 0;
    rc = compare_on(a, b, res, want_tiles ? tiles : nullptr, a->stream, what);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, res, sizeof *res, hipMemcpyDeviceToHost, a->stream));
    if (want_tiles) HIP_TRY(hipMemcpyAsync(tiles_host, tiles, (size_t)tile_count(a) * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return RT_OK;
}

// what rt_render_converged and rt_render_adaptive ask of their arguments alike: a place for the last check, a step, a target that is a number, and two
// whole frames at one pass number below max_passes that will not render the same image
int check_paired_render(const rt_ctx *a, const rt_ctx *b, const char *call, const rt_frame_error *last, int passes_per_check, double target_db, int max_passes) {
    const int na = a->frame.current_sample, nb = b->frame.current_sample;
    if (!last) return fail(RT_ERR_ARG, "last is null");
    if (passes_per_check < 1) return fail(RT_ERR_ARG, "passes_per_check %d", passes_per_check);
    if (std::isnan(target_db)) return fail(RT_ERR_ARG, "%s: the target in dB is not a number", call);
    if (max_passes < na || max_passes < nb) return fail(RT_ERR_ARG, "max_passes %d is below the passes the contexts hold (%d, %d)", max_passes, na, nb);
    if (na != nb) return fail(RT_ERR_STATE, "%s: the contexts hold %d and %d passes", call, na, nb);
    if (na == 0 && a->frame.on_default_stream() && b->frame.on_default_stream())
        return fail(RT_ERR_STATE, "%s: both contexts are at pass 0 of the default seed stream and would render the same frame "
                                  "(rt_seed_stream_async gives each a stream of its own)", call);
    if (a->frame.ragged || b->frame.ragged)
        return fail(RT_ERR_STATE, "%s: the tiles of a context hold different pass counts after a subset launch (rt_reset makes the frame whole)", call);
    return RT_OK;
}

// what the filter and the subset launches ask of a pair: one frame on one device, neither context sharded
int one_unsharded_frame(const rt_ctx *a, const rt_ctx *b, const char *call) {
    int rc = same_frame(a, b, call, "a", "b");
    if (rc == RT_OK) rc = tiles_refuse(a, call);
    if (rc == RT_OK) rc = tiles_refuse(b, call);
    return rc;
}

// the pair rt_compare_filtered* takes: that, both planes current and made by one rt_denoise_pair_async call
int check_filtered_pair(const rt_ctx *a, const rt_ctx *b, const char *call) {
    const int rc = one_unsharded_frame(a, b, call);
    if (rc != RT_OK) return rc;
    if (!a->frame.filtered_with(b->frame))
        return fail(RT_ERR_STATE, "%s: the cross-filtered planes are not current, or were not made by one rt_denoise_pair_async call (whatever moves a colour plane ends its plane)", call);
    return RT_OK;
}

// What a check of the two paired loops compares.  filter == null: the packed frames, as they are.  Else: rt_denoise_pair_async with these
// (checked) parameters on `stream` first, then its packed planes -- the estimate of the FILTERED frame's error.  `rendered_only`: not that call but
// rt_denoise_pair_tiles_async -- the planes of the groups the selection in hand has just rendered, the other groups' as their last check left them.
int check_on(rt_ctx *a, rt_ctx *b, const rt_denoise_params *filter, rt_frame_error *result_dev, uint32_t *tiles_dev, hipStream_t stream,
             bool rendered_only = false) {
    if (!filter) return compare_on(a, b, result_dev, tiles_dev, stream);
    const char *call = rendered_only ? "rt_denoise_pair_tiles_async" : "rt_denoise_pair_async";
    int rc = denoise_pair_refuse(a, b, call);
    if (rc == RT_OK) rc = rendered_only ? denoise_pair_tiles(a, b, *filter, stream, call) : denoise_pair(a, b, *filter, stream);
    if (rc == RT_OK) rc = compare_on(a, b, result_dev, tiles_dev, stream, Of::FilteredPlanes);
    return rc;
}

// the filtered loops' own refusals, ahead of the shared ones: contexts the filter does not take, parameters it does not take (`q`: the checked copy)
int check_filtered_loop(const rt_ctx *a, const rt_ctx *b, const char *call, const rt_denoise_params *p, rt_denoise_params *q) {
    int rc = one_unsharded_frame(a, b, call);
    if (rc == RT_OK && rt_host_denoise_params(p, q) != RT_OK) rc = RT_ERR_ARG;
    return rc;
}

// rt_render_converged and rt_render_converged_filtered: the loop, over what makes the figure
int render_converged(rt_ctx *a, rt_ctx *b, const char *call, const rt_denoise_params *filter, double target_psnr_db, int passes_per_check, int max_passes,
                     rt_frame_error *last, int *checks) {
    int rc = same_frame(a, b, call, "a", "b");
    if (rc == RT_OK) rc = check_paired_render(a, b, call, last, passes_per_check, target_psnr_db, max_passes);
    if (rc == RT_OK && filter) rc = guide_refuse(a, b, call);      // (ahead of the first pass: a refused call changes nothing)
    if (rc == RT_OK) rc = select_device(a);
    if (rc == RT_OK) rc = ensure_scratch(a);
    if (rc != RT_OK) return rc;
    if (checks) *checks = 0;
    rt_frame_error *res = static_cast<rt_frame_error *>(a->d_compare);
    for (int done = 0;; ++done) {
        const int n = std::min(passes_per_check, max_passes - a->frame.current_sample);
        if (n == 0 && done > 0) return 0;                       // max_passes reached: *last is the last check
        if (n > 0) {
            rc = rt_render_async(a, n, a->stream);
            if (rc == RT_OK) rc = rt_render_async(b, n, b->stream);
            if (rc != RT_OK) return rc;
        }
        rc = check_on(a, b, filter, res, nullptr, a->stream);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(last, res, sizeof *res, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
        if (checks) *checks = done + 1;
        if (rt_error_psnr(last) >= target_psnr_db) return 1;
        if (n == 0) return 0;                                   // no pass to render: one check of the frames as they are
    }
}

}  // namespace

extern "C" {

RT_API int rt_compare_tiles(const rt_ctx *c, int *tiles_x, int *tiles_y) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return fail(RT_ERR_ARG, "rt_compare_tiles: a multi-device context cannot be compared");
    const int tx = (int)tiles_per_row(c), ty = (int)tile_row_count(c);
    if (tiles_x) *tiles_x = tx;
    if (tiles_y) *tiles_y = ty;
    return tx * ty;
}

RT_API int rt_compare_async(rt_ctx *a, rt_ctx *b, rt_frame_error *result_dev, uint32_t *tiles_dev, void *hip_stream) {
    int rc = same_frame(a, b, "rt_compare_async", "a", "b");
    if (rc != RT_OK) return rc;
    if (!result_dev) return fail(RT_ERR_ARG, "result_dev is null");
    return compare_on(a, b, result_dev, tiles_dev, (hipStream_t)hip_stream);
}

RT_API int rt_compare(rt_ctx *a, rt_ctx *b, rt_frame_error *out_host, uint32_t *tiles_host) {
    int rc = same_frame(a, b, "rt_compare", "a", "b");
    if (rc != RT_OK) return rc;
    if (!out_host) return fail(RT_ERR_ARG, "out_host is null");
    return compare_blocking(a, b, out_host, tiles_host);
}

RT_API double rt_error_psnr(const rt_frame_error *e) {
    if (!e) {
        (void)fail(RT_ERR_ARG, "the frame error is null");
        return std::numeric_limits<double>::quiet_NaN();
    }
    const double sum = (double)e->sq_err[0] + (double)e->sq_err[1] + (double)e->sq_err[2];
    if (sum == 0.0) return std::numeric_limits<double>::infinity();
    return 10.0 * std::log10(255.0 * 255.0 * 3.0 * (double)e->pixels / sum);
}

RT_API int rt_render_converged(rt_ctx *a, rt_ctx *b, double target_psnr_db, int passes_per_check, int max_passes, rt_frame_error *last, int *checks) {
    return render_converged(a, b, "rt_render_converged", nullptr, target_psnr_db, passes_per_check, max_passes, last, checks);
}

RT_API int rt_render_converged_filtered(rt_ctx *a, rt_ctx *b, double target_psnr_db, int passes_per_check, int max_passes, const rt_denoise_params *p,
                                        rt_frame_error *last, int *checks) {
    rt_denoise_params q;
    const int rc = check_filtered_loop(a, b, "rt_render_converged_filtered", p, &q);
    if (rc != RT_OK) return rc;
    return render_converged(a, b, "rt_render_converged_filtered", &q, target_psnr_db, passes_per_check, max_passes, last, checks);
}

RT_API int rt_compare_filtered_async(rt_ctx *a, rt_ctx *b, rt_frame_error *result_dev, uint32_t *tiles_dev, void *hip_stream) {
    int rc = check_filtered_pair(a, b, "rt_compare_filtered_async");
    if (rc != RT_OK) return rc;
    if (!result_dev) return fail(RT_ERR_ARG, "result_dev is null");
    return compare_on(a, b, result_dev, tiles_dev, (hipStream_t)hip_stream, Of::FilteredPlanes);
}

RT_API int rt_compare_filtered(rt_ctx *a, rt_ctx *b, rt_frame_error *out_host, uint32_t *tiles_host) {
    int rc = check_filtered_pair(a, b, "rt_compare_filtered");
    if (rc != RT_OK) return rc;
    if (!out_host) return fail(RT_ERR_ARG, "out_host is null");
    return compare_blocking(a, b, out_host, tiles_host, Of::FilteredPlanes);
}

// the tile's squared error at which the PSNR over its 192 channel values equals `db`: floor(255^2 * 192 / 10^(db / 10)), kept inside 32 bits
static uint32_t tile_error_at(double db) {
    const double v = std::floor(255.0 * 255.0 * 192.0 / std::pow(10.0, db / 10.0));
    return v >= 4294967295.0 ? 0xffffffffu : (v > 0.0 ? (uint32_t)v : 0u);
}

// rt_render_adaptive, rt_render_adaptive_filtered and rt_render_adaptive_filtered_tiles: the loop, over what makes the map.  `live_checks`: every check
// after the first filters the groups that were just rendered and no others (a retired group is never selected again, so its entry of the map is never
// read again; a live group's planes depend on the colour planes alone)
static int render_adaptive(rt_ctx *a, rt_ctx *b, const char *call, const rt_denoise_params *filter, bool live_checks, double tile_psnr_db, int min_passes,
                           int passes_per_check, int max_passes, rt_frame_error *last, int *checks) {
    int rc = one_unsharded_frame(a, b, call);
    if (rc != RT_OK) return rc;
    if (min_passes < 0) return fail(RT_ERR_ARG, "min_passes %d", min_passes);      // (every refusal ahead of the pass counts' is RT_ERR_ARG: their order does not show)
    rc = check_paired_render(a, b, call, last, passes_per_check, tile_psnr_db, max_passes);
    if (rc == RT_OK && filter) rc = guide_refuse(a, b, call);      // (ahead of the first pass: a refused call changes nothing)
    if (rc != RT_OK) return rc;
    if (checks) *checks = 0;
    rc = select_device(a);
    if (rc == RT_OK) rc = ensure_scratch(a);
    if (rc != RT_OK) return rc;
    // 1. the passes every tile gets, as ordinary full launches
    const int floor_passes = std::min(min_passes, max_passes);
    if (a->frame.current_sample < floor_passes) {
        const int n = floor_passes - a->frame.current_sample;
        rc = rt_render_async(a, n, a->stream);
        if (rc == RT_OK) rc = rt_render_async(b, n, b->stream);
        if (rc != RT_OK) return rc;
    }
    // 2. compare, select on both contexts from the one map, render the selected groups
    const uint32_t above = tile_error_at(tile_psnr_db);
    rt_frame_error *res = static_cast<rt_frame_error *>(a->d_compare);
    uint32_t *map = reinterpret_cast<uint32_t *>(res + 1);
    for (int done = 0;; ++done) {
        rc = check_on(a, b, filter, res, map, a->stream, live_checks && done > 0);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(last, res, sizeof *res, hipMemcpyDeviceToHost, a->stream));
        uint32_t counts_a[2] = { 0, 0 }, counts_b[2] = { 0, 0 };
        rc = rt_select_tiles(a, map, above, a->stream, counts_a);      // (waits for a's stream: *last has landed too)
        if (rc == RT_OK) rc = rt_select_tiles(b, map, above, b->stream, counts_b);
        if (rc != RT_OK) return rc;
        if (checks) *checks = done + 1;
        if (counts_a[0] != counts_b[0] || counts_a[1] != counts_b[1])
            return fail(RT_ERR_STATE, "%s: the contexts selected %u and %u groups from one map (their tile pass counts differ)", call, counts_a[0], counts_b[0]);
        if (counts_a[0] == 0) return 1;                         // every group has retired
        const int n = std::min(passes_per_check, max_passes - a->frame.current_sample);
        if (n == 0) return 0;                                   // max_passes reached with groups still above the target
        rc = rt_render_tiles_async(a, n, a->stream);
        if (rc == RT_OK) rc = rt_render_tiles_async(b, n, b->stream);
        if (rc != RT_OK) return rc;
    }
}

RT_API int rt_render_adaptive(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes, rt_frame_error *last,
                              int *checks) {
    return render_adaptive(a, b, "rt_render_adaptive", nullptr, false, tile_psnr_db, min_passes, passes_per_check, max_passes, last, checks);
}

RT_API int rt_render_adaptive_filtered(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes,
                                       const rt_denoise_params *p, rt_frame_error *last, int *checks) {
    rt_denoise_params q;
    const int rc = check_filtered_loop(a, b, "rt_render_adaptive_filtered", p, &q);
    if (rc != RT_OK) return rc;
    return render_adaptive(a, b, "rt_render_adaptive_filtered", &q, false, tile_psnr_db, min_passes, passes_per_check, max_passes, last, checks);
}

RT_API int rt_render_adaptive_filtered_tiles(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes,
                                             const rt_denoise_params *p, rt_frame_error *last, int *checks) {
    rt_denoise_params q;
    if (rt_host_denoise_params(p, &q) != RT_OK) return RT_ERR_ARG;     // (ahead of the contexts, which render_adaptive checks first: RT_ERR_ARG either way)
    return render_adaptive(a, b, "rt_render_adaptive_filtered_tiles", &q, true, tile_psnr_db, min_passes, passes_per_check, max_passes, last, checks);
}

}  // extern "C"
