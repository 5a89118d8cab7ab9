// rt_tiles.hip -- adaptive sampling (include/rt_api.h, "adaptive sampling"): render only the tiles that are still noisy --
//   rt_select_tiles          an error map (rt_compare_async's) turned into one flag per GROUP of tiles, on the device
//   rt_render_tiles_async    passes on the selected groups and nothing else (the launch itself: rt_launch.hip launch_tiles)
//   rt_tile_passes           the pass count per 8x8 tile
// and the kernels behind them: the selection, the stable compaction that builds a subset launch's tile list, the per-tile pass counts.
// A group is the 8x8 tiles 4g .. 4g+3 of one tile row: 32x8 pixels, the tile of the widest shipped workgroup, so that one-wavefront and
// four-wavefront instances can both render it whole.  Only groups at the FRONT -- pass count == rt_current_sample -- can be selected: the render
// kernels take one first_sample per launch.  The reference renders whole frames only: this is the library's own extension.
// The render kernels are not touched: they take their tile from a list (LaunchParams::order), and a subset launch hands them a shorter list
// and a smaller grid.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_internal.h"

using rt::fail;

// One thread per group.  selected[g] = the group is at the front AND (no map given OR some tile t of it has err[t] * 64 > above * pixels(t)),
// pixels(t) = the image pixels inside tile t (64 but at the right and top edges).  `passes` is null while the context is not ragged: every group
// is at the front then.  counts[0] += selected groups, counts[1] += the 8x8 tiles they cover (cleared on the stream before the launch; integer
// atomics, one pair per wavefront).
__global__ void __launch_bounds__(256) rt_select_tiles_kernel(const uint32_t *__restrict__ err, uint32_t above, const uint32_t *__restrict__ passes,
                                                              uint32_t cur, int w, int rows, uint32_t *__restrict__ selected, uint32_t *counts) {
    const int tiles_x = (w + 7) / 8, tiles_y = (rows + 7) / 8, groups_x = (tiles_x + 3) / 4;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t covered = 0;
    if (g < (uint32_t)(groups_x * tiles_y)) {
        const int ty = (int)(g / (uint32_t)groups_x), tx0 = 4 * (int)(g - (uint32_t)(ty * groups_x));
        const int n = min(4, tiles_x - tx0), ph = min(8, rows - 8 * ty);
        const size_t t0 = (size_t)ty * (size_t)tiles_x + (size_t)tx0;
        bool take = !passes || passes[t0] == cur;           // (a group's tiles hold one count: the first stands for all)
        if (take && err) {
            bool noisy = false;
            for (int k = 0; k < n; ++k) {
                const int pw = min(8, w - 8 * (tx0 + k));
                noisy = noisy || (unsigned long long)err[t0 + k] * 64ull > (unsigned long long)above * (unsigned long long)(pw * ph);
            }
            take = noisy;
        }
        selected[g] = take ? 1u : 0u;
        covered = take ? (uint32_t)n : 0u;
    }
    const uint32_t groups = (uint32_t)__popcll(__ballot(covered != 0u));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) covered += __shfl_xor(covered, m);
    if ((threadIdx.x & 63u) == 0u && groups) {
        atomicAdd(counts, groups);
        atomicAdd(counts + 1, covered);
    }
}

// The tile list of a subset launch: the launch tiles (id = by * launch_tiles_x + bx, the render kernels' numbering for this workgroup shape) whose
// group is selected, in the order of `order` (the heavy-first schedule) or in image order (null) -- a STABLE compaction -- then the sentinel up to
// `slots`.  ONE workgroup walks the n tiles in chunks of 1024: wave ballot + mbcnt give a lane its place inside the wavefront, the sixteen wave
// totals go through LDS, a running base carries over from chunk to chunk.  per_group = launch tiles per group in x: 1 (32x8 tiles) or 4 (8x8).
__global__ void __launch_bounds__(1024) rt_tile_list_kernel(const uint32_t *__restrict__ order, uint32_t n, uint32_t launch_tiles_x, uint32_t per_group,
                                                            uint32_t groups_x, const uint32_t *__restrict__ selected, uint32_t *__restrict__ list,
                                                            uint32_t slots, uint32_t sentinel) {
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    uint32_t base = 0;                                      // (the same in every lane)
    for (uint32_t first = 0; first < n; first += 1024u) {
        const uint32_t i = first + tid;
        uint32_t id = 0;
        bool keep = false;
        if (i < n) {
            id = order ? order[i] : i;
            if (id < n) {                                   // (an order holds each id below n once; anything else is dropped, not followed)
                const uint32_t by = id / launch_tiles_x, bx = id - by * launch_tiles_x;
                keep = selected[by * groups_x + bx / per_group] != 0u;
            }
        }
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
        if (keep && at + before < slots) list[at + before] = id;
        base += total;
        __syncthreads();                                    // (s_wave is written again by the next chunk)
    }
    for (uint32_t k = base + tid; k < slots; k += 1024u) list[k] = sentinel;
}

// One thread per 8x8 tile: + n_samples where the tile's group is selected.  `is_explicit` == 0: the array holds nothing yet (the context was not
// ragged) and every tile starts from `cur`.
__global__ void __launch_bounds__(256) rt_tile_advance_kernel(uint32_t *__restrict__ passes, int is_explicit, uint32_t cur, const uint32_t *__restrict__ selected,
                                                              uint32_t n_tiles, uint32_t tiles_x, uint32_t groups_x, uint32_t n_samples) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t from = is_explicit ? passes[t] : cur;
    passes[t] = from + (selected[ty * groups_x + tx / 4u] ? n_samples : 0u);
}

// rt_merge_async with a ragged context among them (tiles at different pass counts after subset launches; rt_state.hip has the whole-frame kernel): the same arithmetic per float,
// but a context's weight is the pass count of THE TILE THE FLOAT'S PIXEL LIES IN -- passes[k][tile] for a ragged context, cur[k] for a whole one -- a
// context whose tile holds no pass is skipped for that tile, and a tile nobody holds a pass of keeps dst's floats.  The colour plane is y-flipped against
// the tile map (.cl:579): float i belongs to pixel i / 3, plane row (i / 3) / w, image row h - 1 - that.  One float per thread and step: the weights
// change every 24 floats of a row, and the plane's rows start at any multiple of 12 bytes.  Same unrolled, constant-indexed loop over the arguments.
namespace rt {
struct MergeTileArgs {
    const float *plane[kMergeMax];
    const uint32_t *passes[kMergeMax];  // null: the context is whole, every tile holds cur[k]
    uint32_t cur[kMergeMax];
    int count;                          // 1 .. kMergeMax, dst first (every context is listed, whatever it holds)
};
}  // namespace rt

__global__ void __launch_bounds__(256) rt_merge_tiles_kernel(float *out, rt::MergeTileArgs a, int w, int h, size_t n_floats) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t tiles_x = (uint32_t)(w + 7) / 8u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_floats; i += stride) {
        const uint32_t px = (uint32_t)(i / 3), row = px / (uint32_t)w, x = px - row * (uint32_t)w, y = (uint32_t)h - 1u - row;
        const uint32_t tile = (y >> 3) * tiles_x + (x >> 3);
        float acc = 0.f;
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < rt::kMergeMax; ++k) {
            if (k >= a.count) break;
            const uint32_t n = a.passes[k] ? a.passes[k][tile] : a.cur[k];
            if (n == 0u) continue;
            const float term = a.plane[k][i] * (float)n;
            acc = total == 0u ? term : acc + term;
            total += n;
        }
        if (total != 0u) out[i] = acc * (1.0f / (float)total);
    }
}

// ... and dst's tile counts afterwards: the per-tile sums (one thread per tile; dst's own count is read before it is written)
__global__ void __launch_bounds__(256) rt_merge_tile_counts_kernel(uint32_t *out, rt::MergeTileArgs a, uint32_t n_tiles) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < rt::kMergeMax; ++k) {
        if (k >= a.count) break;
        total += a.passes[k] ? a.passes[k][t] : a.cur[k];
    }
    out[t] = total;
}

using namespace rt;

namespace rt {

// the three device arrays, on first use
int tiles_ensure(rt_ctx *c) {
    rt::TileSubset &s = c->tiles;
    const size_t tiles = std::max<size_t>(tile_count(c), 1), tiles_x = tiles_per_row(c);
    RT_TRY(ensure_device(c->owned, &s.d_passes, tiles));
    RT_TRY(ensure_device(c->owned, &s.d_selected, (size_t)group_count(c) + 2));
    RT_TRY(ensure_device(c->owned, &s.d_list, tiles + tiles_x));      // every tile, and the padding of the last grid row
    return RT_OK;
}

int tiles_refuse(const rt_ctx *c, const char *call) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return fail(RT_ERR_ARG, "%s: a multi-device context renders whole frames only", call);
    if (c->nranks > 1) return fail(RT_ERR_ARG, "%s: a sharded context (rank %d of %d) renders whole frames only", call, c->rank, c->nranks);
    return RT_OK;
}

int tiles_build_list(rt_ctx *c, int waves, bool by_order, uint32_t n_launch, uint32_t slots, hipStream_t stream) {
    const rt::TileSubset &s = c->tiles;
    const uint32_t tiles_x = tiles_per_row(c), groups_x = groups_per_row(c);
    if (slots > tile_count(c) + tiles_x) return fail(RT_ERR_STATE, "rt_render_tiles_async: a list of %u entries for %u tiles", slots, tile_count(c));
    hipLaunchKernelGGL(rt_tile_list_kernel, dim3(1), dim3(1024), 0, stream, by_order ? c->order.d_order : nullptr, n_launch,
                       waves == 4 ? groups_x : tiles_x, waves == 4 ? 1u : 4u, groups_x, s.d_selected, s.d_list, slots, n_launch);
    HIP_TRY(hipGetLastError());
    c->frame.list_built(by_order, n_launch, slots);
    return RT_OK;
}

// The selected groups themselves as a list (TileSubset::d_groups: what rt_denoise_pair_tiles_async's kernel walks): the same compaction with a group as
// its own launch tile -- no order, n = slots = sentinel = the group count, groups_x tiles per row, one per group, so that id = i and the flag read is
// selected[id].  The render's list and its key (FrameState::list_built) are not touched.
int tiles_build_group_list(rt_ctx *c, hipStream_t stream) {
    rt::TileSubset &s = c->tiles;
    const uint32_t n_groups = group_count(c), groups_x = groups_per_row(c);
    RT_TRY(ensure_device(c->owned, &s.d_groups, n_groups));
    hipLaunchKernelGGL(rt_tile_list_kernel, dim3(1), dim3(1024), 0, stream, nullptr, n_groups, groups_x, 1u, groups_x, s.d_selected, s.d_groups, n_groups, n_groups);
    HIP_TRY(hipGetLastError());
    c->frame.group_list_built();
    return RT_OK;
}

int tiles_advance(rt_ctx *c, int n_samples, hipStream_t stream) {
    const uint32_t n = tile_count(c);
    hipLaunchKernelGGL(rt_tile_advance_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, c->tiles.d_passes, c->frame.ragged ? 1 : 0,
                       (uint32_t)c->frame.current_sample, c->tiles.d_selected, n, tiles_per_row(c), groups_per_row(c), (uint32_t)n_samples);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int merge_by_tile(rt_ctx *dst, rt_ctx *const *srcs, int n_srcs, int total, hipStream_t stream) {
    int rc = tiles_ensure(dst);
    if (rc != RT_OK) return rc;
    rt::MergeTileArgs t{};
    // behind everything the destination and the sources have queued; their later work behind the merge
    rc = chain(dst, stream);
    for (int k = -1; k < n_srcs && rc == RT_OK; ++k) {
        rt_ctx *x = k < 0 ? dst : srcs[k];
        if (k >= 0) rc = chain(x, stream);
        t.plane[t.count] = x->d_colors;
        t.passes[t.count] = x->frame.ragged ? x->tiles.d_passes : nullptr;
        t.cur[t.count] = (uint32_t)x->frame.current_sample;
        t.count += 1;
    }
    if (rc != RT_OK) return rc;
    const size_t n_floats = color_floats(dst);
    const size_t blocks = std::max<size_t>(1, std::min((n_floats + 255) / 256, (size_t)dst->knobs.n_cus * 8));
    hipLaunchKernelGGL(rt_merge_tiles_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dst->d_colors, t, dst->w, dst->h, n_floats);
    HIP_TRY(hipGetLastError());
    const uint32_t n_tiles = tile_count(dst);
    hipLaunchKernelGGL(rt_merge_tile_counts_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, stream, dst->tiles.d_passes, t, n_tiles);
    HIP_TRY(hipGetLastError());
    dst->frame.merged_by_tile(total);
    return RT_OK;
}

}  // namespace rt

extern "C" {

RT_API int rt_select_tiles(rt_ctx *c, const uint32_t *err_dev, uint32_t above, void *hip_stream, uint32_t counts[2]) {
    int rc = tiles_refuse(c, "rt_select_tiles");
    if (rc != RT_OK) return rc;
    rc = select_device(c);
    if (rc == RT_OK) rc = tiles_ensure(c);
    if (rc != RT_OK) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    const rt::TileSubset &s = c->tiles;
    const uint32_t groups = group_count(c);
    uint32_t *d_counts = s.d_selected + groups;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(rt_select_tiles_kernel, dim3((groups + 255) / 256), dim3(256), 0, stream, err_dev, above, c->frame.ragged ? s.d_passes : nullptr,
                       (uint32_t)c->frame.current_sample, c->w, c->local_rows, s.d_selected, d_counts);
    HIP_TRY(hipGetLastError());
    c->frame.selection_started();                           // (the flags are being rewritten: no selection until the counts are back)
    uint32_t got[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    c->frame.selection_landed(got[0], got[1]);
    if (counts) {
        counts[0] = got[0];
        counts[1] = got[1];
    }
    return RT_OK;
}

RT_API int rt_render_tiles_async(rt_ctx *c, int n_samples, void *hip_stream) {
    int rc = tiles_refuse(c, "rt_render_tiles_async");
    if (rc != RT_OK) return rc;
    rc = select_device(c);
    if (rc != RT_OK) return rc;
    return launch_tiles(c, n_samples, (hipStream_t)hip_stream);
}

RT_API int rt_tile_passes(rt_ctx *c, uint32_t *out_host) {
    int rc = tiles_refuse(c, "rt_tile_passes");
    if (rc != RT_OK) return rc;
    if (!out_host) return fail(RT_ERR_ARG, "out_host is null");
    const uint32_t n = tile_count(c);
    if (!c->frame.ragged) {                                 // implicit: nothing is stored while every tile holds current_sample passes
        std::fill(out_host, out_host + n, (uint32_t)c->frame.current_sample);
        return RT_OK;
    }
    return read_back(c, out_host, c->tiles.d_passes, (size_t)n * sizeof(uint32_t));
}

}  // extern "C"
