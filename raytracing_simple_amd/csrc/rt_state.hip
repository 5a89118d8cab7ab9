// rt_state.hip -- render state in and out of a context (include/rt_api.h, "render state"): a progressive render is the colour
// plane, the per-pixel seed pairs and the pass number, and the calls of this file WRITE them --
//   rt_seed_stream_async   rt_reset_async + a seed stream of the caller's choice, generated on the device
//   rt_write_state         colour plane, seeds and pass number from the host (what rt_read_colors / rt_read_seeds return)
//   rt_save_state / rt_load_state   the same through a checkpoint file
//   rt_merge_async         the sample-weighted average of several contexts' planes
// The reference continues a render from (colours, seeds, currentSample) by construction -- they are the kernel's arguments
// (SimpleRT/kernel/RayTracing_Kernel.cl:551-600); seed streams other than the default one and merged frames are this library's
// own extension and reproduce no reference frame.
// The render kernels are not touched: a launch reads its first pass from LaunchParams::seeds_in and continues the running
// average from LaunchParams::first_sample (rt_launch.hip make_params), whatever put them there.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_internal.h"

using rt::fail;

// The seed stream `stream_id` (rt_stream_seeds, rt_host.cpp: the same arithmetic): one thread per pair, one 8-byte store each.
__global__ void __launch_bounds__(256) rt_seed_stream_kernel(unsigned long long *seeds, size_t n_pairs, unsigned long long stream_id) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    unsigned long long z = stream_id * 0x9E3779B97F4A7C15ull + (unsigned long long)i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    unsigned lo = (unsigned)z, hi = (unsigned)(z >> 32);
    lo = lo < 2u ? 2u : lo;                                 // OpenCLConfig.cpp:676-680
    hi = hi < 2u ? 2u : hi;
    seeds[i] = (unsigned long long)lo | ((unsigned long long)hi << 32);       // seeds[2i] = lo, seeds[2i + 1] = hi
}

// rt_merge_async: out = (sum over the listed planes of plane * weight) * inv_total, per float, in binary32, in list order, multiply and add
// separate (this unit is compiled with -ffp-contract=off).  `out` may be one of the planes: every thread reads an element of every plane
// before it writes that element.  Pointers and weights travel by value; the loop over them is wave-uniform and unrolled, so the
// argument arrays are only ever indexed by constants.
namespace rt {
struct MergeArgs {
    const float *plane[kMergeMax];
    float weight[kMergeMax];
    int count;                          // 1 .. kMergeMax
    float inv_total;                    // 1.0f / (float)N
};
}  // namespace rt

__global__ void __launch_bounds__(256) rt_merge_kernel(float *out, rt::MergeArgs a, size_t n_floats) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n4 = n_floats >> 2;
    for (size_t i = first; i < n4; i += stride) {           // 16 bytes per plane and thread (every plane is a hipMalloc block: aligned)
        float4 v = reinterpret_cast<const float4 *>(a.plane[0])[i];
        float4 acc = make_float4(v.x * a.weight[0], v.y * a.weight[0], v.z * a.weight[0], v.w * a.weight[0]);
#pragma unroll
        for (int k = 1; k < rt::kMergeMax; ++k) {
            if (k >= a.count) break;
            v = reinterpret_cast<const float4 *>(a.plane[k])[i];
            acc.x = acc.x + v.x * a.weight[k];
            acc.y = acc.y + v.y * a.weight[k];
            acc.z = acc.z + v.z * a.weight[k];
            acc.w = acc.w + v.w * a.weight[k];
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(acc.x * a.inv_total, acc.y * a.inv_total, acc.z * a.inv_total, acc.w * a.inv_total);
    }
    for (size_t i = 4 * n4 + first; i < n_floats; i += stride) {   // the tail: 3 * w * h need not be a multiple of 4
        float acc = a.plane[0][i] * a.weight[0];
#pragma unroll
        for (int k = 1; k < rt::kMergeMax; ++k) {
            if (k >= a.count) break;
            acc = acc + a.plane[k][i] * a.weight[k];
        }
        out[i] = acc * a.inv_total;
    }
}

using namespace rt;

namespace {

// ---- the checkpoint file (include/rt_api.h documents the format) ----
constexpr char kStateMagic[8] = { 'R', 'T', 'S', 'T', 'A', 'T', 'E', '\0' };
constexpr uint32_t kStateVersion = 1;
struct StateHeader {
    char magic[8];
    uint32_t version;
    int32_t w, h, current_sample;
};
static_assert(sizeof(StateHeader) == 24, "the checkpoint header is 24 bytes");

// one plain context: everything it has queued is waited for, then the state is written on its own stream (blocking)
int write_one(rt_ctx *c, const float *colors_host, const uint32_t *seeds_host, int current_sample) {
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    rc = wait_all(c);
    if (rc != RT_OK) return rc;
    rc = chain(c, c->stream);
    if (rc != RT_OK) return rc;
    const size_t px = image_pixels(c);
    if (colors_host) HIP_TRY(hipMemcpyAsync(c->d_colors, colors_host, 3 * px * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (seeds_host) HIP_TRY(hipMemcpyAsync(c->d_seeds, seeds_host, 2 * px * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, 32 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_stats, 0, rt::kStatReplicas * 8 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));               // the caller's buffers may go
    end_frame(c).state_written(current_sample, seeds_host != nullptr);
    return RT_OK;
}

}  // namespace

extern "C" {

RT_API int rt_seed_stream_async(rt_ctx *c, uint64_t stream_id, void *hip_stream) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    // pass 0, counters, launch count, the frame's end: rt_reset_async's own (a multi-device context: every shard on its own stream)
    int rc = rt_reset_async(c, hip_stream);
    if (rc != RT_OK || stream_id == 0) return rc;           // stream 0 IS the default stream, read in place
    const int n = c->multi ? rt::multi_shards(c) : 1;
    for (int r = 0; r < n; ++r) {
        rt_ctx *s = c->multi ? rt::multi_shard(c, r) : c;
        hipStream_t stream = c->multi ? s->stream : (hipStream_t)hip_stream;
        rc = select_device(s);
        if (rc != RT_OK) return rc;
        rc = chain(s, stream);
        if (rc != RT_OK) return rc;
        const size_t px = image_pixels(s);
        hipLaunchKernelGGL(rt_seed_stream_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream,
                           reinterpret_cast<unsigned long long *>(s->d_seeds), px, (unsigned long long)stream_id);
        HIP_TRY(hipGetLastError());
        s->frame.custom_seeds_written();                    // the next launch reads d_seeds
    }
    return RT_OK;
}

RT_API int rt_write_state(rt_ctx *c, const float *colors_host, const uint32_t *seeds_host, int current_sample) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (current_sample < 0) return fail(RT_ERR_ARG, "current_sample %d", current_sample);
    if (!colors_host && current_sample != 0)
        return fail(RT_ERR_ARG, "colors_host is null and current_sample is %d: only pass 0 overwrites the colour plane", current_sample);
    if (!c->multi) return write_one(c, colors_host, seeds_host, current_sample);
    int rc = rt::multi_reset(c, false);                     // (refuses a broken context; the front's launch count and time restart)
    if (rc != RT_OK) return rc;
    for (int r = 0; r < rt::multi_shards(c); ++r) {         // every shard gets the full image and goes on rendering its own rows
        rc = write_one(rt::multi_shard(c, r), colors_host, seeds_host, current_sample);
        if (rc != RT_OK) return rc;
    }
    c->frame.front_follows(current_sample);
    return RT_OK;
}

RT_API int rt_save_state(rt_ctx *c, const char *path) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (!path) return fail(RT_ERR_ARG, "path is null");
    if (c->frame.ragged) return fail(RT_ERR_STATE, "rt_save_state: the tiles hold different pass counts after a subset launch, and the file format holds one pass number");
    const size_t px = image_pixels(c);
    std::vector<float> colors(3 * px);
    std::vector<uint32_t> seeds(2 * px);
    int rc = rt_read_colors(c, colors.data());
    if (rc == RT_OK) rc = rt_read_seeds(c, seeds.data());
    if (rc != RT_OK) return rc;
    StateHeader hd;
    memcpy(hd.magic, kStateMagic, sizeof hd.magic);
    hd.version = kStateVersion;
    hd.w = c->w;
    hd.h = c->h;
    hd.current_sample = c->frame.current_sample;
    FILE *f = fopen(path, "wb");
    if (!f) return fail(RT_ERR_ARG, "rt_save_state: cannot open %s for writing", path);
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && fwrite(colors.data(), sizeof(float), colors.size(), f) == colors.size() &&
              fwrite(seeds.data(), sizeof(uint32_t), seeds.size(), f) == seeds.size();
    ok = (fclose(f) == 0) && ok;
    if (!ok) return fail(RT_ERR_ARG, "rt_save_state: writing %s failed", path);
    return RT_OK;
}

RT_API int rt_load_state(rt_ctx *c, const char *path) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (!path) return fail(RT_ERR_ARG, "path is null");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RT_ERR_ARG, "rt_load_state: cannot open %s", path);
    const size_t px = image_pixels(c);
    std::vector<float> colors;
    std::vector<uint32_t> seeds;
    StateHeader hd;
    auto read_all = [&]() -> int {                          // the whole file is read and checked before the context is touched
        if (fread(&hd, sizeof hd, 1, f) != 1) return fail(RT_ERR_ARG, "rt_load_state: %s is too short for a header (%zu bytes)", path, sizeof hd);
        if (memcmp(hd.magic, kStateMagic, sizeof hd.magic) != 0) return fail(RT_ERR_ARG, "rt_load_state: %s has the wrong magic (not a render state)", path);
        if (hd.version != kStateVersion) return fail(RT_ERR_ARG, "rt_load_state: %s is version %u, this library reads version %u", path, hd.version, kStateVersion);
        if (hd.w != c->w || hd.h != c->h)
            return fail(RT_ERR_ARG, "rt_load_state: %s holds another image size, %dx%d, and the context is %dx%d", path, hd.w, hd.h, c->w, c->h);
        if (hd.current_sample < 0) return fail(RT_ERR_ARG, "rt_load_state: %s holds pass number %d", path, hd.current_sample);
        colors.resize(3 * px);
        seeds.resize(2 * px);
        if (fread(colors.data(), sizeof(float), colors.size(), f) != colors.size() || fread(seeds.data(), sizeof(uint32_t), seeds.size(), f) != seeds.size())
            return fail(RT_ERR_ARG, "rt_load_state: %s is too short for %dx%d (%zu bytes expected)", path, c->w, c->h, sizeof hd + 20 * px);
        return RT_OK;
    };
    const int rc = read_all();
    fclose(f);
    if (rc != RT_OK) return rc;
    return rt_write_state(c, colors.data(), seeds.data(), hd.current_sample);
}

RT_API int rt_merge_async(rt_ctx *dst, rt_ctx *const *srcs, int n_srcs, void *hip_stream) {
    if (!dst) return fail(RT_ERR_ARG, "ctx is null");
    if (!srcs) return fail(RT_ERR_ARG, "srcs is null");
    if (n_srcs < 1 || n_srcs > rt::kMergeMax - 1) return fail(RT_ERR_ARG, "n_srcs %d (1 .. %d)", n_srcs, rt::kMergeMax - 1);
    for (int k = 0; k < n_srcs; ++k) {
        char name[16];
        snprintf(name, sizeof name, "srcs[%d]", k);
        const int rc = same_frame(srcs[k], dst, "rt_merge_async", name, "the destination");
        if (rc != RT_OK) return rc;
        for (int j = 0; j < k; ++j)
            if (srcs[j] == srcs[k]) return fail(RT_ERR_ARG, "srcs[%d] repeats srcs[%d]", k, j);
    }
    // the contexts that hold passes, destination first: one at pass 0 is skipped, not weighted by zero (its plane may hold an old frame, or nothing)
    rt::MergeArgs a{};
    rt_ctx *used[rt::kMergeMax];
    long long total = 0;
    for (int k = -1; k < n_srcs; ++k) {
        rt_ctx *x = k < 0 ? dst : srcs[k];
        if (x->frame.current_sample <= 0) continue;
        used[a.count] = x;
        a.plane[a.count] = x->d_colors;
        a.weight[a.count] = (float)x->frame.current_sample;
        a.count += 1;
        total += x->frame.current_sample;
    }
    if (total == 0) return fail(RT_ERR_STATE, "rt_merge_async: none of the %d contexts holds a pass", n_srcs + 1);
    if (total > INT_MAX) return fail(RT_ERR_ARG, "rt_merge_async: the pass counter would overflow (%lld)", total);
    a.inv_total = 1.0f / (float)total;
    int rc = select_device(dst);
    if (rc != RT_OK) return rc;
    bool ragged = dst->frame.ragged;
    for (int k = 0; k < n_srcs; ++k) ragged = ragged || srcs[k]->frame.ragged;
    if (ragged)                                             // tiles at different pass counts (after subset launches): every float by its own tile's weights
        return merge_by_tile(dst, srcs, n_srcs, (int)total, (hipStream_t)hip_stream);
    // behind everything the destination and the sources it reads have queued; their later work behind the merge
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(dst, stream);
    for (int k = 0; k < a.count && rc == RT_OK; ++k)
        if (used[k] != dst) rc = chain(used[k], stream);
    if (rc != RT_OK) return rc;
    const size_t n_floats = color_floats(dst);
    size_t blocks = (n_floats / 4 + 255) / 256, cap = (size_t)dst->knobs.n_cus * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(rt_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dst->d_colors, a, n_floats);
    HIP_TRY(hipGetLastError());
    dst->frame.merged((int)total);
    return RT_OK;
}

}  // extern "C"
