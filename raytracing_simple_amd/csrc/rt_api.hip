// rt_api.hip -- the C ABI of include/rt_api.h: context = the reference's OpenCLConfigBuffer
// (SimpleRT/src/OpenCLConfig.cpp:398-747) re-done for one MI355X: device buffers, scene
// tables, launch geometry, row-tile sharding, counters.  No CPU fallback: without a HIP
// device every entry point fails with RT_ERR_NO_DEVICE.
//
// Ordering rule of this file: ALL device work of one context -- launches, resets, scene updates,
// read-backs -- executes in the order the calls were made, whatever streams the caller passes:
// when a call uses another stream than the context's previous piece of work, the library records an
// event on the previous stream and makes the new one wait for it (chain()).  Nothing here uses the
// null stream or a device-wide synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <mutex>
#include <new>
#include <vector>

#include "rt_internal.h"

#ifndef RT_DIAGNOSTICS
#define RT_DIAGNOSTICS 0
#endif

namespace {
thread_local char g_err[512] = "";
// where the last rt_create / rt_create_sharded spent its host time, in milliseconds (rt_debug_create_breakdown):
// [0] device query, [1] stream + events, [2] device allocations, [3] kernel function attributes (the first context of a
// process pays the load of the library's code object here), [4] default seed stream generated on the host, [5] its upload,
// [6] the restore kernel (first launch) and the wait for it, [7] total
double g_create_ms[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
double now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}
}

namespace rt {
const double *create_breakdown() { return g_create_ms; }
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace rt

using rt::fail;

// the one place a handle of a record (rt_owned.h) goes back to the runtime
void rt::owned_free(rt::Owned::Kind kind, void *handle) {
    switch (kind) {
    case rt::Owned::Kind::Device: (void)hipFree(handle); break;
    case rt::Owned::Kind::Pinned: (void)hipHostFree(handle); break;
    case rt::Owned::Kind::Registered: (void)hipHostUnregister(handle); break;
    case rt::Owned::Kind::Event: (void)hipEventDestroy(static_cast<hipEvent_t>(handle)); break;
    case rt::Owned::Kind::Stream: (void)hipStreamDestroy(static_cast<hipStream_t>(handle)); break;
    }
}

// rt_reset_async zeroes the work counters with a kernel on the caller's stream and restores NO seeds:
// the next launch reads the pristine default stream directly (LaunchParams::seeds_in).
__global__ void rt_zero_counters_kernel(unsigned long long *counters, unsigned long long *stats) {
    for (int i = threadIdx.x; i < 32; i += blockDim.x) counters[i] = 0ull;
    for (int i = threadIdx.x; i < rt::kStatReplicas * 8; i += blockDim.x) stats[i] = 0ull;
}

// rt_create / rt_reset: seeds = the pristine default stream, colour plane, pixels and counters zero
// (OpenCLConfig.cpp:613-682), as ONE kernel instead of a runtime copy and four fills.
__global__ void __launch_bounds__(256) rt_restore_kernel(unsigned long long *seeds, const unsigned long long *seeds0, size_t n_pairs,
                                                         uint32_t *colors, size_t n_colors, uint32_t *pixels, size_t n_pixels,
                                                         unsigned long long *counters, unsigned long long *stats) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = first; i < n_pairs; i += stride) seeds[i] = seeds0[i];
    for (size_t i = first; i < n_colors; i += stride) colors[i] = 0u;
    for (size_t i = first; i < n_pixels; i += stride) pixels[i] = 0u;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < 32; i += blockDim.x) counters[i] = 0ull;
        for (int i = threadIdx.x; i < rt::kStatReplicas * 8; i += blockDim.x) stats[i] = 0ull;
    }
}

// rt_deinterleave_rows: full[y] = row (t/n)*tile_rows + y%tile_rows of rank t%n's block, t = y/tile_rows.
// One thread per 16 bytes where the row length allows it (w % 4 == 0 keeps every row 16-byte aligned).
__global__ void __launch_bounds__(256) rt_deinterleave_kernel(uint32_t *__restrict__ full, const uint32_t *__restrict__ gathered, int w,
                                                              int h, int nranks, int tile_rows, int pad_rows, int vec) {
    const int per_row = vec ? w / 4 : w;
    const size_t total = (size_t)per_row * (size_t)h;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / (size_t)per_row), xq = (int)(i - (size_t)y * (size_t)per_row);
        const int t = y / tile_rows, r = t % nranks, lrow = (t / nranks) * tile_rows + (y - t * tile_rows);
        const size_t src = ((size_t)r * (size_t)pad_rows + (size_t)lrow) * (size_t)w, dst = (size_t)y * (size_t)w;
        if (vec)
            reinterpret_cast<uint4 *>(full + dst)[xq] = reinterpret_cast<const uint4 *>(gathered + src)[xq];
        else
            full[dst + xq] = gathered[src + xq];
    }
}

namespace rt {

int select_device(const rt_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    return RT_OK;
}

// the context's work runs in issue order: `stream` waits for whatever the context queued last elsewhere
int chain(rt_ctx *c, hipStream_t stream) {
    if (c->last_stream != stream) {
        HIP_TRY(hipEventRecord(c->ev_dep, c->last_stream));
        HIP_TRY(hipStreamWaitEvent(stream, c->ev_dep, 0));
        c->last_stream = stream;
        if (stream != c->stream) c->used_foreign_stream = true;
    }
    return RT_OK;
}

int chain_all(hipStream_t stream, std::initializer_list<rt_ctx *> ctxs) {
    for (rt_ctx *c : ctxs) RT_TRY(chain(c, stream));
    return RT_OK;
}

// host waits for everything the context has queued
int wait_all(rt_ctx *c) {
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    return RT_OK;
}

// rt_read_pixels / rt_read_pixels_async / rt_compare_async: if the last launches ran with the pixel store off, a small kernel packs the
// frame from the running average (same toInt, .cl:34,594-596) into the buffer the launches write
int refresh_pixels(rt_ctx *c, hipStream_t stream) {
    if (c->frame.pixels_current || c->frame.current_sample <= 0) return RT_OK;
    rt::LaunchParams p = make_params(c, 0);
    hipError_t e = c->knobs.fast() ? rt::launch_pack_fast(p, stream) : rt::launch_pack_parity(p, stream);
    if (e != hipSuccess) return fail(RT_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    c->frame.pixels_packed();
    return RT_OK;
}

int read_back(rt_ctx *c, void *host, const void *dev, size_t bytes, bool wait) {
    int rc = select_device(c);
    if (rc == RT_OK) rc = chain(c, c->stream);          // behind everything the context has queued, on whatever stream
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
    return RT_OK;
}

int read_plane(rt_ctx *c, const char *call, Plane which, float *host, uint32_t *packed_host) {
    RT_TRY(tiles_refuse(c, call));
    const PlaneView v = plane_view(c, which);
    if (!host && !packed_host) return v.host_name ? fail(RT_ERR_ARG, "%s: %s is null", call, v.host_name) : fail(RT_ERR_ARG, "%s: both buffers are null", call);
    if (!v.current) return fail(RT_ERR_STATE, "%s: the context holds no current %s", call, v.absent);
    if (host) RT_TRY(read_back(c, host, v.plane, v.floats * sizeof(float), packed_host == nullptr));
    if (packed_host) RT_TRY(read_back(c, packed_host, v.packed, image_pixels(c) * sizeof(uint32_t)));
    return RT_OK;
}

int filter_input(const rt_ctx *c, const char *call, const char *who, bool want_moments, PlaneInput *out) {
    const bool from_temporal = temporal_current(c);
    if (!from_temporal && c->frame.current_sample <= 0) return fail(RT_ERR_STATE, "%s: %s holds neither a current temporal plane nor a pass", call, who);
    *out = { from_temporal ? c->planes.temporal : c->d_colors, from_temporal ? 4 : 3, (float)c->frame.current_sample,
             want_moments && moments_current(c) ? reinterpret_cast<const float4 *>(c->planes.moments) : nullptr };
    return RT_OK;
}

int same_frame(const rt_ctx *a, const rt_ctx *b, const char *call, const char *a_name, const char *b_name, bool sharding) {
    if (!a || !b) return fail(RT_ERR_ARG, "%s: %s is null", call, a ? b_name : a_name);
    if (a == b) return fail(RT_ERR_ARG, "%s: %s is %s itself", call, a_name, b_name);
    if (a->multi || b->multi) return fail(RT_ERR_ARG, "%s: %s is a multi-device context", call, a->multi ? a_name : b_name);
    if (a->w != b->w || a->h != b->h || (sharding && (a->rank != b->rank || a->nranks != b->nranks || a->tile_rows != b->tile_rows)))
        return fail(RT_ERR_ARG, "%s: %s is %dx%d, rank %d of %d by %d rows; %s %dx%d, rank %d of %d by %d rows", call, a_name, a->w, a->h, a->rank, a->nranks,
                    a->tile_rows, b_name, b->w, b->h, b->rank, b->nranks, b->tile_rows);
    if (a->device != b->device) return fail(RT_ERR_ARG, "%s: %s lives on device %d, %s on device %d", call, a_name, a->device, b_name, b->device);
    return RT_OK;
}

int upload_default_seeds(rt_ctx *c) {
    const size_t count = 2 * image_pixels(c);
    const double t0 = now_ms();
    std::vector<uint32_t> host(count);
    rt_default_seeds(host.data(), count);
    g_create_ms[4] = now_ms() - t0;
    HIP_TRY(hipMemcpyAsync(c->d_seeds0, host.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // `host` goes out of scope
    return RT_OK;
}

int restore_state(rt_ctx *c) {                          // rt_create / rt_reset: blocking
    int rc = chain(c, c->stream);
    if (rc != RT_OK) return rc;
    const size_t px = image_pixels(c);
    size_t blocks = (3 * px + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rt_restore_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, reinterpret_cast<unsigned long long *>(c->d_seeds),
                       reinterpret_cast<const unsigned long long *>(c->d_seeds0), px, reinterpret_cast<uint32_t *>(c->d_colors), 3 * px,
                       c->d_pixels, local_pixels(c), c->d_counters, c->d_stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RT_OK;
}

}  // namespace rt

using namespace rt;

extern "C" {

RT_API const char *rt_last_error(void) { return g_err; }

// used by rt_host.cpp (hidden: not part of the export table)
void rt_host_set_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg ? msg : ""); }

RT_API int rt_create_sharded(rt_ctx **out, int w, int h, int device, int rank, int nranks, int tile_rows) {
    if (!out) return fail(RT_ERR_ARG, "out is null");
    *out = nullptr;
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return fail(RT_ERR_ARG, "image size %dx%d (1 .. 65535 in either direction)", w, h);
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(RT_ERR_ARG, "rank %d of %d", rank, nranks);
    if (tile_rows <= 0 || tile_rows % rt::kTileH != 0)
        return fail(RT_ERR_ARG, "tile_rows must be a positive multiple of %d", rt::kTileH);

    const double t_begin = now_ms();
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(RT_ERR_NO_DEVICE, "no HIP device (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n_dev) return fail(RT_ERR_ARG, "device %d of %d", device, n_dev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RT_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device,
                    prop.gcnArchName);

    rt_ctx *c = new (std::nothrow) rt_ctx();
    if (!c) return fail(RT_ERR_ALLOC, "host allocation failed");
    c->device = device;
    c->knobs.n_cus = n_cus;
    c->w = w;
    c->h = h;
    c->rank = rank;
    c->nranks = nranks;
    c->tile_rows = tile_rows;
    c->local_rows = rt::rows_of_rank(h, rank, nranks, tile_rows);

    int rc = select_device(c);
    const size_t px = image_pixels(c);
    g_create_ms[0] = now_ms() - t_begin;
    auto alloc_all = [&]() -> int {
        double t = now_ms();
        auto lap = [&](int k) { const double n_ = now_ms(); g_create_ms[k] = n_ - t; t = n_; };
        rt::Owned &own = c->owned;
        RT_TRY(own_stream(own, &c->stream));        // the record's first entry: the last to go
        c->last_stream = c->stream;
        RT_TRY(own_event(own, &c->ev0));
        RT_TRY(own_event(own, &c->ev1));
        for (int k = 0; k < 4; ++k) RT_TRY(own_event(own, &c->probe_ev[k]));
        RT_TRY(own_event(own, &c->ev_dep, hipEventDisableTiming));
        RT_TRY(c->scene.ring.ensure_events(own, hipEventDisableTiming));        // (made here: the first upload costs what every upload costs)
        lap(1);
        RT_TRY(own_device(own, &c->d_seeds, 2 * px));
        RT_TRY(own_device(own, &c->d_seeds0, 2 * px));
        RT_TRY(own_device(own, &c->d_colors, 3 * px));
        RT_TRY(own_device(own, &c->d_pixels, local_pixels(c) + 4));
        RT_TRY(own_device(own, &c->d_counters, 32));
        RT_TRY(own_device(own, &c->d_stats, (size_t)rt::kStatReplicas * 8));
        c->order.n_tiles = tile_count(c);           // the finest tile shape (8x8)
        if (c->order.n_tiles) {
            RT_TRY(own_device(own, &c->order.d_tile_cost, c->order.n_tiles));
            RT_TRY(own_device(own, &c->order.d_order, c->order.n_tiles));
        }
        lap(2);
        // function attributes (dynamic-LDS limit) are per device, not per context
        static std::mutex mu;
        static bool prepared[64] = {};
        {
            std::lock_guard<std::mutex> lock(mu);
            if (device >= 64 || !prepared[device]) {
                HIP_TRY(rt::prepare_parity());
                HIP_TRY(rt::prepare_fast());
                HIP_TRY(rt::prepare_bvh_build());
                if (device < 64) prepared[device] = true;
            }
        }
        lap(3);
        int r2 = upload_default_seeds(c);
        lap(5);
        g_create_ms[5] -= g_create_ms[4];
        if (r2 == RT_OK) r2 = restore_state(c);
        lap(6);
        g_create_ms[7] = now_ms() - t_begin;
        return r2;
    };
    if (rc == RT_OK) rc = alloc_all();
    if (rc != RT_OK) {
        rt_destroy(c);
        return rc;
    }
    *out = c;
    return RT_OK;
}

RT_API int rt_create(rt_ctx **out, int w, int h) { return rt_create_sharded(out, w, h, 0, 0, 1, rt::kTileH); }

RT_API void rt_destroy(rt_ctx *c) {
    if (!c) return;
    if (c->multi) {
        rt::multi_destroy(c);
        delete c;
        return;
    }
    // A shard of a multi-device context whose gather failed AND whose streams had not drained two seconds later (rt_multi.hip multi_destroy
    // polls them) abandons its streams: one may hold a transfer that never completes, and hipFree / hipHostFree / hipStreamDestroy synchronise
    // with the device's work -- so nothing on the device is waited for or given back; what the record holds is leaked, the call returns.
    // (A device that cannot be selected: likewise.)
    if (c->abandon_streams || hipSetDevice(c->device) != hipSuccess) {
        c->owned.forget();
        delete c;
        return;
    }
    if (c->last_stream && c->last_stream != c->stream) (void)hipStreamSynchronize(c->last_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->owned.release();                 // everything the context acquired, wherever (rt_owned.h), the last first; its stream at the end
    delete c;
}

RT_API int rt_scene_choice(rt_ctx *c, double *hierarchy_ms_per_pass, double *sweep_ms_per_pass) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    rt_ctx *s = c->multi ? rt::multi_first_shard(c) : c;
    if (select_device(s) == RT_OK) probe_poll(s, false);
    if (hierarchy_ms_per_pass) *hierarchy_ms_per_pass = s->choice.probe_ms[0];
    if (sweep_ms_per_pass) *sweep_ms_per_pass = s->choice.probe_ms[1];
    return rt::verdict_number(s->choice.bvh_pick);
}

RT_API const char *rt_last_kernel(const rt_ctx *c) { return !c ? "" : (c->multi ? rt::multi_last_kernel(c) : c->last_kernel); }

RT_API int rt_shard_count(const rt_ctx *c) { return !c ? RT_ERR_ARG : (c->multi ? rt::multi_shards(c) : 1); }

RT_API int rt_set_scene(rt_ctx *c, const rt_sphere *spheres, uint32_t count) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (count > 0 && !spheres) return fail(RT_ERR_ARG, "spheres is null");
    if (count > RT_MAX_SPHERES) return fail(RT_ERR_ARG, "%u spheres > RT_MAX_SPHERES (%u)", count, RT_MAX_SPHERES);
    if (c->multi) return rt::multi_set_scene(c, spheres, count);
    rt::SceneState &st = c->scene.state;
    // the very scene the context already holds (a host that sets it before every frame): nothing to do
    if (st.have_scene && count == c->scene.tables.n_spheres && c->scene.h_spheres.size() == count &&
        (count == 0 || memcmp(c->scene.h_spheres.data(), spheres, (size_t)count * sizeof(rt_sphere)) == 0)) {
        st.same_records_set();
        return RT_OK;
    }
    st.records_replaced();
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    rc = ensure_scene_capacity(c, count);
    if (rc != RT_OK) return rc;
    c->scene.is_light.assign(c->scene.cap, 0);
    c->scene.h_spheres.assign(spheres, spheres + count);
    c->order.forget();
    c->choice.new_scene();              // hierarchy or plain sweep, cooperative any-hit or not: undecided again
    rc = upload_spheres(c, 0, count, spheres, count, c->stream, true);
    if (rc != RT_OK) st.upload_failed();
    else st.uploaded();
    return rc;
}

RT_API int rt_update_spheres_async(rt_ctx *c, uint32_t first, uint32_t count, const rt_sphere *spheres, void *hip_stream) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (!c->scene.state.have_scene && !c->multi) return fail(RT_ERR_STATE, "rt_set_scene must precede rt_update_spheres_async");
    if (count > 0 && !spheres) return fail(RT_ERR_ARG, "spheres is null");
    if (c->multi) return rt::multi_update_spheres(c, first, count, spheres);
    const uint32_t n = c->scene.tables.n_spheres;
    if (first > n || count > n - first) return fail(RT_ERR_ARG, "spheres [%u, %u) of a scene of %u", first, first + count, n);
    c->scene.state.records_updated();
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (count) memcpy(c->scene.h_spheres.data() + first, spheres, (size_t)count * sizeof(rt_sphere));
    // the last frame's costs still predict this one (moving spheres): the order stays in use and the next long launch sorts it again from them
    c->order.scene_or_camera_moved();
    // (the records go now; tables and hierarchy are rebuilt once, by the next launch -- rt_scene.hip refresh_tables -- however many updates precede it)
    return upload_spheres(c, first, count, spheres, n, (hipStream_t)hip_stream, false);
}

RT_API int rt_set_camera(rt_ctx *c, const rt_camera *cam) {
    if (!c || !cam) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_set_camera(c, cam);
    if (!c->scene.state.have_cam || memcmp(&c->cam, cam, sizeof *cam) != 0) c->order.scene_or_camera_moved();
    c->cam = *cam;                      // a kernel argument: nothing to upload
    c->scene.state.camera_set();
    return RT_OK;
}

RT_API int rt_set_mode(rt_ctx *c, int mode) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    bool ok = mode == RT_MODE_PARITY || mode == RT_MODE_FAST;
#if RT_DIAGNOSTICS
    // 100+k / 200+k: A/B instances of the parity / fast arithmetic (rt_debug.h; not part of the contract)
    int n_par = 0, n_fast = 0;
    (void)rt::parity_instances(&n_par);
    (void)rt::fast_instances(&n_fast);
    ok = ok || (mode >= 100 && mode < 100 + n_par) || (mode >= 200 && mode < 200 + n_fast);
#endif
    if (!ok) return fail(RT_ERR_ARG, "mode %d", mode);
    if (c->multi) return rt::multi_set_mode(c, mode);
    c->knobs.mode = mode;
#if RT_DIAGNOSTICS
    return rt::debug_layout_for_mode(c);        // (an A/B instance gets the pair table it reads: rt_debug.hip)
#else
    return RT_OK;
#endif
}

RT_API int rt_reset(rt_ctx *c) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_reset(c, false);
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    rc = wait_all(c);
    if (rc != RT_OK) return rc;
    end_frame(c).reset_blocking();      // restore_state copies the default stream into d_seeds
    return restore_state(c);
}

RT_API int rt_reset_async(rt_ctx *c, void *hip_stream) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_reset(c, true);
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    rc = chain(c, (hipStream_t)hip_stream);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(rt_zero_counters_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, c->d_counters, c->d_stats);
    HIP_TRY(hipGetLastError());
    end_frame(c).reset_in_place();      // the next launch reads d_seeds0
    return RT_OK;
}

RT_API int rt_render_async(rt_ctx *c, int n_samples, void *hip_stream) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_render(c, nullptr, n_samples, false);
    if (c->frame.ragged) return fail(RT_ERR_STATE, "rt_render_async: the tiles hold different pass counts after a subset launch (rt_render_tiles_async goes on; rt_reset makes the frame whole)");
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (!c->throttle_on || n_samples <= 0) return launch(c, n_samples, (hipStream_t)hip_stream);
    // rt_throttle's bookkeeping: this launch between two events of the ring (the oldest entry is waited for first)
    hipStream_t stream = (hipStream_t)hip_stream;
    rt_ctx::Flight &f = c->flight[c->flight_next];
    if (f.pending) {
        HIP_TRY(hipEventSynchronize(f.stop));
        f.pending = false;
    }
    rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(f.start, stream));
    rc = launch(c, n_samples, stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(f.stop, stream));
    f.n_samples = n_samples;
    f.pending = true;
    c->flight_next = (c->flight_next + 1) % rt_ctx::kFlights;
    return RT_OK;
}

RT_API int rt_throttle(rt_ctx *c, int max_in_flight, double *ms_per_pass) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (max_in_flight < 0) return fail(RT_ERR_ARG, "max_in_flight %d", max_in_flight);
    if (ms_per_pass) *ms_per_pass = 0.0;
    if (c->multi) {
        if (max_in_flight > 0) return RT_OK;
        const int n = rt::multi_shards(c);
        for (int r = 0; r < n; ++r) {
            rt_ctx *s = rt::multi_shard(c, r);
            HIP_TRY(hipSetDevice(s->device));
            HIP_TRY(hipStreamSynchronize(s->last_stream));
        }
        return rt::multi_wait_frame(c);
    }
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (!c->throttle_on) {
        for (auto &f : c->flight) {         // (a call that failed half-way left the events it made in place: they are not made again)
            if (!f.start) RT_TRY(own_event(c->owned, &f.start));
            if (!f.stop) RT_TRY(own_event(c->owned, &f.stop));
        }
        c->throttle_on = true;
        if (max_in_flight == 0) return wait_all(c);
        return RT_OK;
    }
    // oldest first: retire what has finished, wait for the oldest while too many are left
    int pending = 0;
    for (const auto &f : c->flight) pending += f.pending ? 1 : 0;
    for (int k = 0; k < rt_ctx::kFlights && pending > 0; ++k) {
        rt_ctx::Flight &f = c->flight[(c->flight_next + k) % rt_ctx::kFlights];
        if (!f.pending) continue;
        if (pending > max_in_flight) {
            HIP_TRY(hipEventSynchronize(f.stop));
        } else if (hipEventQuery(f.stop) != hipSuccess) {
            (void)hipGetLastError();
            break;                          // (launches of one context finish in issue order)
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, f.start, f.stop) == hipSuccess && f.n_samples > 0) c->flight_ms_per_pass = (double)ms / f.n_samples;
        else (void)hipGetLastError();
        f.pending = false;
        pending -= 1;
    }
    if (max_in_flight == 0) {
        rc = wait_all(c);                   // (launches from before the first rt_throttle call, copies)
        if (rc != RT_OK) return rc;
    }
    if (ms_per_pass) *ms_per_pass = c->flight_ms_per_pass;
    return RT_OK;
}

RT_API int rt_render_pass(rt_ctx *c, uint32_t *out_host, int n_samples) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_render(c, out_host, n_samples, true);
    if (c->frame.ragged) return fail(RT_ERR_STATE, "rt_render_pass: the tiles hold different pass counts after a subset launch (rt_render_tiles_async goes on; rt_reset makes the frame whole)");
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    rc = chain(c, c->stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    rc = launch(c, n_samples, c->stream, true);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    if (out_host && c->local_rows > 0)
        HIP_TRY(hipMemcpyAsync(out_host, frame_pixels(c), local_pixels(c) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->frame.timed(ms);
    return RT_OK;
}

RT_API int rt_set_pixel_write(rt_ctx *c, int enable) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_set_pixel_write(c, enable);
    c->pixel_write = enable ? 1 : 0;
    return RT_OK;
}

RT_API int rt_read_pixels(rt_ctx *c, uint32_t *out_host) {
    if (!c || !out_host) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_read_pixels(c, out_host);
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (c->local_rows == 0) return RT_OK;
    rc = chain(c, c->stream);
    if (rc != RT_OK) return rc;
    rc = refresh_pixels(c, c->stream);
    if (rc != RT_OK) return rc;
    return read_back(c, out_host, frame_pixels(c), local_pixels(c) * sizeof(uint32_t));
}

RT_API int rt_read_pixels_async(rt_ctx *c, uint32_t *out_host, void *hip_stream) {
    if (!c || !out_host) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_read_pixels(c, out_host);
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (c->local_rows == 0) return RT_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    rc = refresh_pixels(c, stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, frame_pixels(c), local_pixels(c) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return RT_OK;
}

RT_API int rt_pin_output(rt_ctx *c, uint32_t *out_host, size_t count) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return rt::multi_pin_output(c, out_host, count);
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    if (c->pinned_out) {
        rc = wait_all(c);
        if (rc != RT_OK) return rc;
        c->owned.drop(c->pinned_out);
        c->pinned_out = nullptr;
    }
    if (!out_host || local_pixels(c) == 0) return RT_OK;    // nothing to pin (a rank without rows)
    if (count < local_pixels(c)) return fail(RT_ERR_ARG, "output buffer of %zu < %zu elements", count, local_pixels(c));
    RT_TRY(own_registered(c->owned, out_host, count * sizeof(uint32_t)));
    c->pinned_out = out_host;
    return RT_OK;
}

RT_API int rt_set_pixel_buffer(rt_ctx *c, void *dptr, size_t count) {
    if (!c) return fail(RT_ERR_ARG, "ctx is null");
    if (c->multi) return fail(RT_ERR_ARG, "rt_set_pixel_buffer: a multi-device context assembles its frame in its own buffer");
    if (dptr && count < local_pixels(c)) return fail(RT_ERR_ARG, "pixel buffer of %zu < %zu elements", count, local_pixels(c));
    c->d_pixels_ext = static_cast<uint32_t *>(dptr);
    return RT_OK;
}

// The context's own stream (hipStream_t, non-blocking): what rt_render_pass launches on.  Callers
// that keep several contexts in flight can launch each on its own stream through
// rt_render_async(ctx, n, rt_stream(ctx)).
RT_API void *rt_stream(rt_ctx *c) { return !c ? nullptr : (c->multi ? rt::multi_stream(c) : (void *)c->stream); }

RT_API int rt_device_pixels(rt_ctx *c, void **dptr, size_t *count) {
    if (!c || !dptr || !count) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_device_pixels(c, dptr, count);
    *dptr = frame_pixels(c);
    *count = local_pixels(c);
    return RT_OK;
}

RT_API int rt_local_rows(const rt_ctx *c) { return c ? c->local_rows : RT_ERR_ARG; }
RT_API int rt_current_sample(const rt_ctx *c) { return c ? c->frame.current_sample : RT_ERR_ARG; }

RT_API int rt_read_colors(rt_ctx *c, float *out_host) {
    if (!c || !out_host) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_read_colors(c, out_host);
    return read_back(c, out_host, c->d_colors, color_floats(c) * sizeof(float));
}

RT_API int rt_read_seeds(rt_ctx *c, uint32_t *out_host) {
    if (!c || !out_host) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_read_seeds(c, out_host);
    return read_back(c, out_host, c->frame.seeds_default ? c->d_seeds0 : c->d_seeds, 2 * image_pixels(c) * sizeof(uint32_t));
}

RT_API int rt_get_stats(rt_ctx *c, rt_stats *out) {
    if (!c || !out) return fail(RT_ERR_ARG, "null argument");
    if (c->multi) return rt::multi_get_stats(c, out);
    unsigned long long v[32], part[rt::kStatReplicas * 8], sum[5] = { 0, 0, 0, 0, 0 };
    int rc = read_back(c, v, c->d_counters, sizeof v, false);       // two copies, one wait
    if (rc == RT_OK) rc = read_back(c, part, c->d_stats, sizeof part);
    if (rc != RT_OK) return rc;
    for (int r = 0; r < rt::kStatReplicas; ++r)
        for (int k = 0; k < 5; ++k) sum[k] += part[r * 8 + k];
    out->samples = sum[0];
    out->closest_rays = sum[1];
    out->shadow_rays = sum[2];
    out->sphere_tests = sum[3];
    out->rng_draws = sum[4];
    memcpy(c->debug_counters, v + 8, sizeof c->debug_counters);
    out->launches = c->frame.launches;
    out->last_kernel_ms = c->frame.last_ms;
    return RT_OK;
}

RT_API int rt_deinterleave_rows(uint32_t *full, const uint32_t *gathered, int w, int h, int nranks, int tile_rows, int pad_rows,
                                int device, void *hip_stream) {
    if (!full || !gathered) return fail(RT_ERR_ARG, "null argument");
    if (w <= 0 || h <= 0 || nranks < 1 || tile_rows <= 0) return fail(RT_ERR_ARG, "image %dx%d, %d ranks, tiles of %d rows", w, h, nranks, tile_rows);
    const int n_tiles = (h + tile_rows - 1) / tile_rows, need = ((n_tiles + nranks - 1) / nranks) * tile_rows;
    if (pad_rows < need && pad_rows < ((n_tiles - 1) / nranks) * tile_rows + (h - (n_tiles - 1) * tile_rows))
        return fail(RT_ERR_ARG, "pad_rows %d is less than a rank's row count", pad_rows);
    HIP_TRY(hipSetDevice(device));
    const int vec = (w % 4 == 0) && ((reinterpret_cast<uintptr_t>(full) | reinterpret_cast<uintptr_t>(gathered)) % 16 == 0);
    const size_t total = (size_t)(vec ? w / 4 : w) * (size_t)h;
    size_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(rt_deinterleave_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, full, gathered, w, h, nranks,
                       tile_rows, pad_rows, vec);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- rt_render: the one-shot call, with the device state of recent sizes kept ----------------
namespace {
struct CacheEntry {
    int w = 0, h = 0;
    rt_ctx *ctx = nullptr;
    uint32_t *h_pix = nullptr;          // page-locked, w*h; this and the events are entered in ctx's record: they go with it
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    unsigned long long stamp = 0;
};
constexpr int kCacheSlots = 4;
CacheEntry g_cache[kCacheSlots];
unsigned long long g_cache_clock = 0;
std::mutex g_cache_mu;

void cache_drop(CacheEntry &e) {
    if (e.ctx) {
        (void)hipSetDevice(e.ctx->device);
        rt_destroy(e.ctx);
    }
    e = CacheEntry{};
}

int cache_get(int w, int h, CacheEntry **out) {
    int victim = 0;
    for (int k = 0; k < kCacheSlots; ++k) {
        if (g_cache[k].ctx && g_cache[k].w == w && g_cache[k].h == h) {
            *out = &g_cache[k];
            return RT_OK;
        }
        if (g_cache[k].stamp < g_cache[victim].stamp) victim = k;
    }
    CacheEntry &e = g_cache[victim];
    cache_drop(e);
    int rc = rt_create(&e.ctx, w, h);
    if (rc != RT_OK) return rc;
    e.w = w;
    e.h = h;
    hipError_t he = take_pinned(e.ctx->owned, &e.h_pix, (size_t)w * h);
    for (int k = 0; k < 4 && he == hipSuccess; ++k) he = take_event(e.ctx->owned, &e.ev[k], hipEventDisableTiming);
    if (he != hipSuccess) {
        cache_drop(e);
        return fail(RT_ERR_ALLOC, "rt_render staging: %s", hipGetErrorString(he));
    }
    *out = &e;
    return RT_OK;
}
}  // namespace

RT_API void rt_release_cache(void) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (auto &e : g_cache) cache_drop(e);
}

RT_API int rt_render(const rt_scene *scene, const rt_camera *cam, uint32_t *out, int w, int h, int spp) {
    if (!scene || !cam || !out) return fail(RT_ERR_ARG, "null argument");
    if (spp < 0) return fail(RT_ERR_ARG, "spp < 0");
    if (w <= 0 || h <= 0) return fail(RT_ERR_ARG, "image size %dx%d", w, h);
    std::lock_guard<std::mutex> lock(g_cache_mu);
    CacheEntry *e = nullptr;
    int rc = cache_get(w, h, &e);
    if (rc != RT_OK) return rc;
    e->stamp = ++g_cache_clock;
    rt_ctx *c = e->ctx;
    auto run = [&]() -> int {
        // a fresh OpenCLConfigBuffer: pass 0, default seed stream (read in place), parity mode, own pixel buffer
        int r = rt_reset_async(c, c->stream);
        if (r == RT_OK) r = rt_set_mode(c, RT_MODE_PARITY);
        if (r == RT_OK) r = rt_set_pixel_write(c, 1);
        if (r == RT_OK) r = rt_set_pixel_buffer(c, nullptr, 0);
        if (r == RT_OK) r = rt_set_scene(c, scene->spheres, scene->count);
        if (r == RT_OK) r = rt_set_camera(c, cam);
        if (r == RT_OK) r = launch(c, spp, c->stream, true);        // (blocking call: a new large scene may be probed first)
        if (r != RT_OK) return r;
        if (spp == 0) {                 // no pass ran: getPixels() of a fresh backend is the zero-filled buffer
            HIP_TRY(hipStreamSynchronize(c->stream));
            memset(out, 0, (size_t)w * h * sizeof(uint32_t));
            return RT_OK;
        }
        // read-back in four row blocks through page-locked staging: block k+1 crosses the bus while block k is
        // copied into the caller's (pageable) buffer
        size_t off[5];
        for (int k = 0; k <= 4; ++k) off[k] = ((size_t)h * k / 4) * (size_t)w;
        for (int k = 0; k < 4; ++k) {
            if (off[k + 1] > off[k])
                HIP_TRY(hipMemcpyAsync(e->h_pix + off[k], c->d_pixels + off[k], (off[k + 1] - off[k]) * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipEventRecord(e->ev[k], c->stream));
        }
        for (int k = 0; k < 4; ++k) {
            HIP_TRY(hipEventSynchronize(e->ev[k]));
            if (off[k + 1] > off[k]) memcpy(out + off[k], e->h_pix + off[k], (off[k + 1] - off[k]) * sizeof(uint32_t));
        }
        return RT_OK;
    };
    rc = run();
    if (rc != RT_OK) {
        char keep[sizeof g_err];
        memcpy(keep, g_err, sizeof keep);
        cache_drop(*e);                 // never reuse a context that failed half-way
        memcpy(g_err, keep, sizeof keep);
    }
    return rc;
}

}  // extern "C"
