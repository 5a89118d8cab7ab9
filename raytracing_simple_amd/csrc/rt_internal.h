// rt_internal.h -- what the translation units of the library share behind the C ABI: the context record and the records embedded in it
// (Choice, TileOrder, FrameState, Owned, Scene, Planes, Knobs), error reporting, acquisition of device resources into the context's record, page-locked
// staging (Staged), the frame's geometry said once, the checks and the blocking read several units share, and the hooks of the multi-device
// context (rt_multi.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "rt_choice.h"
#include "rt_device.h"
#include "rt_frame_state.h"
#include "rt_owned.h"
#include "rt_scene_state.h"
#include "rt_tile_order.h"

struct rt_multi;                    // rt_multi.hip
struct rt_ctx;

namespace rt {

constexpr int kMergeMax = 16;           // rt_merge_async: dst + 15 sources

// Adaptive sampling (rt_tiles.hip; include/rt_api.h "adaptive sampling"): the device arrays.  What they currently mean -- ragged, the selection, what
// the list was built from -- is host state of the frame: rt_frame_state.h.
struct TileSubset {
    uint32_t *d_passes = nullptr;       // one word per 8x8 tile of the local pixel buffer (rt_compare_tiles' indexing); acquired on first use (tiles_ensure).  Its content
                                        // means something only while the frame is ragged: otherwise every tile holds current_sample passes and nothing is stored
    uint32_t *d_selected = nullptr;     // one flag per group (rt_select_tiles), then two words: selected groups, the 8x8 tiles they cover
    uint32_t *d_list = nullptr;         // the subset launch's tile list: the launch tiles of the selected groups, padded with the sentinel to whole grid rows
    uint32_t *d_groups = nullptr;       // rt_denoise_pair_tiles_async (rt_denoise.hip): the selected groups' indices in ascending order, then the sentinel; one
                                        // word per group, acquired on that call's first use (tiles_build_group_list)
};

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return rt::fail(RT_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                               \
    } while (0)
// ... and a call that has said so itself (fail): its code is passed on
#define RT_TRY(call)                    \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != RT_OK) return rc_;   \
    } while (0)

// ---- acquisition into a record (rt_owned.h): the handle is entered where it is made, so whatever fails later, teardown finds it ----
// (the take_* forms return the runtime's answer for callers that report it in words of their own; a failed call enters nothing and leaves null)
template <class T> inline hipError_t take_device(Owned &owned, T **p, size_t count) {
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T));
    if (e == hipSuccess) owned.adopt(Owned::Kind::Device, *p);
    else *p = nullptr;
    return e;
}
template <class T> inline hipError_t take_pinned(Owned &owned, T **p, size_t count) {
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(p), count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) owned.adopt(Owned::Kind::Pinned, *p);
    else *p = nullptr;
    return e;
}
inline hipError_t take_event(Owned &owned, hipEvent_t *ev, unsigned flags) {
    const hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) owned.adopt(Owned::Kind::Event, *ev);
    else *ev = nullptr;
    return e;
}
inline int own_failed(const char *what, hipError_t e, const char *file, int line) {
    return fail(RT_ERR_HIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
// `count` elements of *p's type; RT_ERR_HIP with the caller's file and line, as HIP_TRY says it
template <class T> inline int own_device(Owned &owned, T **p, size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    const hipError_t e = take_device(owned, p, count);
    return e == hipSuccess ? RT_OK : own_failed("hipMalloc", e, file, line);
}
template <class T> inline int own_pinned(Owned &owned, T **p, size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    const hipError_t e = take_pinned(owned, p, count);
    return e == hipSuccess ? RT_OK : own_failed("hipHostMalloc", e, file, line);
}
inline int own_event(Owned &owned, hipEvent_t *ev, unsigned flags = hipEventDefault, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    const hipError_t e = take_event(owned, ev, flags);
    return e == hipSuccess ? RT_OK : own_failed("hipEventCreateWithFlags", e, file, line);
}
inline int own_stream(Owned &owned, hipStream_t *s, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {      // non-blocking, like every stream of the library
    const hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    if (e != hipSuccess) return own_failed("hipStreamCreateWithFlags", e, file, line);
    owned.adopt(Owned::Kind::Stream, *s);
    return RT_OK;
}
inline int own_registered(Owned &owned, void *host, size_t bytes, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {   // a caller's buffer, page-locked in place
    const hipError_t e = hipHostRegister(host, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return own_failed("hipHostRegister", e, file, line);
    owned.adopt(Owned::Kind::Registered, host);
    return RT_OK;
}
// "acquired on first use": nothing when *p is there already
template <class T> inline int ensure_device(Owned &owned, T **p, size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    return *p ? RT_OK : own_device(owned, p, count, file, line);
}

// ---- page-locked staging: N slots of one block, an event behind the copy that reads each slot.  A slot is written only after the copy that last read it has
// completed; the HOST may go on reading it while its copy is pending (host()).  kRing: slots of a power of two, at least 64, elements; otherwise exactly what is asked ----
template <class T, int N, bool kRing = false> struct Staged {
    T *block = nullptr;
    size_t cap = 0;                     // elements per slot
    int next = 0, cur = 0;              // the slot the next acquire takes; the one last handed out
    hipEvent_t ev[N] = {};
    bool pending[N] = {};               // a copy recorded by ev[k] reads slot k

    T *host() const { return block + (size_t)cur * cap; }
    int ensure_events(Owned &owned, unsigned flags, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {     // ... made now, not by the first sent()
        for (int k = 0; k < N; ++k)
            if (!ev[k]) RT_TRY(own_event(owned, &ev[k], flags, file, line));
        return RT_OK;
    }
    int settle(int k) {
        if (pending[k]) HIP_TRY(hipEventSynchronize(ev[k]));
        pending[k] = false;
        return RT_OK;
    }
    // the next slot, round robin, with room for `count` elements and nothing reading it.  A larger block is acquired BEFORE the old one goes (behind every pending
    // copy): a failure leaves the staging as it was
    int acquire(Owned &owned, size_t count, T **out, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (count > cap) {
            size_t grown_cap = kRing ? 64 : count;
            while (grown_cap < count) grown_cap *= 2;
            for (int k = 0; k < N; ++k) RT_TRY(settle(k));
            T *grown = nullptr;
            RT_TRY(own_pinned(owned, &grown, grown_cap * N, file, line));
            owned.drop(block);
            block = grown;
            cap = grown_cap;
        }
        cur = next;
        next = (next + 1) % N;
        RT_TRY(settle(cur));
        *out = host();
        return RT_OK;
    }
    // a copy out of the slot last handed out has been queued on `stream`
    int sent(Owned &owned, hipStream_t stream, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (!ev[cur]) RT_TRY(own_event(owned, &ev[cur], hipEventDisableTiming, file, line));
        HIP_TRY(hipEventRecord(ev[cur], stream));
        pending[cur] = true;
        return RT_OK;
    }
    void give_back(Owned &owned) {      // the block dropped (the caller knows that nothing reads it), the events kept
        owned.drop(block);
        block = nullptr;
        cap = 0;
        for (int k = 0; k < N; ++k) pending[k] = false;
    }
};

// What a context holds of its scene: the state (rt_scene_state.h) and the blocks it speaks of.  Raw pointers, freed by value through Owned
struct Scene {
    SceneState state;
    // raw records + the tables the device-side build kernel derives from them, one allocation
    rt_sphere *d_spheres = nullptr;
    float4 *d_tables = nullptr;         // geom | emis | colr | lightA | lightB, each `cap` entries
    uint32_t cap = 0;                   // records the blocks below are sized for (rt_scene.hip ensure_scene_capacity)
    SceneTables tables{};               // ... as the kernels' argument
    std::vector<unsigned char> is_light;   // host mirror of the light test per sphere (sizes the light list)
    std::vector<rt_sphere> h_spheres;      // host mirror of the records (an identical rt_set_scene uploads nothing)
    Staged<rt_sphere, 4, true> ring;    // sphere uploads go through it
    // hierarchy over the small spheres of a large scene (rt_device.h BvhTables), rebuilt with the tables; current while state.bvh_ok
    float4 *d_bvh = nullptr;            // blob of bvh_blob_capacity(cap) float4
    BvhTables bvh{};
    Staged<float4, 1> tree_stage;       // a host-shaped tree is written into it (rt_bvh.hip upload_host_tree)
    // records that repeat an EARLIER record bit for bit in what a ray test reads ({centre, radius^2}) stay out of the hierarchy (rt_bvh.hip mark_duplicates):
    // one byte per record on the device, uploaded only while the scene has such records (state.have_dups)
    uint8_t *d_dup = nullptr;           // [cap]
    Staged<uint8_t, 1> dup_stage;       // [cap] too: given back with the blocks above
    // feature planes (rt_features.hip; include/rt_api.h "feature planes"): what lies under every pixel, from scene and camera alone -- so it is kept here,
    // not in the frame's state; current while state.features_current
    float *d_features = nullptr;        // [h][w][8]: albedo, normal, distance, scene index; acquired on first use
};

// The planes a context derives from its colour plane, and the two settings that steer how (turning one on or off moves no plane).  Raw pointers, freed
// by value through Owned; every block is acquired on first use by the call that forms it.  Rows run as the colour plane's; "packed" is one word per pixel
// by toInt in the pixel buffer's layout (row 0 at the bottom).  WHEN a plane is current is the frame record's and the scene record's to say, through the
// predicates below rt_ctx (features_current ... atrous_current); the feature plane itself is the scene's (Scene::d_features).
//   plane          layout                              formed by
//   denoise        [h][w][3]                           rt_denoise_async: what the filter writes, EXCHANGED with rt_ctx::d_colors after every call
//   var            [h][w][3]                           rt_denoise_async, rt_denoise_pair*_async: the smoothed variance (of a pair: the first context's, for both)
//   filtered, _px  [h][w][3], packed                   rt_denoise_pair*_async: this half filtered with the other half's weights (rt_compare_filtered reads _px)
//   temporal, _px  [h][w][4] (rgb, n), packed          rt_reproject_async INTO this context
//   moments        [h][w][4] (m1, m2, k, v)            ... while the moments setting of this context is on
//   flags          [h][w] bytes, 0 or 1                ... while the shadow-history setting of this context is on (rule 31; current while flags_formed beside T)
//   pairs          5 float4 a pair, pairs_cap pairs    ... the same call's pair list (rule 29), staged through pair_stage without a host wait
//   atrous, _px    [h][w][4] (rgb, variance), packed   rt_atrous_async, like the three below
//   tmp            [h][w][4]                           the other (rgb, variance) plane the levels alternate with
//   guide          [h][w][4]                           the normal and the scene index of the feature plane, one aligned texel
//   n              [h][w]                              the sample count of a usable pixel, +0.0f for one that is not (rule 20)
struct Planes {
    float *denoise = nullptr, *var = nullptr, *filtered = nullptr, *temporal = nullptr, *moments = nullptr, *atrous = nullptr, *tmp = nullptr, *guide = nullptr, *n = nullptr;
    uint32_t *filtered_px = nullptr, *temporal_px = nullptr, *atrous_px = nullptr;
    struct { rt_guide_params params{}; bool on = false; } guide_set;        // rt_set_denoise_guide: what the filters of a pair of halves add to their weights
    struct { rt_moments_params params{}; bool on = false; } moments_set;    // rt_set_temporal_moments: what rt_reproject_async into the context and rt_atrous_async of it consult
    // shadow-aware history (rt_reproject.hip; include/rt_api.h "shadow-aware history")
    uint8_t *flags = nullptr;
    bool flags_formed = false;          // the reprojection that formed the temporal plane ran with the setting on: K is current while T is
    float4 *pairs = nullptr;
    size_t pairs_cap = 0;               // pairs the block holds room for
    Staged<float4, 4, true> pair_stage;
    struct { rt_shadow_history_params params{}; bool on = false; } shadow_set;     // rt_set_shadow_history: what rt_reproject_async into the context consults
};

// the rows of an image of `h` that rank `rank` of `nranks` renders, the image dealt out in tiles of `tile_rows` (api.local_rows_of says the same in Python)
inline int rows_of_rank(int h, int rank, int nranks, int tile_rows) {
    const int n_tiles = (h + tile_rows - 1) / tile_rows;
    int rows = 0;
    for (int t = rank; t < n_tiles; t += nranks) rows += (t * tile_rows + tile_rows <= h) ? tile_rows : (h - t * tile_rows);
    return rows;
}

}  // namespace rt

struct rt_ctx {
    rt::Owned owned;                    // every device block, page-locked block, registered range, event and stream below (rt_owned.h): entered by the own_* /
                                        // ensure_device helpers where it is acquired, given back by rt_destroy -- no member is freed by name
    int device = 0;
    int w = 0, h = 0;
    int rank = 0, nranks = 1, tile_rows = 8, local_rows = 0;
    rt_multi *multi = nullptr;          // non-null: this record is the front of a multi-device context
    uint32_t *d_seeds = nullptr;
    uint32_t *d_seeds0 = nullptr;       // pristine default stream, for device-side resets
    float *d_colors = nullptr;
    uint32_t *d_pixels = nullptr;
    uint32_t *d_pixels_ext = nullptr;   // caller-owned target of rt_set_pixel_buffer, or null
    void *pinned_out = nullptr;         // host buffer page-locked by rt_pin_output, or null
    int pixel_write = 1;                // rt_set_pixel_write
    rt::FrameState frame;               // what the progressive frame currently is: pass number, seed stream, packed pixels, launch count, tile bookkeeping
    rt::TileSubset tiles;               // adaptive sampling (rt_tiles.hip): a pass count per 8x8 tile, the selected groups, the launch list of a subset launch
    rt::Planes planes;                  // what is derived from the colour plane: the filters' and the reprojection's planes, and the two settings (above)
    void *d_compare = nullptr;          // scratch of the blocking rt_compare / rt_render_converged: one rt_frame_error, then the tile map (rt_compare.hip; acquired on first use)
    unsigned long long *d_counters = nullptr;
    unsigned long long *d_stats = nullptr;      // rt::kStatReplicas x 8 partial work counters
    rt::Scene scene;                    // what the context holds of its scene: records, tables, hierarchy, duplicate flags, feature plane, their staging -- and what of
                                        // that is currently true (rt_scene_state.h)
    rt_camera cam{};                    // a kernel argument (scene.state.have_cam)
    rt::Choice choice;                  // hierarchy or sweep, cooperative any-hit or not: the verdicts for this scene, the measurement behind them, the estimate (rt_choice.h)
    hipEvent_t probe_ev[4] = { nullptr, nullptr, nullptr, nullptr };       // ... and the measurement's events: arm a's timed step lies between probe_ev[2 * a] and probe_ev[2 * a + 1]
    rt::TileOrder order;                // heavy-first tile schedule (rt_tile_order.h; rt_trace.inc.h reads and writes its arrays)
    rt::Knobs knobs;                    // what a launch is made of besides: arithmetic mode, thresholds, the hierarchy's and the walk's knobs, diagnostics knobs (rt_instance.h)
    const char *last_kernel = "";       // symbol of the instance the last launch used
    const char *last_features_kernel = "";      // ... of the kernel the last rt_features_async launched (rt_features.hip)
    unsigned long long debug_counters[24] = {};   // diagnostic instances only
    hipStream_t stream = nullptr;       // the context's own (non-blocking) stream
    hipStream_t last_stream = nullptr;  // stream of the most recent launch / update (what readers wait for)
    bool used_foreign_stream = false;   // some launch went to a caller's stream
    bool abandon_streams = false;       // a shard of a multi-device context whose gather failed: its stream may hold a transfer that never
                                        // completes, so rt_destroy does not wait for it
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_dep = nullptr;
    // rt_throttle: the rt_render_async launches in flight, each between two events (a ring, oldest at flight_next)
    struct Flight {
        hipEvent_t start = nullptr, stop = nullptr;
        int n_samples = 0;
        bool pending = false;
    };
    static constexpr int kFlights = 8;
    Flight flight[kFlights];
    int flight_next = 0;
    bool throttle_on = false;
    double flight_ms_per_pass = 0.0;    // device time per pass of the most recent finished launch
    // diagnostics build: device wall-clock logs
    unsigned long long *d_timelog = nullptr, *d_wavelog = nullptr, *d_blocklog = nullptr;
    uint32_t *d_stalelog = nullptr;
    uint32_t timelog_cap = 0, timelog_used = 0, wavelog_cap = 0;
    unsigned long long timelog_tag = 0;
};

namespace rt {

// ---- the frame's geometry on the host (the kernels keep their own arithmetic) ----
inline uint32_t tiles_per_row(const rt_ctx *c) { return (uint32_t)((c->w + 7) / 8); }                  // 8x8 tiles
inline uint32_t tile_row_count(const rt_ctx *c) { return (uint32_t)((c->local_rows + 7) / 8); }        // ... of the local pixel buffer
inline uint32_t tile_count(const rt_ctx *c) { return tiles_per_row(c) * tile_row_count(c); }
inline uint32_t groups_per_row(const rt_ctx *c) { return (tiles_per_row(c) + 3) / 4; }                 // groups of four tiles (rt_tiles.hip)
inline uint32_t group_count(const rt_ctx *c) { return groups_per_row(c) * tile_row_count(c); }
inline size_t image_pixels(const rt_ctx *c) { return (size_t)c->w * (size_t)c->h; }                    // the full image, whatever rows the context renders
inline size_t local_pixels(const rt_ctx *c) { return (size_t)c->local_rows * (size_t)c->w; }
inline size_t color_floats(const rt_ctx *c) { return 3 * image_pixels(c); }
inline uint32_t *frame_pixels(const rt_ctx *c) { return c->d_pixels_ext ? c->d_pixels_ext : c->d_pixels; }     // the buffer launches write

// ---- when a derived plane is CURRENT, said once: the frame record's flag, the scene record's where it applies, and the blocks ----
inline bool features_current(const rt_ctx *c) { return c->scene.state.features_current && c->scene.d_features; }
inline bool filtered_current(const rt_ctx *c) { return c->frame.filtered_pair != 0 && c->planes.filtered && c->planes.filtered_px; }
inline bool temporal_current(const rt_ctx *c) { return c->frame.temporal_current && features_current(c) && c->planes.temporal && c->planes.temporal_px; }
inline bool moments_current(const rt_ctx *c) { return temporal_current(c) && c->frame.moments_formed && c->planes.moments; }
inline bool flags_current(const rt_ctx *c) { return temporal_current(c) && c->planes.flags_formed && c->planes.flags; }
inline bool atrous_current(const rt_ctx *c) { return c->frame.atrous_current && features_current(c) && c->planes.atrous && c->planes.atrous_px; }
// ... and what a reader of one needs beside that: the name of its buffer in the "is null" refusal (null: the call takes two buffers), what the
// context "holds no current" of, the plane with its length in floats, and the packed plane of a call that hands out two
enum class Plane { Features, Filtered, Temporal, Moments, Atrous };
struct PlaneView { bool current; const char *host_name, *absent; const float *plane; size_t floats; const uint32_t *packed; };
inline PlaneView plane_view(const rt_ctx *c, Plane which) {
    const size_t px = image_pixels(c);
    switch (which) {
    case Plane::Features:
        return { features_current(c), "out_host", "feature plane (rt_features_async forms one; rt_set_scene, rt_update_spheres_async and rt_set_camera end it)",
                 c->scene.d_features, 8 * px, nullptr };
    case Plane::Filtered:
        return { filtered_current(c), "out_host", "cross-filtered plane (rt_denoise_pair_async makes one; whatever moves the colour plane ends it)", c->planes.filtered,
                 3 * px, nullptr };
    case Plane::Temporal:
        return { temporal_current(c), nullptr, "temporal plane (rt_reproject_async forms one; whatever moves the colour plane or ends the feature plane ends it)",
                 c->planes.temporal, 4 * px, c->planes.temporal_px };
    case Plane::Moments:
        return { moments_current(c), "m_host", "moments plane (rt_reproject_async into it forms one while rt_set_temporal_moments is on; whatever ends the temporal plane, "
                 "or a reprojection into the context with the setting off, ends it)", c->planes.moments, 4 * px, nullptr };
    case Plane::Atrous:
        break;
    }
    return { atrous_current(c), nullptr, "filtered plane (rt_atrous_async forms one; whatever ends the temporal plane, a new rt_reproject_async into the context or a "
             "feature plane formed again ends it)", c->planes.atrous, 4 * px, c->planes.atrous_px };
}

// a reset or a written state ends a frame of the current scene for the form choice too (Choice::frame_ended): end_frame(c).reset_in_place()
inline FrameState &end_frame(rt_ctx *c) { c->choice.frame_ended(); return c->frame; }

// ---- rt_api.hip: the context's device and the order of its work ----
int select_device(const rt_ctx *c);
int chain(rt_ctx *c, hipStream_t stream);          // `stream` waits for whatever the context queued last elsewhere (ALL its work runs in issue order)
int chain_all(hipStream_t stream, std::initializer_list<rt_ctx *> ctxs);      // ... for each context in turn, up to the first failure
int wait_all(rt_ctx *c);                            // host waits for everything the context has queued
int refresh_pixels(rt_ctx *c, hipStream_t stream); // the packed frame brought up to date on `stream` (already chained): the pack kernel, if the last launches ran with the pixel store off
const double *create_breakdown();                   // host ms of the last rt_create by phase (rt_debug_create_breakdown)
// blocking read of `bytes` from the context's device: behind everything it has queued, on its own stream (wait = false: the copy is queued, a later call waits)
int read_back(rt_ctx *c, void *host, const void *dev, size_t bytes, bool wait = true);
// the five rt_read_* calls: a plane of the context (plane_view above) and / or, for Temporal and Atrous, its packed plane, either buffer null for "not this one".
// RT_ERR_ARG for a context the adaptive calls do not take or no buffer at all; RT_ERR_STATE unless the plane is current.  Two copies: the wait is for the last one
int read_plane(rt_ctx *c, const char *call, Plane which, float *host, uint32_t *packed_host = nullptr);
// What a filter of the frame reads: the temporal plane (4 floats a pixel, each with its own n) while that is current, else the colour plane (3 floats, every
// pixel at `passes`), else RT_ERR_STATE "<call>: <who> holds neither a current temporal plane nor a pass".  m: the moments plane, if wanted and current
struct PlaneInput { const float *u; int channels; float passes; const float4 *m; };      // (passes: current_sample, whichever plane)
int filter_input(const rt_ctx *c, const char *call, const char *who, bool want_moments, PlaneInput *out);
inline int ragged_refuse(const rt_ctx *c, const char *call, const char *who) {      // ... and both take whole frames only
    return c->frame.ragged ? fail(RT_ERR_STATE, "%s: %s is ragged (its tiles hold different pass counts)", call, who) : RT_OK;
}
// `a` and `b` show the same frame on the same device: non-null, distinct, neither multi-device, same size (`sharding`: and rank, ranks, rows per
// tile), same device -- or RT_ERR_ARG with a message that names `call`, the two contexts as the caller knows them, and the property that differs
int same_frame(const rt_ctx *a, const rt_ctx *b, const char *call, const char *a_name, const char *b_name, bool sharding = true);

// ---- rt_launch.hip: one launch of the render kernel ----
LaunchParams make_params(rt_ctx *c, int n_samples);
const Instance *instances(bool fast, int *count);
SceneFacts scene_facts(const rt_ctx *c);            // what the rule that picks the instance (rt_instance.h) reads of the context's scene
bool tables_fit_lds(const rt_ctx *c, int n_samples);
void probe_poll(rt_ctx *c, bool wait);              // the verdict of the measurement in flight, if its events have completed (Choice::times_arrived)
int refresh_tables(rt_ctx *c, hipStream_t stream);     // rt_scene.hip: tables and hierarchy from the records as they are now, if updates made them stale
int launch(rt_ctx *c, int n_samples, hipStream_t stream, bool may_block = false);

// ---- rt_scene.hip: records, tables, staging ----
int ensure_scene_capacity(rt_ctx *c, uint32_t count);
int upload_spheres(rt_ctx *c, uint32_t first, uint32_t count, const rt_sphere *spheres, uint32_t n_total, hipStream_t stream, bool full_upload);

// the hierarchy of large scenes (rt_bvh.hip): per-device set-up of the build kernel; build on `stream` for the scene the
// context's host mirror holds (sets c->scene.bvh, reports to c->scene.state; nothing is read back)
hipError_t prepare_bvh_build();
int build_bvh(rt_ctx *c, uint32_t n_total, hipStream_t stream, bool full_upload = false);
int render_shard(rt_ctx *c, int n_samples, bool may_block);      // rt_launch.hip: one shard's launch on its own stream

// ---- rt_denoise.hip: the cross-filtered halves, for the paired loops of rt_compare.hip ----
int denoise_pair_refuse(const rt_ctx *a, const rt_ctx *b, const char *call);     // the contexts rt_denoise_pair_async does not take, and pass numbers that differ or are zero
int denoise_pair(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream);    // a checked pair, checked parameters: the planes made on `stream`, both marked current
// ... the same pair and parameters: the planes of the groups in the current selection made again, if the planes are one selection behind (FrameState::filtered_behind);
// RT_OK and nothing launched if they are current; RT_ERR_STATE for anything else, `call` named in the message
int denoise_pair_tiles(rt_ctx *a, rt_ctx *b, const rt_denoise_params &q, hipStream_t stream, const char *call);

// ---- rt_features.hip: the feature plane, for every call that reads it ----
// RT_ERR_STATE unless c's feature plane is current; the message reads "<call>: <lead>the feature plane<of_whom> is not current (...)"
int features_refuse(const rt_ctx *c, const char *call, const char *lead = "", const char *of_whom = "");
// the guide of a pair of halves (rt_set_denoise_guide): RT_ERR_STATE when the two settings differ, or -- on -- a feature plane is not current.  *guided: on
int guide_refuse(const rt_ctx *a, const rt_ctx *b, const char *call, bool *guided = nullptr);

// ---- rt_tiles.hip: the subset launch's device side ----
int tiles_refuse(const rt_ctx *c, const char *call);                  // RT_ERR_ARG for the contexts the adaptive calls do not take (null, multi-device, sharded)
int tiles_ensure(rt_ctx *c);                                          // the three device arrays of rt_ctx::tiles, on first use
int merge_by_tile(rt_ctx *dst, rt_ctx *const *srcs, int n_srcs, int total, hipStream_t stream);   // rt_merge_async with a ragged context among them (checked by the caller)
int tiles_build_list(rt_ctx *c, int waves, bool by_order, uint32_t n_launch, uint32_t slots, hipStream_t stream);   // d_list for an instance of `waves` wavefronts
int tiles_build_group_list(rt_ctx *c, hipStream_t stream);            // d_groups (acquired on first use): the selected groups in ascending order, by the same kernel
int tiles_advance(rt_ctx *c, int n_samples, hipStream_t stream);      // + n_samples on every tile of every selected group (the array made explicit first)
int launch_tiles(rt_ctx *c, int n_samples, hipStream_t stream);       // rt_launch.hip: n_samples passes on the selected groups

// multi-device context (rt_multi.hip); `front` is the rt_ctx whose `multi` points at the record
void multi_destroy(rt_ctx *front);
int multi_set_scene(rt_ctx *front, const rt_sphere *spheres, uint32_t count);
int multi_update_spheres(rt_ctx *front, uint32_t first, uint32_t count, const rt_sphere *spheres);
int multi_set_camera(rt_ctx *front, const rt_camera *cam);
int multi_set_mode(rt_ctx *front, int mode);
int multi_reset(rt_ctx *front, bool async);
int multi_render(rt_ctx *front, uint32_t *out_host, int n_samples, bool blocking);
int multi_set_pixel_write(rt_ctx *front, int enable);
int multi_read_pixels(rt_ctx *front, uint32_t *out_host);
int multi_read_colors(rt_ctx *front, float *out_host);
int multi_read_seeds(rt_ctx *front, uint32_t *out_host);
int multi_get_stats(rt_ctx *front, rt_stats *out);
int multi_device_pixels(rt_ctx *front, void **dptr, size_t *count);
int multi_pin_output(rt_ctx *front, uint32_t *out_host, size_t count);
void *multi_stream(rt_ctx *front);
int multi_shards(const rt_ctx *front);
int multi_wait_frame(rt_ctx *front);
const char *multi_last_kernel(const rt_ctx *front);
rt_ctx *multi_first_shard(rt_ctx *front);
rt_ctx *multi_shard(rt_ctx *front, int r);
int multi_debug_each(rt_ctx *front, int (*fn)(rt_ctx *, int), int arg);
int debug_layout_for_mode(rt_ctx *c);                 // diagnostics (rt_debug.hip): rt_set_mode of an A/B instance builds the pair table it reads
int multi_debug_break(rt_ctx *front);
int multi_debug_set_rccl(const char *path, int repeated_counts_as_distinct);   // diagnostics build

}  // namespace rt
