/*
 * rt_api.h -- C ABI of the MI355X (gfx950) render path for RayTracing_Simple.
 *
 * This is the drop-in boundary: everything the reference's OpenCL backend does between
 * `Config::updateRendering()` and the pixel buffer -- the `RayTracing` kernel
 * (SimpleRT/kernel/RayTracing_Kernel.cl:551-600) and its launch wrapper
 * `OpenCLConfigBuffer` (SimpleRT/src/OpenCLConfig.cpp:398-747) -- behind plain C entry
 * points: POD structs, raw pointers and sizes, int status codes, no C++/torch types.
 * INTEGRATION.md shows the `HipConfig : Config` adapter the reference host would add.
 *
 * All file:line citations are relative to the reference checkout (SimpleRT/...).
 * Threading: calls on one rt_ctx are not re-entrant; any thread may make them (each entry
 * point selects the context's device itself).  Nothing here throws or exits.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with hidden visibility: exactly the functions declared in this header
 * (and, in the diagnostics build librt_hip_diag.so, in rt_debug.h) are exported.               */
#if defined(RT_BUILDING_LIBRARY)
#define RT_API __attribute__((visibility("default")))
#else
#define RT_API
#endif

/* ---- data layouts: identical, byte for byte, to the reference's host structs ---------- */
typedef struct { float x, y, z; } rt_vec3;                /* include/Vec.hpp:10-34   (12 B) */

enum { RT_DIFF = 0, RT_SPEC = 1, RT_REFR = 2 };           /* include/Sphere.hpp:6-8         */

typedef struct {                                          /* include/Sphere.hpp:11-15 (44 B) */
    float   rad;
    rt_vec3 p, e, c;                                      /* centre, emission, colour        */
    int32_t refl;                                         /* RT_DIFF / RT_SPEC / RT_REFR     */
} rt_sphere;

typedef struct {                                          /* include/Camera.hpp:7-14  (60 B) */
    rt_vec3 orig, target;                                 /* set by the user                 */
    rt_vec3 dir, x, y;                                    /* computeCameraVariables' output  */
} rt_camera;

typedef struct {                                          /* `sphere`, `sphereCount` kernel  */
    const rt_sphere *spheres;                             /*  arguments (.cl:553-554)        */
    uint32_t         count;
} rt_scene;

/* Exact work counters of everything rendered since rt_create()/rt_reset(). */
typedef struct {
    uint64_t samples;        /* camera (primary) rays                                         */
    uint64_t closest_rays;   /* closest-hit queries, `Intersect` .cl:215 (primary+extension)  */
    uint64_t shadow_rays;    /* any-hit queries, `IntersectP` .cl:234                         */
    uint64_t sphere_tests;   /* `SphereIntersect` .cl:173 evaluations OF THE REFERENCE'S ALGORITHM for these rays: every closest-hit
                              * query counts all spheres, every shadow query the spheres up to and including its first blocker in
                              * scene order (.cl:215-247).  The plain sweeps execute exactly these tests; the hierarchy of large
                              * scenes (rt_last_kernel "..._pairs") reaches the same answers with far fewer, so there this is the
                              * reference-equivalent count, equal to the oracle's, not the work done: what the walk executes is
                              * counted by the census instance of the diagnostics library (bench.py `roofline.executed`).     */
    uint64_t rng_draws;      /* `GetRandom` .cl:143 calls                                     */
    uint64_t launches;       /* kernel launches                                               */
    double   last_kernel_ms; /* device time of the last rt_render_pass launch (HIP events)    */
} rt_stats;

enum rt_status {
    RT_OK            =  0,
    RT_ERR_ARG       = -1,   /* null pointer, non-positive size, bad enum, scene too large    */
    RT_ERR_NO_DEVICE = -2,   /* no usable gfx950 device / HIP runtime                         */
    RT_ERR_HIP       = -3,   /* a HIP call failed; rt_last_error() has the text               */
    RT_ERR_ALLOC     = -4,
    RT_ERR_STATE     = -5    /* render requested before a scene and a camera were set         */
};

enum rt_mode {
    RT_MODE_PARITY = 0,      /* strict binary32, no contraction, restated libm: bit-exact     */
    RT_MODE_FAST   = 1       /* FMA contraction + hardware rcp/rsq/sin/cos/exp2/log2: an approximation of the reference
                              * path whose tolerance is PSNR >= 50 dB against it at equal sample count (north_star).  It
                              * MEETS that on scenes without many small curved mirrors / glass spheres -- the Demo scene at
                              * 1080p x 64 (61.7 dB) and 2160p x 256 (64.3), the 16-sphere scene (58.3) -- and it does NOT on
                              * 256 scattered spheres at 32 spp (46.0), 1024 at 16 spp (37.6) or the 64-sphere mirror box
                              * (27.1): there a last-bit difference in a direction, amplified by curved reflections, flips a
                              * hit decision, and from that sample on the pixel's one sequential random stream (.cl:143-169)
                              * is consumed differently -- the frames then differ at the noise level although both are correct
                              * renderings.  Use RT_MODE_PARITY where the tolerance matters on such scenes.  Measured per
                              * configuration by tools/fast_gate.py (profiles/r06_fast_gate.jsonl), held by
                              * tests/test_gpu_parity.py::test_fast_mode_against_north_star_gate.                        */
};

#define RT_MAX_SPHERES 262144u /* (the hierarchy numbers its leaves of 8 spheres with 15 bits.  Its tables are staged in LDS while
                                 * five workgroups of that size fit a CU -- 31 KiB, about 1 100 spheres; to about 3 200 spheres its
                                 * pairs still are and only the leaves' spheres are read from HBM / L2 ("..._pairs_m"); beyond,
                                 * everything is ("..._pairs_g"); the plain sweep stages its tables while four workgroups fit a CU
                                 * -- 40 KiB, about 2 500 records -- and reads them through the scalar cache beyond ("..._g"))        */

typedef struct rt_ctx rt_ctx;

/* ---- the headline call ------------------------------------------------------------------
 * Equivalent to: a fresh OpenCLConfigBuffer(w,h) [seeds = never-seeded std::rand() stream
 * clamped to >= 2, OpenCLConfig.cpp:676-680] + sceneSetup + `spp` calls of
 * Config::updateRendering() [Config.cpp:73-81], after which `out` holds what getPixels()
 * returns: out[y*w+x] = R | G<<8 | B<<16, row 0 = bottom of the image (.cl:594-596).
 * `cam` carries dir/x/y already computed by the host (Utility.cpp:71-85).
 * `out` is a host buffer of w*h uint32.  Parity mode, device 0, blocking.
 * The library keeps the device state of the last few (w, h) it was called with -- buffers, the
 * device-resident default seed stream, page-locked staging for the read-back -- so that a host
 * which calls rt_render per frame pays for them once; rt_release_cache() frees it.
 * Thread-safe (calls are serialised inside).                                                  */
RT_API int rt_render(const rt_scene *scene, const rt_camera *cam, uint32_t *out, int w, int h, int spp);
RT_API void rt_release_cache(void);

/* ---- progressive interface: one context = one OpenCLConfigBuffer ------------------------ */

/* ctor + allocateBuffer (OpenCLConfig.cpp:398-400, 613-682): device buffers for colours
 * (12 B/px), seeds (8 B/px, initialised to the default stream) and pixels (4 B/px).         */
RT_API int rt_create(rt_ctx **out, int w, int h);

/* one context that renders on `ngpus` devices of this process (HIP devices
 * 0..ngpus-1; rt_create_multi_on names them).  The image is sharded by interleaved row tiles of
 * `tile_rows` rows (tile t -> device t % ngpus; 0 = the default of 8), every device renders its rows
 * on its own stream, and each frame ends with ONE gather to the first device over RCCL
 * (ncclGroupStart; root: ncclRecv x (n-1); others: ncclSend; ncclGroupEnd; ncclUint32), a
 * de-interleave kernel there and one copy to the host.  The receives and the de-interleave run on a SECOND stream of
 * the first device, into one of two receive slots, so that device's render of frame k + 1 overlaps the gather of frame k
 * (asynchronous frames: rt_render_async; rt_throttle(ctx, 0) and the blocking calls wait for the assembled frame).  Every other call of this header works on
 * such a context as on a plain one and means the whole image: rt_render_pass returns all h rows,
 * rt_get_stats sums the devices, rt_read_colors / rt_read_seeds merge them.  Results are bit-identical
 * to a one-device context by construction (pixels are independent); with ngpus = 1 there is nothing to move: no
 * communicator (RCCL is not loaded), no gather, no de-interleave -- the one shard renders straight into the frame.  One kernel instance renders the whole frame: the first shard measures hierarchy
 * against sweep (rt_scene_choice) and the others follow it.
 * STATUS of the n > 1 RCCL branch: it executes on one GPU against a test double of RCCL (tests/rccl_double.cpp, bound through the diagnostics
 * library's rt_debug_set_rccl_library: communicator, the grouped n - 1 receives and n - 1 sends, de-interleave -- on 2, 3 and 8 shards, C4 at
 * full size on 8 -- and every failure site: ncclGroupStart, ncclSend / ncclRecv inside the group, ncclGroupEnd); against librccl on distinct
 * devices over xGMI it has run on no hardware yet (tests/test_gpu_features.py holds that test, skipped below two devices): treat real links as
 * unverified until it has passed on a multi-GPU node.
 * rt_create_multi_on with ONE device listed ngpus times is that one-GPU rehearsal of the path: RCCL refuses two
 * ranks on one device, so the transfers into the root's receive slots are device-to-device copies there; everything
 * else (shards, slots, de-interleave) is unchanged.  A list that mixes repeated and distinct devices is refused
 * (RT_ERR_ARG).  If a gather fails half-way (an RCCL error inside the group or at ncclGroupEnd) the context is marked
 * unusable: every later call on it returns RT_ERR_STATE naming the failure, and only rt_destroy is meaningful -- it polls the
 * context's streams (never a blocking wait) for up to two seconds and frees everything once they have drained; only a context whose streams
 * still hold a transfer after that keeps its device memory and streams (a teardown that returns instead of hanging).    */
RT_API int rt_create_multi(rt_ctx **out, int w, int h, int ngpus);
RT_API int rt_create_multi_on(rt_ctx **out, int w, int h, const int *devices, int ngpus, int tile_rows);
RT_API int rt_shard_count(const rt_ctx *ctx);                     /* 1 for a plain context        */

/* Same, on HIP device `device`, rendering only the row tiles this rank owns: tile t (rows
 * [t*tile_rows, (t+1)*tile_rows)) belongs to rank t % nranks.  tile_rows must be a positive
 * multiple of 8.  The rank's rows are packed in order into a local pixel buffer of
 * rt_local_rows() rows (interleaved row tiles).  nranks = 1 is rt_create().       */
RT_API int rt_create_sharded(rt_ctx **out, int w, int h, int device, int rank, int nranks,
                             int tile_rows);

RT_API void rt_destroy(rt_ctx *ctx);                              /* freeBuffer, :684-717            */

/* sceneSetup (:720-747) + the per-pass sphere upload (:450).  Copies; caller keeps `spheres`.
 * The 44-byte records go to the device as they are and a small kernel there builds the tables the
 * render kernel reads (centre | radius^2, emission | material, colour | radius, and the light list
 * SampleLights walks, with 4*pi*radius^2 -- all in binary32, the reference's own operations).
 * Scenes with 56 and more small spheres also get a hierarchy over them, its shape chosen by surface area (below 1500 such
 * spheres on the host, which then also knows whether walking it will pay; up to 8192 by a second kernel on the same stream, the
 * caller held for microseconds; beyond that built on the host from the records and copied): it changes which instance renders
 * the scene, never the result (rt_last_kernel, rt_scene_choice).  Up to RT_MAX_SPHERES spheres; tables that do not fit LDS are read
 * from HBM / L2.  Ordered after every launch issued on this context; no device-wide synchronisation.  A refused
 * scene (bad arguments, too many spheres) leaves the previous one in place.                                                  */
RT_API int rt_set_scene(rt_ctx *ctx, const rt_sphere *spheres, uint32_t count);

/* Device-resident scene update: replace spheres [first, first+count) of the scene set
 * by rt_set_scene -- moving spheres, changed materials, lights switched on or off -- without a
 * host wait: the records are staged through page-locked memory and copied asynchronously on `hip_stream` (a hipStream_t;
 * NULL = the default stream, as for rt_render_async); launches issued later on this context see the new scene.  The tables and,
 * for large scenes, the hierarchy are rebuilt ONCE, by the device-side kernels on the stream of the next launch, however many
 * updates precede it (a host that moves 200 scattered spheres by 200 calls pays one rebuild, as for one call over the whole
 * range) -- up to 8192 spheres inside the tree by the device's own build by surface area, with no host wait; beyond that the
 * host builds the fixed (halved) shape from its mirror of the records and that launch waits for the previous such build's
 * upload to have left its staging buffer; the choice between hierarchy and sweep is kept.  The sphere count does not change.
 * `spheres` may be reused as soon as the call returns.                                          */
RT_API int rt_update_spheres_async(rt_ctx *ctx, uint32_t first, uint32_t count, const rt_sphere *spheres,
                                   void *hip_stream);

/* updateCamera's result + the per-pass camera upload (:418).  dir/x/y must be filled in.     */
RT_API int rt_set_camera(rt_ctx *ctx, const rt_camera *cam);

RT_API int rt_set_mode(rt_ctx *ctx, int mode);                    /* enum rt_mode; default parity    */

/* Back to pass 0: mCurrentSample = 0, seeds = default stream, counters cleared.              */
RT_API int rt_reset(rt_ctx *ctx);

/* rt_reset() without a host round trip: the next launch starts from a device-resident copy of
 * the default stream (read in place, nothing is copied) and the counters are cleared by a small
 * kernel on `hip_stream`.  The colour plane and the packed pixels are NOT cleared (pass 0 overwrites
 * every pixel, .cl:580-582): until the next launch rt_read_colors / rt_read_pixels still return the
 * previous frame, rt_read_seeds the default stream.  The launch counter and last_kernel_ms restart.
 * Like every call on a context it must not race with other calls on the same context.        */
RT_API int rt_reset_async(rt_ctx *ctx, void *hip_stream);

/* `n_samples` x { setArguments(); execute(); ++mCurrentSample; } (Config.cpp:73-81) as ONE
 * launch that keeps seeds and the running average in registers, then one D2H copy of the
 * pixel buffer into `out_host` (the full image for an unsharded context, the local rows for
 * a sharded one).  out_host may be NULL to skip the copy.  Blocking.
 * Scheduling, never results: launches leave what each tile cost them, and later launches walk the tiles heaviest first (sorted
 * again from the last costs whenever the scene or the camera has changed).  A long launch (8 passes and more) prices the tiles by
 * itself; a launch of 24 passes or more that has no costs to go by renders 4 of its passes first to get them, then the rest
 * heaviest first -- so a scene's first frame is a few percent slower than its later ones.  Short launches -- a pass per call, the
 * reference's own regime -- add their costs up instead, and the one that finds 16 passes' worth sorts from them: a host that only
 * ever launches a pass or two at a time gets the same order (8-23 % on scenes of hundreds of spheres and more) from its 17th pass on.  */
RT_API int rt_render_pass(rt_ctx *ctx, uint32_t *out_host, int n_samples);

/* Page-lock the host buffer that rt_render_pass copies into (the host's `pPixels`,
 * OpenCLConfig.cpp:618-621), so the per-pass readback of the reference's display loop
 * (clEnqueueReadBuffer after every pass, OpenCLConfig.cpp:498-512) runs at the full PCIe rate
 * instead of through a pageable staging copy.  `count` uint32 from `out_host` must stay valid
 * and at the same address until rt_pin_output(ctx, NULL, 0) or rt_destroy.  Optional.        */
RT_API int rt_pin_output(rt_ctx *ctx, uint32_t *out_host, size_t count);

/* enable = 0: later launches advance seeds and the running average but leave the packed pixel
 * buffer alone (no toInt, .cl:34,594-596, and no pixel store) -- for passes whose frame nobody
 * will look at; the next launch with enable = 1 writes every pixel of its frame from the running
 * average, so nothing is lost.  Default 1.                                                    */
RT_API int rt_set_pixel_write(rt_ctx *ctx, int enable);

/* getPixels() for hosts that skip pixel stores: brings the packed frame up to date -- if the last
 * launches ran with the pixel store off, a small kernel packs the frame from the running average
 * (same toInt, .cl:34,594-596) -- and copies it to `out_host` (local rows x w uint32).  Waits for
 * the launches issued on this context.  While the context is at pass 0 nothing is packed and the
 * pixels are unspecified: whatever the buffer held (rt_reset clears it, the other calls do not).  */
RT_API int rt_read_pixels(rt_ctx *ctx, uint32_t *out_host);

/* Same launch, asynchronous on `hip_stream` (a hipStream_t, NULL = default stream), no copy
 * and no synchronisation: the caller orders later work on that stream.                       */
RT_API int rt_render_async(rt_ctx *ctx, int n_samples, void *hip_stream);

/* rt_read_pixels without the wait: the packed frame is brought up to date and its copy to `out_host` is queued on
 * `hip_stream` behind everything issued on this context; the buffer holds the frame once that stream has drained (or
 * rt_throttle(ctx, 0, ...) has returned).  `out_host` should be page-locked (rt_pin_output), or the runtime stages
 * the copy and the call may block.  On a multi-device context this is rt_read_pixels (it blocks).               */
RT_API int rt_read_pixels_async(rt_ctx *ctx, uint32_t *out_host, void *hip_stream);

/* Pacing for hosts that queue passes with rt_render_async (the adapter's display loop): returns when at most
 * `max_in_flight` of the rt_render_async launches issued on this context since the first rt_throttle call are still
 * unfinished (0 = wait for all of them).  *ms_per_pass (may be NULL) receives the device time per pass of the most
 * recent launch that has finished, 0 if none has.  The first call only switches the bookkeeping on (two events per
 * launch from then on) and returns at once.  A multi-device context waits for everything when max_in_flight is 0
 * and reports no time.                                                                                          */
RT_API int rt_throttle(rt_ctx *ctx, int max_in_flight, double *ms_per_pass);

/* The context's own non-blocking stream (a hipStream_t), the one rt_render_pass uses.  With
 * several contexts in flight, rt_render_async(ctx, n, rt_stream(ctx)) runs each on its own.
 * HIP gives a process GPU_MAX_HW_QUEUES hardware queues (default 4) and lets further streams
 * share them: two contexts on one queue do not overlap at all, so a host that keeps F contexts
 * in flight should start with GPU_MAX_HW_QUEUES >= the number of streams it uses (bench.py: 8).
 * PLATFORM PRECONDITION (profiles/r02_stale_seed/): do not put more hardware queues on ONE GPU
 * than its scheduler keeps resident -- one process per GPU is always fine; four processes of 8 queues each on one
 * GPU were not: the scheduler then time-slices the queues, a dispatch can run XCD-share by XCD-share around a
 * descheduling, and on this driver stack the early share occasionally loses its writes (no fence or store form the
 * library could issue prevents it).  tools/gather_stress.py is the acceptance test for a deployment.
 * Of a MULTI-DEVICE context: the stream its assembled frame is complete on -- with several devices the first device's
 * gather stream, behind the receives and the de-interleave of the last frame queued (rt_render_async takes no stream there:
 * every device renders on its own).  Work queued on it after rt_render_async sees the whole frame in rt_device_pixels, and
 * the next frame's assembly waits for that work: this is the stream that orders the frame buffer.                    */
RT_API void *rt_stream(rt_ctx *ctx);

/* Device address and element count (uint32) of the local pixel buffer.                       */
RT_API int rt_device_pixels(rt_ctx *ctx, void **dptr, size_t *count);

/* Redirect the packed pixels of later launches into a caller-owned DEVICE buffer of at least
 * rt_local_rows()*w uint32 (e.g. the send buffer of the frame-end gather, so no copy is needed);
 * NULL restores the context's own buffer.  The caller keeps the buffer alive and orders its
 * reuse against the launches it issued.                                                      */
RT_API int rt_set_pixel_buffer(rt_ctx *ctx, void *dptr, size_t count);

RT_API int rt_local_rows(const rt_ctx *ctx);                      /* rows this context renders       */
RT_API int rt_current_sample(const rt_ctx *ctx);                  /* mCurrentSample                  */

/* Copies of the reference's other two buffers, for parity checks: the colour plane
 * (3 floats/px, y-flipped as .cl:579 stores it) and the seed pairs, full image size; rows
 * this rank does not own keep their initial content.                                         */
RT_API int rt_read_colors(rt_ctx *ctx, float *out_host);
RT_API int rt_read_seeds(rt_ctx *ctx, uint32_t *out_host);

/* ---- render state in and out: seed streams, checkpoints, merged frames ---------------------
 * A progressive render is three things -- the colour plane, the seed pairs and the pass number: the `colors`, `seeds` and
 * `currentSample` arguments of the reference's kernel (.cl:551-600), which continues whatever running average it is handed
 * (.cl:580-590).  rt_read_colors / rt_read_seeds / rt_current_sample read them; the calls below write them.  The render kernels
 * are the same: a launch reads its first pass's seeds and continues the average from the pass number, whatever put them there.
 * THIS LIBRARY'S OWN EXTENSION: the reference has one seed stream (OpenCLConfig.cpp:676-680) and never combines frames.  A frame
 * rendered on a stream other than 0, and a merged frame, are correct renderings of the scene that reproduce NO reference frame;
 * resuming a render (rt_write_state / rt_load_state of a state read earlier) reproduces the uninterrupted one bit for bit.       */

/* Back to pass 0 of seed stream `stream_id`, without a host round trip: rt_reset_async (pass number, counters, launch count;
 * the colour plane and packed pixels stay until the next launch overwrites them) plus a small kernel on `hip_stream` that writes
 * the stream into the context's seed buffer -- one thread and one 8-byte store per pixel, nothing crosses the bus (uploading the
 * same words would be 16.6 MB per 1080p frame).  The words are rt_stream_seeds(stream_id, ...); stream 0 is the default
 * stream and is read in place exactly as after rt_reset_async.  The tile order's costs are kept (the scene has not changed).
 * A host that animates a scene gives frame k stream k + 1 so that the noise does not stand still while the scene moves.
 * Sharded and multi-device contexts: every shard gets the same full-image stream (a multi-device context on its shards' own
 * streams; `hip_stream` is not used there).                                                                               */
RT_API int rt_seed_stream_async(rt_ctx *ctx, uint64_t stream_id, void *hip_stream);

/* Restore a render: `colors_host` (3 floats/px) and `seeds_host` (2 words/px) in exactly the layouts rt_read_colors and
 * rt_read_seeds return -- the full image, also for a sharded context, which goes on rendering its own rows; a multi-device
 * context hands them to every shard -- and the pass number the next launch continues from.  seeds_host == NULL means the
 * default stream; colors_host == NULL is allowed only with current_sample == 0 (pass 0 overwrites the plane, .cl:580-582).
 * Counters and the launch count restart as by rt_reset.  The packed pixels are NOT written: rt_read_pixels right after the
 * call packs the restored plane (same toInt, .cl:34,594-596) -- of a state beyond pass 0.  AT PASS 0 THE PACKED PIXELS ARE
 * UNSPECIFIED: pass 0 means that the plane holds nothing (rt_reset_async leaves an old frame there, rt_merge_async skips such a
 * context), so nothing is packed from it and rt_read_pixels returns whatever the buffer held before the call.  The same holds
 * for the tiles of a ragged context that hold no pass.  Blocking, like rt_reset; the buffers may be reused on return.
 * A refused call (RT_ERR_ARG: negative pass number, colours missing beyond pass 0) leaves the context as it was.             */
RT_API int rt_write_state(rt_ctx *ctx, const float *colors_host, const uint32_t *seeds_host, int current_sample);

/* The same through a checkpoint file, so that a long render can be stopped and resumed.  Format (little-endian, no padding):
 *     bytes 0-7    magic "RTSTATE\0"
 *     bytes 8-11   uint32 version = 1
 *     bytes 12-23  int32 w, int32 h, int32 current_sample
 *     then         float32[3 * w * h]   the colour plane, as rt_read_colors returns it
 *     then         uint32[2 * w * h]    the seed pairs, as rt_read_seeds returns them
 * rt_load_state reads and checks the whole file before it touches the context: a file that is short, has the wrong magic or
 * version, or holds another image size returns RT_ERR_ARG with the reason in rt_last_error, and the context is unchanged.
 * Scene, camera and mode are not part of the state.                                                                       */
RT_API int rt_save_state(rt_ctx *ctx, const char *path);
RT_API int rt_load_state(rt_ctx *ctx, const char *path);

/* Combine independent renders of one scene: afterwards `dst` holds the sample-weighted average of itself and the `n_srcs`
 * sources.  Per float of the colour plane, in binary32 without contraction, over X = dst, srcs[0], srcs[1], ... with
 * n_X = rt_current_sample(X) > 0:   acc = c_X * (float)n_X  for the first such X,  acc = acc + c_X * (float)n_X  for the others,
 * out = acc * (1.0f / (float)N),  N = sum of n_X  -- the multiply by a reciprocal is the reference's own idiom for its running
 * average (.cl:580-590).  A context at pass 0 is skipped, not weighted by zero: after rt_reset_async its plane still holds an
 * old frame.  dst's pass number becomes N, its seeds and counters stay, and rt_read_pixels packs the merged plane; the sources
 * are only read.  One bandwidth-bound kernel on `hip_stream`, ordered behind everything dst and the sources have queued, and
 * their later work behind it.  The sources should have rendered on seed streams of their own (rt_seed_stream_async):
 * contexts on one stream render the same frame, and merging them gains nothing.
 * RT_ERR_ARG: n_srcs outside 1 .. 15, a null entry, dst among the sources, a source listed twice, contexts that differ in
 * size or sharding (w, h, rank, nranks, tile_rows) or device, any multi-device context.  RT_ERR_STATE: N == 0.
 * A refused call changes nothing.
 * With a RAGGED context among them (adaptive sampling, below) a second kernel does the same arithmetic with n_X = the pass count X holds
 * FOR THE TILE THE FLOAT'S PIXEL LIES IN: a context whose tile holds no pass is skipped for that tile, a tile nobody holds a pass of keeps
 * dst's floats.  dst's tile counts become the per-tile sums, its pass number the sum of the pass numbers as always, and dst is ragged.
 * With whole contexts only, nothing has changed: the same kernel, the same bits.                                                      */
RT_API int rt_merge_async(rt_ctx *dst, rt_ctx *const *srcs, int n_srcs, void *hip_stream);

/* ---- frame error on the device: compare two frames, map the error, render to a PSNR ------------
 * How far apart the packed frames of two contexts are, computed where the frames live: one bandwidth-bound kernel reads both
 * pixel buffers once (8 B per pixel) and leaves 48 bytes, instead of two read-backs (8.3 MB each at 1080p) and a host loop.
 * THIS LIBRARY'S OWN EXTENSION: the reference renders one frame on one seed stream and compares nothing; these calls reproduce
 * no reference frame.  Their use: two contexts that render the same scene on seed streams of their own (rt_seed_stream_async) are
 * independent estimates of one image, and the difference between two N-pass estimates measures the noise of an N-pass render.
 *
 * The metric is exact integer arithmetic on the packed words (R | G<<8 | B<<16): with p from a and q from b, for channel c
 * d_c = ((p >> 8c) & 255) - ((q >> 8c) & 255); bits 24-31 are ignored everywhere.                                            */
typedef struct {              /* 48 bytes, no padding */
    uint64_t sq_err[3];       /* per channel R, G, B: sum over the compared pixels of d_c^2                                    */
    uint64_t differing;       /* pixels whose low 24 bits differ                                                               */
    uint64_t pixels;          /* pixels compared = rt_local_rows * w                                                           */
    uint32_t max_abs;         /* largest |d_c| of any channel of any pixel                                                     */
    uint32_t reserved;        /* 0                                                                                             */
} rt_frame_error;

/* The tile map that goes with it: one uint32 per 8x8 tile of the LOCAL pixel buffer (the render kernels' tile; edge tiles are
 * partial), tiles[ty * tiles_x + tx] = sum of d_0^2 + d_1^2 + d_2^2 over the tile (at most 64 * 3 * 255^2 = 12 484 800), with
 * tiles_x = ceil(w / 8), tiles_y = ceil(rt_local_rows / 8).  rt_compare_tiles stores the two (either pointer may be NULL) and
 * returns tiles_x * tiles_y, the number of words a map holds (0 for a sharded context without rows), or RT_ERR_ARG.           */
RT_API int rt_compare_tiles(const rt_ctx *ctx, int *tiles_x, int *tiles_y);

/* Compare the frames of `a` and `b` on `hip_stream`, without a host wait.  `result_dev` is a caller-owned DEVICE address of one
 * rt_frame_error (required); `tiles_dev` a DEVICE address of rt_compare_tiles() words, or NULL for no map.  The call is ordered
 * behind everything both contexts have queued, on whatever streams, and their later work behind it (as rt_merge_async); it clears
 * the result on the stream itself, so that two calls in a row give the same answer.  What is compared are the buffers the
 * contexts' launches write -- the rt_set_pixel_buffer target if one is set, else the context's own -- each first brought up to
 * date exactly as by rt_read_pixels_async (the pack kernel, if the last launches ran with the pixel store off).  Modes and pass
 * numbers may differ between a and b (fast against parity is the 50 dB gate).  Nothing else of either context changes: colours,
 * seeds, pass number, counters, tile-order costs and rt_last_kernel stay.  Sharded contexts compare their local rows (a context
 * without rows yields zeros and launches nothing); the sums are integers, so the ranks' results add up exactly (max_abs by maximum).
 * RT_ERR_ARG, and nothing changes: a null context or result, a == b, contexts that differ in size or sharding (w, h, rank,
 * nranks, tile_rows) or device, any multi-device context.                                                                    */
RT_API int rt_compare_async(rt_ctx *a, rt_ctx *b, rt_frame_error *result_dev, uint32_t *tiles_dev, void *hip_stream);

/* The same, blocking, into HOST memory (`tiles_host` may be NULL): on a's own stream through scratch that `a` owns (allocated on
 * first use, freed by rt_destroy), then the 48 bytes -- and the map, if asked for -- are waited for.                           */
RT_API int rt_compare(rt_ctx *a, rt_ctx *b, rt_frame_error *out_host, uint32_t *tiles_host);

/* 10 * log10(255^2 * 3 * pixels / (sq_err[0] + sq_err[1] + sq_err[2])) in binary64: the PSNR over the packed 8-bit channels that
 * every quality figure of this project is (tools/fast_gate.py, tools/convergence.py).  +infinity when the sum is 0.  Needs no
 * device.  (NaN, with rt_last_error set, for a null pointer.)                                                                  */
RT_API double rt_error_psnr(const rt_frame_error *e);

/* Render two contexts in step until the frames agree: repeat { n = min(passes_per_check, max_passes - rt_current_sample) passes
 * on each context, asynchronously, each on its own rt_stream; rt_compare; wait for the 48 bytes } and return 1 after the first
 * check whose rt_error_psnr >= target_psnr_db, 0 when max_passes is reached first, a negative rt_status on error.  *last (host,
 * required) is the last check, *checks (may be NULL) their number; if no pass could be rendered (max_passes equals the pass
 * number) it is one check of the frames as they are.  The call sets no seed streams and merges nothing: the caller gives each
 * context a stream before (rt_seed_stream_async) and combines them after (rt_merge_async).
 * THE FIGURE IS THE PSNR BETWEEN THE TWO HALVES, each an N-pass render.  The merged 2N-pass frame is closer to the converged
 * image than the halves are to each other: with independent errors of equal variance the difference of the halves carries twice
 * the variance of one half and four times that of their mean, about 6 dB in the linear colour plane.  How much of that survives
 * the clamp, the gamma and the rounding to 8 bits has NOT been measured yet (tools/frame_error_probe.py records it): until it
 * is, treat the pair figure as a lower bound of the merged frame's quality and add nothing to it.  (For the FILTERED merge the offset is
 * about 13 dB, and "the error of the filtered frame" below has a figure of its own for it: rt_render_converged_filtered.)
 * RT_ERR_ARG: a pair rt_compare refuses, a null `last`, passes_per_check < 1, max_passes below the contexts' pass number, a NaN
 * target.  RT_ERR_STATE: contexts at different pass numbers; both at pass 0 of the default seed stream (they would render the
 * same frame and "converge" at once).  A refused call changes nothing.                                                       */
RT_API int rt_render_converged(rt_ctx *a, rt_ctx *b, double target_psnr_db, int passes_per_check, int max_passes,
                               rt_frame_error *last, int *checks);

/* ---- adaptive sampling: render only the 8x8 tiles that are still noisy ----------------------------
 * rt_render_converged adds whole frames until the frame as a whole has converged; one noisy corner keeps every sky tile rendering.  The
 * calls below render SUBSETS of the tiles, chosen on the device from rt_compare_async's tile map.  THIS LIBRARY'S OWN EXTENSION, like the
 * state and compare calls.  The render kernels are the same: they take their tile from a list, and a subset launch is a shorter list and a
 * smaller grid.
 * WHAT MAKES IT EXACT: pixels are independent, so a tile that has received p passes holds the colours, seeds and packed pixels of a uniform
 * p-pass render of its seed stream, bit for bit, whatever happened to the other tiles.  rt_get_stats stays exact too (the kernels count
 * valid lanes only): samples = sum over the pixels of the pixel's pass count.
 * THE GROUP RULE: what is selected and rendered is a GROUP -- the 8x8 tiles 4g .. 4g+3 of one tile row: 32x8 pixels aligned at multiples
 * of 32 in x (fewer tiles and pixels at the right and top edges), the tile of the widest shipped workgroup.  A group is rendered whole or
 * not at all, so its tiles hold one pass count, and both the one-wavefront (8x8) and the four-wavefront (32x8) instances can render it.
 * THE FRONT RULE: a launch has ONE first pass number, so only groups whose pass count equals rt_current_sample -- the FRONT -- can be
 * selected.  A group that was left out of a subset launch has fallen behind and stays retired until the context is whole again.  The
 * device enforces this (rt_select_tiles reads the counts), not the caller.
 * A context is RAGGED while some tile holds fewer passes than rt_current_sample.  rt_reset, rt_reset_async, rt_seed_stream_async,
 * rt_write_state and rt_load_state make it whole again (and drop the selection).  ON A RAGGED CONTEXT these return RT_ERR_STATE and change
 * nothing: rt_render_pass, rt_render_async, rt_render_converged, rt_render_adaptive (a full-frame launch would continue the retired tiles
 * from the wrong pass number) and rt_save_state (file format 1 holds one pass number).  rt_read_colors, rt_read_seeds, rt_read_pixels(_async),
 * rt_compare*, rt_get_stats and rt_set_pixel_write with the pack kernel work as on any context; rt_merge_async weights each tile by its own
 * count (below).  Multi-device contexts and sharded contexts (nranks > 1) are refused by every call of this section with RT_ERR_ARG.
 * NOT TIMED ON AN MI355X YET: a subset launch pays the LDS staging per workgroup like any other launch, each rt_select_tiles waits for
 * 8 bytes, and the list is built once per selection; tools/adaptive_probe.py records what that costs against what it saves
 * (profiles/r11_adaptive.jsonl).  No speed-up is promised.                                                                            */

/* The pass count of every 8x8 tile: rt_compare_tiles() words in that call's indexing, into HOST memory.  Blocking.  For a context that
 * is not ragged every word equals rt_current_sample (nothing is stored on the device until a subset launch leaves tiles behind).      */
RT_API int rt_tile_passes(rt_ctx *ctx, uint32_t *out_host);

/* Select the groups the next rt_render_tiles_async renders.  A group is selected when it is at the front AND (err_dev is NULL, OR some
 * tile t of it has  err_dev[t] * 64 > above * pixels(t)),  pixels(t) = the image pixels inside tile t: 64 for a full tile -- the rule is
 * then err > above -- fewer at the right and top edges.  `err_dev` is a DEVICE array of rt_compare_tiles() words in that layout:
 * rt_compare_async's map, or anything else.  One small kernel on `hip_stream`, ordered behind the context's work, writes one flag per
 * group into the context; the call then WAITS for 8 bytes: counts[0] = selected groups, counts[1] = the 8x8 tiles they cover (`counts`
 * may be NULL; the context keeps both).  A new selection replaces the old one; a reset or a merge into the context drops it.
 * RT_ERR_ARG: a null, multi-device or sharded context.                                                                               */
RT_API int rt_select_tiles(rt_ctx *ctx, const uint32_t *err_dev, uint32_t above, void *hip_stream, uint32_t counts[2]);

/* n_samples passes on the selected groups and on nothing else, asynchronously on `hip_stream`.  RT_OK and nothing done when the
 * selection is empty or n_samples == 0.  The launch uses the kernel form the context's last launch used (before any launch: what the
 * thresholds say for the scene); it starts, advances and times none of the measurements rt_scene_choice reports, and it reads the
 * heavy-first tile order without touching it or the tile costs.  A small kernel builds the launch's tile list from the selection -- the
 * selected groups' tiles in heavy-first order where one exists, else in image order -- once per selection, order and tile shape; another
 * adds n_samples to the pass count of every tile of every selected group.  Afterwards rt_current_sample has grown by n_samples, the
 * launch count by one, rt_last_kernel names the instance, and the context is ragged unless the selection held every group of the image.
 * A launch from pass 0 that leaves groups out leaves them as a 0-pass render holds them: the seeds of the context's stream and a colour
 * plane of zeros (one fill of the plane ahead of the launch), whatever frame rt_reset_async had left there; their packed pixels stay unspecified.
 * RT_ERR_STATE: no selection; no scene or camera; a kernel instance whose tile is wider than a group (the diagnostics library's
 * two-pixels-per-lane rows).  RT_ERR_ARG: n_samples < 0 or a pass counter overflow; a null, multi-device or sharded context.            */
RT_API int rt_render_tiles_async(rt_ctx *ctx, int n_samples, void *hip_stream);

/* rt_render_converged per tile.  Preconditions and refusals are that call's; besides, min_passes >= 0 (RT_ERR_ARG) and neither context
 * may be ragged on entry (RT_ERR_STATE).
 *   1. while the pass number is below min(min_passes, max_passes): the shortfall as ordinary full launches on both contexts;
 *   2. repeat { rt_compare with the tile map (a's scratch); rt_select_tiles on BOTH contexts from that one map with
 *      above = floor(255^2 * 192 / 10^(tile_psnr_db / 10)) -- the tile's squared error at which the PSNR over its 192 channel values
 *      equals the target; the same map gives the same selection, so the two contexts stay in step tile for tile;
 *      no group selected: return 1;  pass number == max_passes: return 0;
 *      rt_render_tiles_async of min(passes_per_check, max_passes - passes) on each context, each on its own rt_stream }.
 * *last (host, required) is the last WHOLE-FRAME comparison, *checks (may be NULL) their number.  A negative rt_status on error.
 * The call merges nothing: rt_merge_async(a, &b, 1, ...) afterwards is exact per tile, and rt_tile_passes gives the sample map.
 * Everything said above rt_render_converged about the pair figure holds PER TILE: a tile's figure is the PSNR between the two halves, a
 * lower bound of the merged tile's quality by an offset that has not been measured.  Besides, a tile's figure at few passes is itself
 * NOISY -- it is a sum over 64 pixels, not over a frame -- so a tile can retire by chance with both halves wrong in the same direction or
 * simply close; retired is final.  min_passes is the guard against that: no tile is judged before it holds that many passes.          */
RT_API int rt_render_adaptive(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes,
                              rt_frame_error *last, int *checks);

/* ---- denoising: a non-local-means filter steered by the difference of two halves ------------------
 * The last step of the pipeline above: two contexts render one scene on seed streams of their own, are compared, rendered until they agree
 * and merged -- and the merged frame still carries the residual noise.  The two halves are the standard input of a filter for it: their
 * difference is a per-pixel estimate of the variance, and a non-local-means filter whose weights are steered by that estimate is what
 * Rousselle, Knaus and Zwicker pair with adaptive sampling (2012).  THIS LIBRARY'S OWN EXTENSION: the reference filters nothing,
 * and these calls reproduce no reference frame.  A FILTERED FRAME IS BIASED: it is no longer the average of its passes, and rendering on
 * from it (rt_render_async on dst afterwards) continues a biased average.  Filter the frame you show, not the state you keep.
 *
 * THE ARITHMETIC, the same in rt_denoise_async's kernel and in rt_denoise_planes, all binary32, uncontracted, in this order, IEEE division.
 * Planes are [h][w][3] floats as rt_read_colors returns them; cl(y, x) clamps both coordinates to the image; D is the image, A and B the
 * halves; R = search_radius, P = patch_radius, kk = k * k, inv = 1.0f / (float)(3 * (2P + 1) * (2P + 1)).
 *   1. V[y][x][c] = d * d with d = (A - B) * 0.5f                    (the variance of the mean of two equal halves)
 *   2. Vs[y][x][c] = (sum of V[cl(y + j, x + i)][c], j = -1..1 outer, i = -1..1 inner, from its first term) * (1.0f / 9.0f)
 *   3. for an offset o = (oy, ox), a pixel p inside the image and q' = cl(p + o), per channel: t = D[p][c] - D[q'][c],
 *      m = Vs[q'][c] < Vs[p][c] ? Vs[q'][c] : Vs[p][c],
 *      dc = (t * t - alpha * (Vs[p][c] + m)) / (1e-10f + kk * (Vs[p][c] + Vs[q'][c]));     e(p, o) = (d0 + d1) + d2
 *   4. S(p, o) = sum of e(cl(p + delta), o), dy = -P..P outer, dx inner, from its first term;  T = S * inv.  e is taken at the clamped
 *      position AND THAT POSITION'S OWN clamped partner -- not at cl(p + delta + o); the two differ at the border
 *   5. offsets run oy = -R..R outer, ox inner.  o = (0, 0): wgt = 1.0f.  p + o outside the image: skipped.  T a NaN, or any of the three
 *      D[p + o][c] not finite: skipped.  Otherwise g = T > 0 ? T : 0 and wgt = 1.0f / (1.0f + g * (1.0f + g * 0.5f))
 *   6. num[c] and den start at 0.0f; every offset that is not skipped adds wgt * D[p + o][c] and wgt, in offset order;
 *      out[p][c] = num[c] / den.  den >= 1.  A non-finite pixel stays non-finite and spreads to no neighbour.
 * With R = 0 the output is the image, bit for bit.
 * MEASURED, in numpy on a CPU, with frames of this project's oracle (the arithmetic above before any kernel existed): the Demo scene at 96x64,
 * halves on seed streams 1 and 2, against a 4096-pass frame of the default stream (32 768 passes for the two larger N), PSNR over 8-bit
 * channels packed by numpy's clip, **(1 / 2.2), * 255 + 0.5:
 *     passes per half     pair      merged    filtered (R 5, P 1, alpha 1, k 0.45)
 *           4           14.8 dB      20.4        27.7
 *          16           20.9         26.5        31.6
 *          64           26.4         31.3        35.8
 *         256           31.3         36.3        40.3
 * R = 3 gives the same within 0.4 dB; k = 1.0 and P = 2 are 1 - 2.5 dB worse.  tools/denoise_probe.py measures the gain and the kernel's time
 * on the device (profiles/r12_denoise.jsonl); no time is promised.                                                                     */
typedef struct {              /* 16 bytes */
    int32_t search_radius;    /* R: the window is (2R + 1)^2 offsets; 0 .. 8                                                    */
    int32_t patch_radius;     /* P: patches of (2P + 1)^2 pixels; 0 .. 2                                                        */
    float alpha;              /* how much of the noise's own share is taken off a squared difference; finite, >= 0             */
    float k;                  /* the filter's strength: distances are measured in units of k^2 * variance; finite, > 0         */
} rt_denoise_params;

/* {5, 1, 1.0f, 0.45f}.  Needs no device.                                                                                       */
RT_API void rt_denoise_defaults(rt_denoise_params *p);

/* Filter dst's colour plane -- the image D -- steered by the colour planes of `a` and `b`, the two independent halves A and B, on
 * `hip_stream`, without a host wait.  The intended use: dst is a third context that holds their merge, rt_merge_async(dst, {a, b}, 2, s) with
 * dst at pass 0.  That also holds after rt_render_adaptive: the merge is then per tile, the variance estimate is per pixel.  `p` == NULL
 * means the defaults.  The call is ordered behind everything the three contexts have queued, on whatever streams, and their later work
 * behind it (as rt_merge_async).  Two kernels: the smoothed variance (rule 2) into a plane that dst owns, then the filter -- a workgroup per
 * 32x8 pixels, D and Vs of the tile and its halo of R + P staged in LDS, e(., o) formed once per offset for the tile and its P-halo and
 * shared by the patches that cover it -- into a SCRATCH PLANE THAT dst OWNS (both allocated on first use, freed by rt_destroy).  The
 * scratch plane then BECOMES the colour plane BY EXCHANGING THE TWO POINTERS; nothing is copied, and the old plane is the next call's scratch.
 * Afterwards dst's colour plane holds the filtered image and its packed pixels are stale: rt_read_pixels and rt_compare* pack the plane with
 * the same toInt as after a merge.  Nothing else of dst changes and nothing at all of a or b: pass number, seeds, counters, tile counts,
 * selection, tile order and rt_last_kernel stay.  search_radius == 0 launches nothing and leaves dst as it is.
 * Ragged contexts are accepted.  The arithmetic weights the halves equally, which is right when a and b hold equal counts tile for tile;
 * rt_render_adaptive leaves them that way and checks it.  THAT IS NOT CHECKED HERE.
 * RT_ERR_ARG: a null context; dst equal to a or b, or a == b; contexts that differ in size or device; any multi-device or sharded context
 * (the halo would cross shards); search_radius outside 0 .. 8, patch_radius outside 0 .. 2; alpha negative or not finite; k not finite
 * or <= 0.  RT_ERR_STATE: rt_current_sample(a) != rt_current_sample(b); either of them 0; rt_current_sample(dst) different from their sum
 * (dst is not their merge).  A refused call changes nothing.                                                                            */
RT_API int rt_denoise_async(rt_ctx *dst, rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream);

/* The same arithmetic on HOST planes of w x h pixels, as plain loops: the readable statement of the rules above, and what the device is
 * tested against bit for bit.  `out` may not overlap the inputs.  Needs no device.  RT_ERR_ARG: a null plane, w or h < 1, parameters
 * rt_denoise_async refuses.                                                                                                           */
RT_API int rt_denoise_planes(float *out, const float *merged, const float *a, const float *b, int w, int h, const rt_denoise_params *p);

/* ---- the error of the filtered frame: cross-filtered halves, render to ITS PSNR -------------------
 * The pipeline above judges one frame and shows another: rt_render_converged and rt_render_adaptive measure the PSNR between the UNFILTERED halves,
 * and the frame the user looks at is the filtered merge, for which nothing above has an error figure.  Rousselle, Knaus and Zwicker (2012)
 * close the gap with dual buffers: half A is filtered with weights taken from half B, and B with weights taken from A.  Each half's weights are then
 * independent of its own noise, and the difference of the two filtered halves estimates the error of the filtered result.  THIS LIBRARY'S OWN
 * EXTENSION; it reproduces no reference frame.  No call above changes behaviour.
 *
 * THE ARITHMETIC, the same in rt_denoise_pair_async's kernel and in rt_denoise_pair_planes: all binary32, uncontracted, in the written order, IEEE
 * division; the symbols are those of the denoising section.
 *   7. Vs comes from rules 1-2 unchanged.  Vh = Vs + Vs is the variance of ONE half: (A - B)^2 / 4 estimates the variance of the mean, which is half
 *      of one half's variance.
 *   8. For X in {A, B} with the guide G = the other half, FX follows rules 3-6 with three substitutions: in rule 3  t = G[p][c] - G[q'][c]  and every
 *      Vs is Vh;  rule 5's finiteness test reads X[p + o][c];  rule 6 accumulates wgt * X[p + o][c].  Everything else holds as written: the double
 *      clamp of rule 4, the offset order, the centre weight 1.0f, a NaN T skipped.
 *   9. With R = 0, FX = X bit for bit.  Exchanging a and b exchanges FA and FB bit for bit.  A non-finite value of X stays at its place in FX and
 *      spreads nowhere; a NaN in the guide removes only the offsets whose patches touch it.
 * MEASURED, in numpy on a CPU, with frames of this project's oracle alone (before any kernel existed): 96x64, the halves on seed streams 1 and 2 and
 * packed by the oracle's toInt, truth a 4096-pass frame of the default stream (2048 passes for the 16-sphere scene), the defaults; PSNR in dB:
 *     scene               passes per half   pair A/B (the loops above)   filtered merge vs truth (what is shown)   cross-filtered pair FA/FB
 *     Demo                      4                 14.78                          27.69                                    28.00
 *     Demo                     16                 20.90                          31.60                                    32.44
 *     Demo                     64                 26.41                          35.43                                    35.83
 *     c16_demo_plus_10          4                 15.00                          27.23                                    27.21
 *     c16_demo_plus_10         16                 20.82                          31.42                                    31.86
 * The cross-filtered pair figure lands within 0.9 dB of the true quality of the frame shown, where the raw pair is about 13 dB away: a host that
 * wants a 28 dB picture and stops on the raw pair renders about twenty times the passes it needs.  Summed squared error, Demo at 4 passes: 1.90 M
 * for the cross pair against a true 2.04 M and 39.8 M for the raw pair.  Per 8x8 tile, the rank correlation of the map with the filtered frame's
 * true tile error is 0.90 / 0.87 / 0.94 for the cross pair and 0.71 / 0.89 / 0.91 for the raw pair (Demo, 4 / 16 / 64 passes).
 * TWO THINGS THE SAME RUNS SHOWED:
 *   - The mean of FA and FB is about 1 dB WORSE than rt_denoise_async of the merge (27.09 against 27.69, 30.63 against 31.60).  The cross-filtered
 *     planes are an estimator, not the picture.  The picture stays rt_denoise_async's.
 *   - The estimate sees variance, not the filter's bias, because both halves blur the same edge.  It is up to 0.85 dB optimistic in the table and
 *     will be more so where bias dominates.  IT IS AN ESTIMATE, NOT A BOUND.
 * ON THE DEVICE: tools/filtered_error_probe.py records the pair kernel's time beside rt_denoise_async's and the table above from rendered contexts
 * (profiles/r14_filtered_error.jsonl); no time is promised.  The pair call does two filters' arithmetic on shared staging.                        */

/* Each half filtered with the other half's weights, on `hip_stream`, without a host wait.  FA goes into a float plane that `a` owns, FB into one
 * that `b` owns, laid out like the colour planes; beside each goes the plane packed by the library's toInt (.cl:34 -- the function the pack
 * kernel of that context's mode uses), one uint32 per pixel in the PIXEL BUFFER's layout (row 0 = bottom), which is what rt_compare_filtered
 * reads.  The four planes are allocated on first use and freed by rt_destroy.  `p` == NULL means rt_denoise_defaults.  Ordering, ragged contexts
 * and refusals are rt_denoise_async's: behind everything both contexts have queued, their later work behind it.  Two kernels: rule 2's variance
 * (into scratch that `a` owns), then ONE kernel that forms FA and FB together -- a workgroup per 32x8 pixels; A, B and Vh of the tile and its halo
 * of R + P in LDS; rule 3's alpha * (Vh[p] + m) and 1e-10f + kk * (Vh[p] + Vh[q']) formed once and shared by both directions.
 * Nothing else of either context changes: colour planes, seeds, pass numbers, packed pixels, counters, tile counts, selection, tile order and
 * rt_last_kernel stay.  search_radius == 0 copies the halves (and packs them).
 * A context's cross-filtered plane is CURRENT from this call until anything moves its colour plane: a launch, a reset, rt_seed_stream_async,
 * rt_write_state / rt_load_state, a merge or rt_denoise_async into it.
 * RT_ERR_ARG: a null context, a == b, contexts that differ in size or device, any multi-device or sharded context, parameters rt_denoise_async
 * refuses.  RT_ERR_STATE: pass numbers that differ, or zero.  A refused call changes nothing.                                                    */
RT_API int rt_denoise_pair_async(rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream);

/* rt_denoise_pair_async for the groups of the CURRENT SELECTION alone (adaptive sampling's groups of 32x8 pixels; rt_select_tiles): the float and the
 * packed cross-filtered planes of the selected groups are formed again from the two colour planes as they are now, by rules 7-9 and the same packing,
 * and every other pixel of the four planes keeps the words it held.  A pixel of a selected group receives exactly what rt_denoise_pair_async would
 * write there now -- rt_denoise_pair_planes of the two current colour planes at that pixel.  What the call is for: after rt_render_tiles_async only the
 * selected groups' colours have moved, and a group that was left out is never selected again (the front rule), so a check that only steers the next
 * selection need not filter it again.  A RETIRED GROUP'S FILTERED VALUES ARE THEN THOSE OF ITS LAST CHECK, formed with its neighbours' colours of that
 * time; they are not what rt_denoise_pair_async would write now.
 * Three kernels on `hip_stream`, ordered as rt_denoise_pair_async's: one workgroup that compacts a's selection flags into the list of selected groups
 * in ascending order (once per selection), rule 2's variance for the whole frame (it is bandwidth-bound and small beside the filter), and the pair
 * kernel's body with ONE WORKGROUP PER SELECTED GROUP, its origin taken from the list: the grid is the selection, not the frame.  search_radius == 0
 * copies and packs the halves of the selected groups.  `p` need not equal the parameters the planes were made with; a plane then holds both.
 * THE KERNEL READS a's SELECTION FLAGS.  That b's selection is the same set of groups is the caller's responsibility, as in rt_render_adaptive (one map
 * selects on both contexts); only the counts are compared.
 * Accepted when every precondition of rt_denoise_pair_async holds, both contexts hold a selection with equal counts, and both contexts' cross-filtered
 * planes are in the same one of two states:
 *   (a) current, and made by one pair call: there is nothing to refresh; RT_OK, nothing is launched and nothing changes;
 *   (b) ONE SELECTION BEHIND: they were current and made by one pair call (rt_denoise_pair_async or this one), and since then nothing has moved either
 *       colour plane but rt_render_tiles_async of the selection still in hand, once or several times.
 * Anything else leaves the planes stale for this call as for every other: a whole-frame launch, a reset, rt_seed_stream_async, a written or loaded
 * state, a merge or rt_denoise_async into the context, a new rt_select_tiles, planes never made, or the two contexts behind different pair calls.
 * Afterwards both planes are current under a new pair id that the two contexts share: rt_read_filtered and rt_compare_filtered* accept them.  Nothing
 * else of either context changes.
 * RT_ERR_ARG: as rt_denoise_pair_async.  RT_ERR_STATE: pass numbers that differ or are zero; no selection on either context; selections of different
 * counts; planes in neither state (a) nor (b).  A refused call changes nothing.
 * tools/live_check_probe.py times the call against rt_denoise_pair_async (profiles/r15_live_checks.jsonl); no time is promised.                      */
RT_API int rt_denoise_pair_tiles_async(rt_ctx *a, rt_ctx *b, const rt_denoise_params *p, void *hip_stream);

/* The same arithmetic on HOST planes of w x h pixels, as plain loops, FA into `out_a` and FB into `out_b`: what the device is tested against bit
 * for bit.  The outputs may not overlap the inputs or each other.  Needs no device.  Refusals are rt_denoise_planes'.                          */
RT_API int rt_denoise_pair_planes(float *out_a, float *out_b, const float *a, const float *b, int w, int h, const rt_denoise_params *p);

/* The context's cross-filtered plane, 3 floats per pixel as rt_read_colors lays them out, into HOST memory.  Blocking.  RT_ERR_STATE when the
 * plane is not current; RT_ERR_ARG for a null, multi-device or sharded context or a null buffer.                                               */
RT_API int rt_read_filtered(rt_ctx *ctx, float *out_host);

/* rt_compare_async / rt_compare over the two PACKED CROSS-FILTERED PLANES instead of the packed frames: the same kernel, the same exact integer
 * metric, the same tile map in rt_compare_tiles' indexing.  Nothing is packed or refreshed and nothing of either context changes.
 * RT_ERR_ARG as rt_compare, and for sharded contexts.  RT_ERR_STATE when either plane is not current or the two were not made by ONE
 * rt_denoise_pair_async call.                                                                                                                  */
RT_API int rt_compare_filtered_async(rt_ctx *a, rt_ctx *b, rt_frame_error *result_dev, uint32_t *tiles_dev, void *hip_stream);
RT_API int rt_compare_filtered(rt_ctx *a, rt_ctx *b, rt_frame_error *out_host, uint32_t *tiles_host);

/* rt_render_converged's loop and refusals with the check replaced: rt_denoise_pair_async(a, b, p) on a's stream, the comparison of the packed
 * cross-filtered planes, a wait for the 48 bytes.  The target is then the estimated PSNR of the FILTERED merge.  The call merges and filters
 * nothing: the caller goes on with rt_merge_async and rt_denoise_async, USING THE SAME PARAMETERS.  Besides that call's refusals, RT_ERR_ARG for
 * sharded contexts and for parameters rt_denoise_async refuses; a check at pass 0 (max_passes == 0) is RT_ERR_STATE.                            */
RT_API int rt_render_converged_filtered(rt_ctx *a, rt_ctx *b, double target_psnr_db, int passes_per_check, int max_passes,
                                        const rt_denoise_params *p, rt_frame_error *last, int *checks);

/* rt_render_adaptive with the tile map taken from the cross-filtered pair: the group rule, the front rule and `above` are unchanged, and one map
 * selects on both contexts, so they stay in step tile for tile.  A tile then retires when the FILTERED tile is estimated to have reached
 * tile_psnr_db; what is said above about a tile's figure being noisy, and about min_passes, holds as it stands.                               */
RT_API int rt_render_adaptive_filtered(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes,
                                       const rt_denoise_params *p, rt_frame_error *last, int *checks);

/* rt_render_adaptive_filtered with checks that filter only what is still rendering: the first check is the whole-frame rt_denoise_pair_async, every
 * later one rt_denoise_pair_tiles_async of the selection that was just rendered; each is followed by the unchanged comparison of the whole packed planes
 * and rt_select_tiles on both contexts.  Arguments and refusals are rt_render_adaptive_filtered's.
 * THE SAME RENDER: the return value, *checks, rt_tile_passes, the colour planes, seeds and packed pixels of both contexts and rt_get_stats equal
 * rt_render_adaptive_filtered's with the same arguments, bit for bit -- a live group's filtered values depend on the current colour planes alone, and a
 * retired group's entry of the map is never read again.
 * WHAT DIFFERS: *last, and the retired groups' part of the cross-filtered planes.  Both hold, for every group, the figures of THAT GROUP'S LAST CHECK: a
 * retired group's filtered values were formed with its neighbours' colours of that time, and *last sums them as they stand.  As before, the figure is an
 * estimate, not a bound.  The planes are current on return, as after rt_render_adaptive_filtered.                                                  */
RT_API int rt_render_adaptive_filtered_tiles(rt_ctx *a, rt_ctx *b, double tile_psnr_db, int min_passes, int passes_per_check, int max_passes,
                                             const rt_denoise_params *p, rt_frame_error *last, int *checks);

/* ---- feature planes from camera rays, and NL-means guided by them -----------------------------------
 * Every filter above sees colour only.  At 4 to 16 passes per half the variance estimate of two halves is itself noisy, and colour-only NL-means then
 * blurs across object and wall boundaries.  Rousselle, Manzi and Zwicker (2013) add noise-free geometry features -- albedo, normal, depth --
 * that can only RESTRICT a weight.  THIS LIBRARY'S OWN EXTENSION: it reproduces no reference frame and touches no render kernel, and no call above
 * changes behaviour while no guide is set.  The planes are useful on their own: what lies under every pixel.
 *
 * THE FEATURE PLANE is F[h][w][8], 32 bytes per pixel, in the colour plane's row order (row h - 1 - y for image row y, .cl:579): words 0-2 the albedo,
 * 3-5 the normal, 6 the distance, 7 the bits of the scene index as uint32.  Rules 10-12 are binary32, uncontracted, IEEE division and square root, in
 * the written order -- ALWAYS parity's arithmetic, whatever rt_set_mode says.
 *  10. the ray: GenerateCameraRay (.cl:494-549) with both random numbers 0.5, r1 = r2 = 0.0f: kcx = ((float)x + 0.0f) * (1.f / w) - 0.5f, kcy alike;
 *      rdir = (cam.x * kcx + cam.y * kcy) + cam.dir per component; o = 0.1f * rdir + cam.orig; d = rdir * (1.f / sqrt(rdir . rdir)).
 *  11. the hit: Intersect (.cl:215-232) over every record in scene order with SphereIntersect (.cl:173-201): t = 1e20f; a record replaces it when
 *      dist != 0.f && dist < t, so equal distances keep the lowest index.  A hit is t < 1e20f.
 *  12. the values.  On a hit P = o + d * t, n = vnorm(P - p_id) (.cl:346-347, NOT turned towards the ray), albedo = c_id + e_id per channel,
 *      word 6 = t, word 7 = id.  On a miss seven 0.0f and 0xFFFFFFFF.  Non-finite records behave as in the reference: a NaN discriminant never
 *      hits; a zero-radius hit gives a NaN normal, which is stored as it is.
 * WHAT IT COSTS.  One lane per pixel over 8x8 tiles, by one of two kernels that give the same words (rt_last_features_kernel says which ran):
 *   SWEPT -- scenes without a hierarchy (fewer than 56 small, finite spheres that repeat no earlier record): pixels x records tests, the geometry
 *   table staged in LDS in chunks of 1024 records with a barrier between chunks, so any count up to RT_MAX_SPHERES works; the reference's Intersect
 *   by construction.
 *   WALKED -- every scene that has a hierarchy, from 56 records on (the count was measured: walked, the plane was the faster one at every probed
 *   count that has a hierarchy): the few large records (the hierarchy's always-list) swept, then ONE closest-hit query per pixel through the hierarchy
 *   the render kernels walk, with their tie rule (lowest scene index among equal distances) and their three table placements: tables in LDS
 *   (rt_features_pairs), pairs in LDS and slots in HBM / L2 (_pairs_m), everything in HBM / L2 (_pairs_g).  The hierarchy only selects candidates;
 *   every test that is made is rule 11's arithmetic.  An interactive host forms the plane every frame (rt_set_camera and rt_update_spheres_async end
 *   it): walked, the plane cost less than ONE pass of the same scene at every count measured, where the sweep cost 6 passes at 8192 records and 39
 *   at 262 144.  Measured, profiles/r35_features_walk.jsonl (tools/features_probe.py: both curves and the count); no time is promised.
 *
 * THE GUIDE.  Rules 13-14 extend rules 1-9; the symbols are those of the denoising sections.
 *  13. the feature distance of a pixel p and q = p + o inside the image.  ia = 1.0f / (k_albedo * k_albedo), in and id alike.
 *      PHIa = ((a0 * a0 + a1 * a1) + a2 * a2) * ia with a_c = F[p][c] - F[q][c];  PHIn the same over words 3-5, times in;
 *      r = (t_p - t_q) / ((t_p + t_q) + 1e-10f), PHId = (r * r) * id.  PHI = 0.0f; then for PHIa, PHIn, PHId in that order: if (term > PHI) PHI = term
 *      (a NaN term constrains nothing).  wf = 1.0f / (1.0f + PHI * (1.0f + PHI * 0.5f)).
 *  14. in rule 5, for an offset other than (0, 0) that is not skipped, wgt = wf < wgt ? wf : wgt.  Nothing else of rules 1-9 changes: the skips, the
 *      centre weight, the offset order, the double clamp.  In the pair filter one wf, formed once, serves both directions.
 * So: with R = 0 the output is the input; with every k = 1e18f and finite features, or with a constant feature plane, wf is exactly 1 and the guided
 * result equals the unguided one bit for bit.
 * MEASURED, in numpy on a CPU before any kernel existed (the prototype), with frames of this project's oracle alone: halves on seed streams 1 and 2,
 * truth 2048 passes of the default stream, PSNR over 8-bit channels packed by clip ** (1 / 2.2) * 255 + .5, the filter's defaults, the guide's
 * defaults {0.15, 0.2, 0.05}; "k 0.6" is the same guide with the filter's k raised to 0.6.  96x64, dB:
 *     scene           passes per half    merged    NL-means unguided    guided    guided, k 0.6
 *     Demo                  4            20.41         27.62            27.83        27.97
 *     Demo                 16            26.43         31.46            31.57        31.30
 *     cornell.scn           4            17.14         25.05            25.67        26.01
 *     cornell.scn          16            21.16         28.50            29.11        29.22
 *     simple.scn            4            24.83         29.67            30.94        30.73
 *     simple.scn           16            31.69         34.18            34.90        34.20
 * AND BY rt_denoise_guided_planes ITSELF (tests/test_guided_cpu.py asserts half of each gain): the scenes of tests/golden at 96x96, 4 passes per half,
 * truth 1024 oracle passes, the same pack, dB:
 *     scene                          unguided    guided     gain      (the prototype's gain at 96x64)
 *     cornell (18 records)            24.76       25.30     +0.54           +0.6
 *     simple (10 records)             29.04       30.29     +1.24           +1.3
 *     Demo                            27.56       28.15     +0.59           +0.2
 * The gain is largest on scenes of diffuse surfaces and smallest on the Demo scene, which is mostly glass.
 * ON THE DEVICE: a guided workgroup stages words 0-6 of its tile and an R-halo beside the colour planes, 28 (32 + 2R)(8 + 2R) bytes more LDS -- about
 * 58 KiB for the pair kernel at the defaults, 92 KiB at R 8, P 2 (the dynamic-LDS limit is raised for it).
 * MEASURED on an MI355X by tools/guided_probe.py (profiles/r21_guided.jsonl; device time between two events, medians; NO TIME IS PROMISED):
 *   rt_features_async, 800x600 / 1920x1080, beside ONE pass of the same scene:  Demo 0.010 / 0.022 ms (a pass 0.042 / 0.10);  1024 spheres 0.26 / 0.92
 *   (0.22 / 0.58);  8192 spheres 1.96 / 6.04 (0.42 / 1.02);  262 144 spheres 60 / 193 (2.0 / 4.9).  That was the plain sweep, then the only kernel:
 *   one pass at a thousand records and forty at RT_MAX_SPHERES.  Scenes with a hierarchy are walked since (WHAT IT COSTS, above).
 *   the filters at 1920x1080, unguided / guided:  rt_denoise_async 0.94 / 1.42 ms;  rt_denoise_pair_async 1.58 / 2.79;  rt_denoise_pair_tiles_async with
 *   half of the groups selected 0.85 / 1.45.  The unguided kernels are the machine code they were before the guide existed.
 *   the table above from rendered contexts, filtered on the device: unguided / guided 27.62 / 27.83 and 31.46 / 31.57 (Demo, 4 and 16 passes),
 *   25.05 / 25.67 and 28.50 / 29.11 (cornell), 29.67 / 30.94 and 34.18 / 34.90 (simple): the prototype's figures to the last digit.              */
typedef struct { float k_albedo, k_normal, k_depth; uint32_t reserved; } rt_guide_params;   /* 16 bytes; each k finite and > 0, reserved 0 */

/* {0.15f, 0.2f, 0.05f, 0}.  Needs no device.                                                                                   */
RT_API void rt_guide_defaults(rt_guide_params *g);

/* Form the feature plane of ctx's scene and camera on `hip_stream`, without a host wait, into plane memory that ctx owns (allocated on first use, freed
 * by rt_destroy).  Ordered behind everything the context has queued: a table rebuild that rt_update_spheres_async left pending runs first.
 * The plane is CURRENT from this call until rt_set_scene, rt_update_spheres_async or rt_set_camera on the context -- whatever they set.  Launches,
 * resets, merges and filters do not touch it: it depends on scene and camera alone.  Nothing else of the context changes.
 * RT_ERR_STATE without scene or camera; RT_ERR_ARG for a null, multi-device or sharded context.                                               */
RT_API int rt_features_async(rt_ctx *ctx, void *hip_stream);

/* The symbol of the kernel the context's last rt_features_async launched: "rt_features_kernel" (swept), "rt_features_pairs", "rt_features_pairs_m" or
 * "rt_features_pairs_g" (walked, by table placement).  "" before any such call and for a null context.  Like rt_last_kernel for the render path, the
 * only way to see the choice: it depends on the scene, never the result.                                                                         */
RT_API const char *rt_last_features_kernel(const rt_ctx *ctx);

/* The context's feature plane, 8 words per pixel, into HOST memory.  Blocking.  RT_ERR_STATE when the plane is not current; RT_ERR_ARG for a null,
 * multi-device or sharded context or a null buffer.                                                                                            */
RT_API int rt_read_features(rt_ctx *ctx, float *out_host);

/* Rules 10-12 as plain host loops over `count` records: what the device is tested against bit for bit.  Needs no device.  RT_ERR_ARG: a null
 * argument (spheres may be null when count is 0), w or h < 1.                                                                                 */
RT_API int rt_features_planes(float *out, const rt_sphere *spheres, uint32_t count, const rt_camera *cam, int w, int h);

/* The guide, a per-context setting like rt_set_mode.  NULL = off, the default.  While it is off on both halves every filter call and loop above is
 * what it was, bit for bit.  Six calls consult it: rt_denoise_async, rt_denoise_pair_async, rt_denoise_pair_tiles_async, rt_render_converged_filtered,
 * rt_render_adaptive_filtered and rt_render_adaptive_filtered_tiles.  The setting of the two HALVES a and b counts (dst's is ignored): both off, or
 * both on with the same 16 bytes -- otherwise RT_ERR_STATE.  When on, the feature plane is READ FROM a, and the planes of a and b must both be current
 * (RT_ERR_STATE otherwise); that they describe one scene and camera is the caller's responsibility, as the selections are in
 * rt_denoise_pair_tiles_async.  Exchanging a and b keeps exchanging FA and FB.  A refused call changes nothing.  As with differing rt_denoise_params,
 * changing the guide does not by itself make cross-filtered planes stale.
 * RT_ERR_ARG: a null, multi-device or sharded context; a k that is not finite or <= 0; reserved != 0.                                            */
RT_API int rt_set_denoise_guide(rt_ctx *ctx, const rt_guide_params *g);

/* rt_denoise_planes and rt_denoise_pair_planes under a guide: `feat` is a feature plane of w x h pixels, 8 words each.  With g == NULL they ARE those
 * functions (feat is not read).  Need no device.  Refusals are theirs, and a null feat or parameters rt_set_denoise_guide refuses.              */
RT_API int rt_denoise_guided_planes(float *out, const float *merged, const float *a, const float *b, const float *feat, int w, int h,
                                    const rt_denoise_params *p, const rt_guide_params *g);
RT_API int rt_denoise_pair_guided_planes(float *out_a, float *out_b, const float *a, const float *b, const float *feat, int w, int h,
                                         const rt_denoise_params *p, const rt_guide_params *g);

/* ---- temporal reprojection: carry a frame's samples to a moved camera ---------------------------------
 * An interactive host throws every sample away each time something moves: rt_set_camera or rt_update_spheres_async is followed by a reset, and the
 * new view starts at pass 0 with one-pass noise.  This section reprojects the previous view's accumulated colour into the new view through the
 * first-hit geometry of the feature planes and blends it with the new view's few passes.  Spheres make it clean: a translation describes a sphere's
 * motion completely, and the scene index identifies the surface.  THIS LIBRARY'S OWN EXTENSION: it reproduces no reference frame and touches no render
 * kernel, and no call above changes behaviour.
 *
 * THE TEMPORAL PLANE is T[h][w][4] floats in the colour plane's row order, owned by dst: rgb and n, the effective sample count behind the pixel.
 * Beside it goes the plane packed by the toInt of dst's mode (as rt_denoise_pair_async packs its planes), one uint32 per pixel in the PIXEL BUFFER's
 * layout (row 0 = bottom).  Both are allocated on first use and freed by rt_destroy.  T is a frame to show and a history to reproject from, NEVER a
 * state to render on from: dst's colour plane, seeds, pass number, counters, selection, tile order and rt_last_kernel stay, and nothing of src changes.
 *
 * THE ARITHMETIC, the same in rt_reproject_async's kernel and in rt_reproject_planes: all binary32, uncontracted, in the written order, IEEE division
 * and square root -- ALWAYS parity's arithmetic, whatever rt_set_mode says.  dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2.  D = dst, S = src; F is a
 * feature plane, C a colour plane, p the centres of the records.
 *  15. the point and where it was.  Image pixel (x, y) of D: id = word 7 of FD, t = word 6.  id == 0xFFFFFFFF (or any id that is no record's: the
 *      feature calls write none): NO HISTORY.  Otherwise (o, d) by rule 10 with D's camera, P = o + d * t per component, m = pD[id] - pS[id],
 *      Pp = P - m.
 *  16. where S saw it.  v = Pp - camS.orig; z = dot(v, camS.dir); !(z > 0.0f): no history.
 *      kx = (dot(v, camS.x) * dot(camS.dir, camS.dir)) / (z * dot(camS.x, camS.x)), ky the same with camS.y;
 *      fx = (kx + 0.5f) * (float)w, fy = (ky + 0.5f) * (float)h;  !(fx >= -1.0f && fx < (float)w && fy >= -1.0f && fy < (float)h): no history.
 *      x0 = floorf(fx), ax = fx - x0; y0 and ay alike.  This inverts rule 10 for the orthogonal basis rt_compute_camera makes; for any other basis it
 *      is still what both sides compute.
 *  17. the taps: the four pixels (x0 + i, y0 + j) of S, j = 0, 1 outer and i = 0, 1 inner, weight b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay).
 *      A tap q COUNTS only when it lies inside the image; word 7 of FS[q] equals id; with (oq, dq) by rule 10 with S's camera at q and tq = word 6 of
 *      FS[q]: Pq = oq + dq * tq, e = Pq - Pp, r = k_pos * (tq * (sqrtf(dot(camS.x, camS.x)) * (1.f / (float)w))) and dot(e, e) <= r * r -- S saw the same
 *      place within k_pos pixel footprints, which rejects the far side of the same sphere (other surfaces fail on id); and the three colour words of
 *      U[q] are finite and its n is > 0.0f.  Any NaN makes a comparison false: the tap does not count.  U is S's temporal plane while that is
 *      current, otherwise S's colour plane with n = (float)rt_current_sample(S).
 *  18. the history.  sw = sn = sc[c] = 0.0f; each counted tap, in tap order, adds b, b * U.n and b * U[c].  !(sw > 0.0f): no history.  Otherwise
 *      H[c] = sc[c] / sw, nh = sn / sw, if (nh > max_history) nh = max_history.
 *  19. the blend.  nd = (float)rt_current_sample(D).  No history: T = (CD, nd) -- with nd == 0 four 0.0f.  History and nd == 0: T = (H, nh), a pure
 *      warp before the new view has a sample.  Otherwise inv = 1.0f / (nd + nh), T[c] = (CD[c] * nd + H[c] * nh) * inv, T.n = nd + nh.  D's colour
 *      plane is not read at pass 0.
 * INTENDED USE: two contexts take turns.  Frame k + 1 sets its camera or records on the OLDER context, resets it (rt_seed_stream_async gives frame k
 * stream k + 1), forms its features, renders a pass or two and reprojects from the other.  Because S's temporal plane is used while it is current,
 * history carries across many frames, capped by max_history.
 * LIMITS: history follows the FIRST hit.  What a mirror or a glass sphere shows, and the shadows moved spheres cast, lag by up to max_history samples
 * ("shadow-aware history" below ends the history of pixels where such a shadow came or went, while its setting is on).
 * A changed radius, material or emission is not detected.  Sky pixels have no history.
 * MEASURED, in numpy on a CPU before any kernel existed (the prototype; tests/test_reproject_cpu.py holds the restatement), with frames of this
 * project's oracle alone: 96x96, the camera's origin moved sideways by 2 % of its distance to the target, S at 16 passes of seed stream 1 from the
 * old origin, D at 2 passes of stream 2 from the new one, truth 1024 oracle passes of the new origin, PSNR over 8-bit channels packed by
 * clip ** (1 / 2.2) * 255 + .5, the defaults k_pos 4, max_history 64; dB:
 *     scene                      D alone     T        gain      hit pixels without history
 *     cornell (18 records)        11.60      20.77    +9.17            2.09 %
 *     Demo                        13.19      24.51   +11.32            0.94 %
 * (rt_reproject_planes gives the prototype's figures to the last digit: the two agree bit for bit.)  Two passes of a path tracer are mostly noise,
 * so sixteen older passes that lie within a pixel of the right place gain 9 to 11 dB; nothing there spoke against the defaults, and they were kept.
 * tests/test_reproject_cpu.py asserts half of each gain with rt_reproject_planes itself, and less than twice the share without history on cornell.
 * MEASURED on an MI355X by tools/reproject_probe.py (profiles/r27_reproject.jsonl; device time between two events, the device idle before the first,
 * medians of 12; NO TIME IS PROMISED), the Demo scene, 800x600 / 1920x1080:  rt_reproject_async from S's colour plane 0.019 / 0.057 ms, from S's
 * temporal plane 0.019 / 0.057 ms -- beside rt_features_async 0.010 / 0.021 ms and ONE pass 0.044 / 0.103 ms in the same run: a little over half
 * a pass.  A lane asks for words 4-7 of FD (16 bytes; words 0-3 are not needed and not read), per tap words 4-7 of FS and 12 or 16 bytes of U, 12
 * bytes of CD and two centres, and stores 20 bytes: 160 or 176 bytes a pixel, the taps of neighbouring pixels sharing their cache lines.  The quality
 * table from rendered contexts, reprojected on the device: 11.60 -> 20.77 dB and 2.09 % (cornell), 13.19 -> 24.51 dB and 0.94 % (Demo): the
 * prototype's figures to the last digit.                                                                                                          */
typedef struct { float k_pos; float max_history; uint32_t reserved[2]; } rt_reproject_params;   /* 16 bytes; both finite and > 0, reserved 0 */

/* {4.0f, 64.0f, {0, 0}}.  Needs no device.                                                                                      */
RT_API void rt_reproject_defaults(rt_reproject_params *p);

/* Rules 15-19 on `hip_stream`, without a host wait: src's history carried into dst's view and blended with dst's colour plane, into dst's temporal
 * plane and its packed plane.  Ordered behind everything both contexts have queued, and their later work behind it, as rt_merge_async; a table
 * rebuild that rt_update_spheres_async left pending on either context runs first, as in rt_features_async.  `p` == NULL means the defaults.
 * One kernel, one lane per pixel over 8x8 tiles as rt_features_async's, no LDS; the centres are read from the two contexts' geometry tables at id.
 * T is CURRENT from this call until something moves dst's colour plane -- a launch, a reset, rt_seed_stream_async, a written or loaded state, a merge
 * or a filter into it -- or ends dst's feature plane: rt_set_scene, rt_update_spheres_async, rt_set_camera.
 * RT_ERR_ARG: a null context, dst == src, contexts that differ in size or device, any multi-device or sharded context, k_pos or max_history not finite
 * or <= 0, reserved words not 0.  RT_ERR_STATE: either feature plane not current, either context ragged, scenes that differ in record count, a src with
 * neither a current temporal plane nor a pass.  A refused call changes nothing.                                                                   */
RT_API int rt_reproject_async(rt_ctx *dst, rt_ctx *src, const rt_reproject_params *p, void *hip_stream);

/* The context's temporal plane, 4 floats per pixel, into `rgbn_host`, and its packed plane, one word per pixel as rt_read_pixels lays them out, into
 * `packed_host`; either may be NULL, not both.  Blocking.  RT_ERR_STATE when T is not current; RT_ERR_ARG for a null, multi-device or sharded
 * context or two null buffers.                                                                                                                   */
RT_API int rt_read_temporal(rt_ctx *ctx, float *rgbn_host, uint32_t *packed_host);

typedef struct {                 /* one side of the host statement */
    const float *plane;          /* [h][w][channels], colour-plane row order; dst's may be NULL when its passes are 0 */
    int channels;                /* 3 = a colour plane, every pixel at `passes`; 4 = a temporal plane (rgb, n).  dst: rgb are read, nd is `passes` */
    int passes;
    const float *feat;           /* [h][w][8], rt_features_planes' layout */
    const rt_camera *cam;
    const rt_sphere *spheres;    /* `count` records */
} rt_reproject_view;

/* Rules 15-19 as plain host loops into out_rgbn[h][w][4]: what the device is tested against bit for bit.  The output may not overlap the inputs.
 * Needs no device.  RT_ERR_ARG: a null argument (a side's records may be null when count is 0), channels other than 3 or 4, negative passes, w or
 * h < 1, parameters rt_reproject_async refuses.                                                                                                  */
RT_API int rt_reproject_planes(float *out_rgbn, const rt_reproject_view *dst, const rt_reproject_view *src, uint32_t count, int w, int h,
                               const rt_reproject_params *p);

/* ---- edge-avoiding wavelet filter for the frame the interactive loop shows ------------------------------
 * The interactive loop of the section above ends in the temporal plane T, and nothing filtered it: the table there puts T at 20.8 dB (cornell) and
 * 24.5 dB (Demo) against 1024 passes, and pixels without history are raw one- or two-pass noise.  The filters of "denoising" need two independent
 * halves and cost five to eight interactive frames.  This section is an edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010;
 * the spatial stage of Schied et al.'s SVGF, 2017): ONE plane, 25 taps per level, steered by the feature plane rt_reproject_async needs anyway and
 * weighted by the sample count n that T carries.  Spheres make the geometry test exact: the scene index identifies the surface, and on a sphere the
 * normal identifies the point, so depth is not needed.  THIS LIBRARY'S OWN EXTENSION: it reproduces no reference frame, touches no render kernel and
 * changes no call above.
 *
 * THE ARITHMETIC, the same in rt_atrous_async's kernels and in rt_atrous_planes: all binary32, uncontracted, in the written order, IEEE division --
 * ALWAYS parity's arithmetic, whatever rt_set_mode says.  All planes are in the colour plane's row order; neighbours are ARRAY neighbours.
 * THE INPUT U has rgb and n per pixel: while the context's temporal plane is current U is that plane, otherwise its colour plane with
 * n = (float)rt_current_sample at every pixel (rule 17's convention).  F is the context's feature plane: id = word 7 compared as uint32 (0xFFFFFFFF is
 * an id like any other: sky filters with sky), N = words 3-5.
 *  20. luminance and usability.  lum(c) = (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2.  A pixel is USABLE when its three colour words of U are finite
 *      and its n > 0.0f.  Usability is judged on U once, for all levels.
 *  21. the variance estimate V0.  s0 = s1 = s2 = 0.0f; dy = -1 .. 1 outer, dx = -1 .. 1 inner, q = p + (dx, dy): a q inside the image that is usable
 *      and has id_q == id_p adds 1.0f to s0, l_q to s1 and l_q * l_q to s2, l_q = lum(U[q]).  s0 > 0.0f: m = s1 / s0, v = s2 / s0 - m * m,
 *      V0[p] = v > 0.0f ? v : 0.0f.  Otherwise V0[p] = 0.0f.
 *  22. one level takes (Ci, Vi) to (Ci+1, Vi+1) with step s = 1 << i; C0 = U's rgb.  hk = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
 *      in = 1.0f / (k_normal * k_normal), kl2 = k_lum * k_lum.  A pixel that is not usable KEEPS its Ci and Vi words: it stays what it was and spreads
 *      nowhere.  A usable p: lp = lum(Ci[p]), acc[c] = aw = av = 0.0f; taps j = -2 .. 2 outer, i = -2 .. 2 inner, q = p + s * (i, j).
 *      The centre tap (i = j = 0) always counts, wgt = (0.375f * 0.375f) * n_p.  Any other tap counts only when q is inside the image (no clamping),
 *      usable, and id_q == id_p; then a = N_p - N_q per component, gn = ((a0 * a0 + a1 * a1) + a2 * a2) * in; d = lp - lum(Ci[q]),
 *      gl = (d * d) / (kl2 * (Vi[p] + Vi[q]) + 1e-10f); g = 0.0f, if (gn > g) g = gn, if (gl > g) g = gl (a NaN term constrains nothing, as in rule 13);
 *      wgt = ((hk[j + 2] * hk[i + 2]) * (1.0f / (1.0f + g * (1.0f + g * 0.5f)))) * n_q.
 *      Each counted tap, in tap order, adds wgt * Ci[q][c] to acc[c], wgt to aw and (wgt * wgt) * Vi[q] to av.
 *      Ci+1[p][c] = acc[c] / aw, Vi+1[p] = av / (aw * aw); aw > 0 because the centre counts.
 *  23. the levels i = 0 .. levels - 1 run in turn; the output plane A[h][w][4] is (C_levels, V_levels).  With levels = 0, A = (U's rgb, V0) bit for bit.
 *  24. the packed plane: A's rgb words packed by the toInt of the context's mode, one uint32 per pixel in the PIXEL BUFFER's layout (row 0 = bottom),
 *      exactly as rt_reproject_async packs T.
 * WHAT THE FILTER DOES NOT DO: it never feeds back.  T, the colour plane, seeds, pass number, counters, selection, tile order and rt_last_kernel stay
 * as they are; rt_reproject_async reads T, never A, so history stays unfiltered and no bias accumulates across frames.  A is a frame to show.
 * LIMITS: the guidance is the FIRST hit's: inside a mirror or a glass sphere only the luminance test protects edges.  The variance estimate is spatial
 * (3x3, one frame) and over-estimates on shadow edges, which it therefore softens ("temporal luminance moments" below offers an estimate from the
 * pixel's history in its place, off by default).
 * MEASURED, in numpy on a CPU before any kernel existed (the prototype; tests/test_atrous_cpu.py holds the restatement), in the set-up of the table of
 * "temporal reprojection" (origin moved sideways by 2 %, S 16 passes of stream 1, D 2 passes of stream 2, truth 1024 oracle passes -- 512 at 192x192 --
 * PSNR over 8-bit channels), T = rt_reproject_planes' output, "D alone" = D's colour plane with n = 2 everywhere, k_lum 1.5, k_normal 0.3; dB:
 *     scene, size          T       T filtered, levels 1 / 2 / 3 / 4 / 5          D alone   D alone filtered, levels 3
 *     cornell 96x96      20.77    25.07 / 26.72 / 27.13 / 27.22 / 27.26          11.60        21.57
 *     Demo 96x96         24.51    27.50 / 27.64 / 27.16 / 26.70 / 26.36          13.19        23.05
 *     simple 96x96       28.14    29.55 / 29.30 / 29.13 / 28.86 / 28.62          16.54        25.97
 *     Demo 192x192       24.89    28.37 / 29.17 / 29.15 / 28.87 / 28.59          13.25        23.88
 *     cornell 192x192    20.07    24.53 / 26.40 / 27.05 / 27.29 / 27.39          11.60        22.14
 * With levels 0 the output is T bit for bit.  Diffuse scenes gain with every level; scenes of glass and mirrors peak at one or two, because inside a
 * reflection only the luminance test protects edges and the spatial variance estimate is inflated there.  Three levels is the compromise and the default.
 * tests/test_atrous_cpu.py asserts half of each gain at 96x96 with rt_atrous_planes itself.
 * MEASURED on an MI355X by tools/atrous_probe.py (profiles/r30_atrous.jsonl; device time between two events, the device idle before the first,
 * medians of 12; NO TIME IS PROMISED), the Demo scene, 800x600 / 1920x1080: rt_atrous_async from T with 1 / 3 / 5 levels 0.072 / 0.160 / 0.236 ms and
 * 0.247 / 0.581 / 0.865 ms, from the colour plane 0.070 / 0.159 / 0.234 ms and 0.253 / 0.587 / 0.861 ms; with no level -- the preparation kernel
 * alone -- 0.024 / 0.073 ms.  Beside it in the same run: ONE pass 0.042 / 0.093 ms, rt_features_async 0.010 / 0.020 ms, rt_reproject_async 0.018 /
 * 0.054 ms, rt_denoise_async (two halves of one pass, the defaults) 0.253 / 0.839 ms.  So the default three levels cost 0.63 / 0.69 of rt_denoise_async
 * and 2.3 / 3.5 times the interactive frame they filter (features, one pass, reprojection: 0.070 / 0.167 ms); one level 1.0 / 1.5 times.
 * A level is 0.17 ms at 1920x1080 at steps 1 to 4 and 0.14 ms at steps 8 and 16: the time does not grow with the taps' spread, and by instruction count
 * most of it is the rules' own arithmetic, 25 taps of two IEEE divisions each.
 * The quality table from rendered contexts, filtered on the device: at 96x96 and 192x192 the prototype's figures above to the last digit.  At
 * 800x600, which the prototype had not measured (truth 1024 passes):
 *     Demo 800x600       25.87    30.67 / 32.54 / 33.00 / 33.05 / 32.94          14.04        25.63
 *     cornell 800x600    20.99    25.58 / 27.92 / 28.89 / 29.30 / 29.51          11.76        22.90
 * -- larger frames gain more (+7.1 and +7.9 dB at three levels) and peak later: a pixel's footprint shrinks, so more taps lie on its surface.  Quality
 * has not been measured at 1920x1080.                                                                                                             */
typedef struct { int32_t levels; float k_lum; float k_normal; uint32_t reserved; } rt_atrous_params;   /* 16 bytes; levels 0 .. 5, both k finite and > 0, reserved 0 */

/* {3, 1.5f, 0.3f, 0}.  Needs no device.                                                                                          */
RT_API void rt_atrous_defaults(rt_atrous_params *p);

/* Rules 20-24 on `hip_stream`, without a host wait: the context's temporal plane while that is current, otherwise its colour plane, filtered into the
 * (rgb, variance) plane A and its packed plane, which the context owns (allocated on first use with three working planes, freed by rt_destroy).  Ordered
 * behind everything the context has queued, its later work behind the call.  `p` == NULL means the defaults.  One preparation kernel (rules 20-21) and
 * one kernel per level, one lane per pixel.
 * A is CURRENT from this call until anything that ends the temporal plane -- a launch, a reset, rt_seed_stream_async, a written or loaded state, a
 * merge or a filter into the context, rt_set_scene, rt_update_spheres_async, rt_set_camera -- a new rt_reproject_async into the context, or a feature
 * plane formed again where none was current.
 * RT_ERR_ARG: a null, multi-device or sharded context, levels outside 0 .. 5, k_lum or k_normal not finite or <= 0, reserved not 0.  RT_ERR_STATE:
 * the feature plane is not current, the context is ragged, there is neither a current temporal plane nor a pass.  A refused call changes nothing.  */
RT_API int rt_atrous_async(rt_ctx *ctx, const rt_atrous_params *p, void *hip_stream);

/* The filtered plane, 4 floats per pixel (rgb, variance) in the colour plane's row order, into `rgbv_host`, and its packed plane, one word per pixel as
 * rt_read_pixels lays them out, into `packed_host`; either may be NULL, not both.  Blocking.  RT_ERR_STATE when A is not current; RT_ERR_ARG for a
 * null, multi-device or sharded context or two null buffers.                                                                                     */
RT_API int rt_read_atrous(rt_ctx *ctx, float *rgbv_host, uint32_t *packed_host);

/* Rules 20-23 as plain host loops into out_rgbv[h][w][4]: what the device is tested against bit for bit.  `plane` is [h][w][channels]: 3 = a colour
 * plane, every pixel at n = (float)passes; 4 = a temporal plane (rgb, n), `passes` not read.  `feat` is [h][w][8], rt_features_planes' layout.  The
 * output may not overlap the inputs.  Needs no device.  RT_ERR_ARG: a null plane, channels other than 3 or 4, negative passes, w or h < 1, parameters
 * rt_atrous_async refuses.                                                                                                                       */
RT_API int rt_atrous_planes(float *out_rgbv, const float *plane, int channels, int passes, const float *feat, int w, int h, const rt_atrous_params *p);

/* ---- temporal luminance moments: the a-trous variance from a pixel's history -----------------------------
 * Rule 21 estimates the variance the a-trous filter is steered by from ONE frame, a 3x3 neighbourhood, and so mistakes structure for noise: it
 * over-estimates on shadow edges and inside mirrors and glass.  The interactive loop already follows a surface point through many frames, each
 * rendered on a seed stream of its own, so how a pixel's luminance varied FROM FRAME TO FRAME measures its noise and not its neighbourhood: a static
 * shadow edge has low temporal variance, a noisy flat wall a high one.  This section carries the first and second luminance moments and a frame count
 * through rt_reproject_async and lets rt_atrous_async take V0 from them (Schied et al.'s SVGF, 2017).  THIS LIBRARY'S OWN EXTENSION: it reproduces no
 * reference frame and touches no render kernel, and WITH THE SETTING OFF, WHICH IS THE DEFAULT, every call above is what it was.
 *
 * THE MOMENTS PLANE is M[h][w][4] floats in the colour plane's row order, owned by dst: (m1, m2, k, v) -- the mean luminance of the pixel's history,
 * the mean of its square, the number of frames behind it, and the variance estimate of rule 27.  rt_reproject_async(dst, src, ..) forms it beside T
 * while the setting is ON FOR dst; it is allocated on first use and freed by rt_destroy.  M IS CURRENT exactly while dst's temporal plane is current
 * AND that plane's last rt_reproject_async ran with the setting on: its currency is derived from T's, not a state of its own.  rt_atrous_async(ctx, ..)
 * applies rule 28 when the setting is on for ctx AND M is current -- that test alone decides; turning the setting off or on moves no plane.
 *
 * THE ARITHMETIC, the same in the kernels and in the two host functions: binary32, uncontracted, in the written order, IEEE division -- ALWAYS
 * parity's arithmetic.  lum is rule 20's; D, S, U, b, sw, sn, nd, nh and inv are those of rules 15-19.
 *  25. a tap's moments.  The taps COUNT exactly as in rule 17; moments never decide whether a tap counts.  While S's moments plane MS is current,
 *      (m1q, m2q, kq) are words 0-2 of MS[q].  Otherwise lq = lum(U[q]) and (m1q, m2q, kq) = (lq, lq * lq, 1.0f): an S without the setting, an S whose
 *      temporal plane was formed without it, and an S read through its colour plane -- whatever S holds then counts as ONE frame.
 *  26. the history's moments.  s1 = s2 = sk = 0.0f; each counted tap, in tap order, adds b * m1q, b * m2q and b * kq.  With history (sw > 0.0f):
 *      h1 = s1 / sw, h2 = s2 / sw, hk = sk / sw, and with nr = sn / sw (rule 18's nh before its cap): if (nr > max_history) hk = hk * (max_history / nr)
 *      -- frames are capped in proportion to samples.
 *  27. the blend.  lD = lum(CD).  No history and nd == 0: four 0.0f.  No history otherwise: (lD, lD * lD, 1.0f, 0.0f).  History and nd == 0:
 *      (h1, h2, hk, v).  Otherwise m1 = (lD * nd + h1 * nh) * inv, m2 = ((lD * lD) * nd + h2 * nh) * inv, k = hk + 1.0f.
 *      The estimate: d = m2 - m1 * m1; v = (k > 1.0f && d > 0.0f) ? d / (k - 1.0f) : 0.0f (a NaN makes both comparisons false).
 *      Why this form: T is the sample-weighted mean of per-frame means l_k, and for K frames of equal counts
 *      Var(T) = sum (l_k - m1)^2 / (K (K - 1)) = (m2 - m1^2) / (K - 1).  With unequal counts and under the cap it is an APPROXIMATION.
 *  28. V0 from history.  In rt_atrous_async's preparation step, for a pixel p that is usable (rule 20) with M[p].k >= k_min: V0[p] = M[p].v.  Every
 *      other pixel keeps rule 21.  Rules 22-24 are unchanged.  When rt_atrous_async filters the colour plane (no current T), M is not consulted.
 * INVARIANTS: (a) T and its packed plane are bit for bit the same with the setting on or off.  (b) With k_min larger than any k present the a-trous
 * output is bit for bit the plain one.  (c) With levels = 0, A's variance word is M's v where rule 28 applies.
 * LIMITS: like T, the moments follow the FIRST hit: what a mirror shows of a moving scene lags, and its frame-to-frame change counts as noise.  The
 * estimate is an approximation where frames hold unequal sample counts and under max_history's cap; below k_min frames rule 21 stands in.
 * k is a weighted MEAN of the taps' frame counts, not an integer: a pixel whose four taps all held 3 frames may come out a rounding below 4 after the
 * next blend, and then needs one frame more to reach k_min 4.
 * MEASURED, in numpy on a CPU before any kernel existed (the prototype; tests/test_moments_cpu.py holds the restatement), with frames of this
 * project's oracle alone: 96x96, EIGHT frames of 2 passes, frame f on seed stream f from an origin moved sideways by f * 0.5 % of its distance to
 * the target, two sides taking turns as INTENDED USE above has it (the first frame's colour plane is the second's source), the defaults of
 * rt_reproject_async, truth 1024 oracle passes of the last view, PSNR over 8-bit channels as in the tables above; A by rule 21 against A by rule 28
 * (k_min 4) at EQUAL levels, dB:
 *     scene      last T    rule 21, levels 1 / 3 / 5    rule 28, levels 1 / 3 / 5    gain at 3     pixels at k >= 4
 *     cornell    22.13     25.26 / 26.68 / 26.81        26.07 / 27.94 / 27.95        +1.26            99.9 %
 *     simple     27.68     29.16 / 28.89 / 28.52        29.58 / 29.61 / 29.19        +0.72            52.9 %
 *     Demo       24.69     27.34 / 27.03 / 26.21        27.59 / 27.10 / 26.26        +0.06            78.5 %
 * The same over the pixels within 2 pixels of a SHADOW EDGE -- defined on the truth frame: a pair of 4-neighbours that show the same diffuse record
 * with normals within 0.1 of each other, both luminances below 1, differing by more than 35 % of the larger; on these scenes the rims of shadows and,
 * under glass spheres, of caustics; 10.6 / 10.3 / 20.4 % of the pixels:
 *     cornell    21.49     24.13 / 24.38 / 24.37        24.62 / 24.45 / 24.34        +0.07
 *     simple     22.50     23.26 / 22.46 / 22.35        24.11 / 23.92 / 23.80        +1.47
 *     Demo       20.95     23.46 / 22.78 / 22.16        23.53 / 22.58 / 21.98        -0.20
 * So the estimate pays on the whole frame of the two fixtures (+1.3 and +0.7 dB at three levels, at every level measured) and does nothing for Demo
 * (+0.06 dB); at shadow edges, which it was meant for, it gains 1.5 dB on `simple`, nothing on cornell beyond one level, and LOSES 0.2 dB on Demo at
 * three and five levels, where the edges lie under glass spheres whose caustics flicker from frame to frame: a high temporal variance there opens the
 * luminance stop across the edge.  k_min stays at 4.  tests/test_moments_cpu.py asserts half of the two whole-frame gains and, for Demo, no more than
 * 0.3 dB below rule 21, with the two host functions.
 * MEASURED on an MI355X by tools/moments_probe.py (profiles/r32_moments.jsonl; device time between two events, the device idle before the first, the
 * setting ON and OFF alternating call by call in one process, medians of 12 each; NO TIME IS PROMISED), the Demo scene, 800x600 / 1920x1080, on against
 * off: rt_reproject_async from a source's colour plane 0.0213 against 0.0195 ms / 0.0612 against 0.0568 ms (+8 %: the 16-byte store and the sums);
 * from a source's temporal and moments planes 0.0231 against 0.0196 ms / 0.0764 against 0.0578 ms (+32 % at 1920x1080: the extra 16-byte load per
 * tap costs more than the estimate of one load in five assumed); rt_atrous_async with no level -- the preparation kernel alone -- 0.0238 against
 * 0.0238 ms / 0.0786 against 0.0757 ms, with three levels 0.1598 against 0.1582 ms / 0.5773 against 0.5744 ms.  The interactive frame (features, a
 * pass, reprojection, three levels: about 0.75 ms at 1920x1080) grows by some 0.02 ms.  The quality table from rendered contexts, reprojected and
 * filtered on the device: the prototype's figures above to the last digit, all three scenes, both tables.                                           */
typedef struct { float k_min; uint32_t reserved[3]; } rt_moments_params;   /* 16 bytes; k_min finite and >= 1, reserved 0 */

/* {4.0f, {0, 0, 0}} -- SVGF's four frames.  Needs no device.                                                                     */
RT_API void rt_moments_defaults(rt_moments_params *p);

/* The context's setting that rt_reproject_async INTO it and rt_atrous_async OF it consult, as rt_set_denoise_guide's is consulted by the filters;
 * NULL turns it off (the default).  Moves no plane and ends none.  RT_ERR_ARG: a null, multi-device or sharded context, k_min not finite or < 1,
 * reserved words not 0.  A refused call changes nothing.                                                                                          */
RT_API int rt_set_temporal_moments(rt_ctx *ctx, const rt_moments_params *m);

/* The context's moments plane, 4 floats per pixel (m1, m2, k, v) in the colour plane's row order.  Blocking.  RT_ERR_STATE when M is not current;
 * RT_ERR_ARG for a null, multi-device or sharded context or a null buffer.                                                                         */
RT_API int rt_read_moments(rt_ctx *ctx, float *m_host);

/* Rules 15-19 and 25-27 as plain host loops into out_rgbn[h][w][4] and out_m[h][w][4]: what the device is tested against bit for bit.  out_rgbn is
 * rt_reproject_planes' output bit for bit.  `src_m` is S's moments plane [h][w][4], or NULL for rule 25's luminance of U.  RT_ERR_ARG: a null
 * output, and whatever rt_reproject_planes refuses.                                                                                               */
RT_API int rt_reproject_moments_planes(float *out_rgbn, float *out_m, const rt_reproject_view *dst, const rt_reproject_view *src,
                                        const float *src_m /* [h][w][4] or NULL */, uint32_t count, int w, int h, const rt_reproject_params *p);

/* Rules 20-23 with rule 28 as plain host loops; `m` is the moments plane [h][w][4], NULL = rule 21 everywhere (rt_atrous_planes bit for bit).  `mp`
 * == NULL means the defaults.  RT_ERR_ARG: whatever rt_atrous_planes refuses, and parameters rt_set_temporal_moments refuses.                       */
RT_API int rt_atrous_moments_planes(float *out_rgbv, const float *plane, int channels, int passes, const float *m /* NULL = rule 21 everywhere */,
                                     const float *feat, int w, int h, const rt_atrous_params *p, const rt_moments_params *mp);

/* ---- shadow-aware history: a pixel's history ends where a moved sphere's shadow comes or goes ---------------
 * History follows the first hit ("temporal reprojection", LIMITS): a floor pixel under a shadow that has just left keeps up to max_history dark
 * samples against two new lit ones, and the filter then smooths the ghost instead of removing it.  In this renderer the occluders are spheres and
 * the host knows which records changed, so the question "did the direct light at this point change?" has a geometric answer: for the point under a
 * pixel and a light, decide whether a changed sphere stands in the cone from the point to the light, before and after the change.  Where that state
 * differs, or is a penumbra, the pixel's history is capped at `keep` samples.  THIS LIBRARY'S OWN EXTENSION: it reproduces no reference frame and
 * touches no render kernel, and WITH THE SETTING OFF, WHICH IS THE DEFAULT, every call above is what it was and launches the kernel it launched.
 *
 * THE FLAG PLANE is K[h][w], one byte per pixel, 0 or 1, in the colour plane's row order, owned by dst.  rt_reproject_async(dst, src, ..) forms it
 * beside T while the setting is ON FOR dst; it is allocated on first use and freed by rt_destroy.  K IS CURRENT exactly while dst's temporal plane is
 * current AND that plane's last rt_reproject_async ran with the setting on -- derived from T's currency, as M's is.
 *
 * THE ARITHMETIC, the same in the kernels and in rt_reproject_shadow_planes: binary32, uncontracted, in the written order, IEEE division -- ALWAYS
 * parity's arithmetic; no square root.  dot is rule 15's; D, S, P, Pp, id, nd, nh, sw and hk are those of rules 15-19 and 26.  The records are
 * read from the two contexts' host mirrors (device) or the two views (host function) to build the lists, and from the lists afterwards.
 *  29. the lists.  Record j is a LIGHT when the library's own light test holds for D's record j: !(e.x == 0.f && e.z == 0.f).  Record j is CHANGED
 *      when any of the four words {centre, radius} of S's and D's record j differ BITWISE.  Records whose radius is 0.0f on both sides are neither
 *      (the loader's phantom records).  A PAIR (l, j) exists when l is a light, j != l, j is no such zero-radius record, and l or j is changed.
 *      Pairs are ordered l ascending outer, j ascending inner.  A pair carries S's and D's {centre, radius} of l and of j.  No pair: no flag.
 *  30. a pair's state at a point, state(X, L, rl, c, r).  seg = L - X per component, ll = dot(seg, seg); !(ll > 0.0f): state 0.
 *      s = dot(c - X, seg) / ll;  if (!(s > 0.0f)) s = 0.0f;  if (s > 1.0f) s = 1.0f.
 *      e = (X + seg * s) - c, d2 = dot(e, e), pen = rl * s, a = r + pen, b = r - pen.
 *      State 0 (clear) when d2 > a * a; otherwise state 2 (umbra) when b > 0.0f && d2 < b * b; otherwise state 1 (penumbra).  A NaN makes every
 *      comparison false and so gives state 1.  The cone is that of the light's bounding sphere, seen from the point.
 *  31. the flag of pixel p.  p is flagged only when it has history (sw > 0.0f) and nd != 0: at pass 0 the call is a pure warp and nothing newer
 *      exists to prefer.  For each pair in order with id != l and id != j:  old = state(Pp, S's l, S's j), new = state(P, D's l, D's j); the pair
 *      CHANGES p when old != new || old == 1 || new == 1.  p is FLAGGED when any pair changes it.  (The host loop stops at the first such pair; the
 *      device predicates.)
 *  32. the effect.  For a flagged pixel, after rule 18's cap:  if (nh > keep) { hk = hk * (keep / nh); nh = keep; } -- the hk part in the moments arm
 *      only, in proportion as rule 26 caps frames.  Rules 19 and 27 then run unchanged.  With keep 0 a flagged pixel comes out as (CD, nd).
 * INVARIANTS: (a) with no changed record T, its packed plane and M are bit for bit what they are with the setting off, and K is all 0.  (b) With
 * keep >= max_history T and M are bit for bit the plain ones while K may hold ones.  (c) At nd == 0, K is all 0.
 * LIMITS: a moved sphere's own shading, a moved light's falloff on unshadowed surfaces, reflections, refractions and caustics still lag.  (A mirror
 * rule -- flag a mirror pixel whose reflected ray meets a moved sphere -- was prototyped: it changed A by -0.07 and 0.00 dB and is not part of this.)
 * A changed material or emission is not detected; a record that BECOMES a light is a light (D's record decides), one that ceases to be is not.
 * REJECTED: textbook variance clipping -- the history clipped to mean +- k sigma of the new frame's 5x5 or 7x7 same-record neighbourhood, sigma of
 * the pixels or the standard error of the mean, k 1 .. 6, with and without shrinking nh.  At two passes the box is as wide as the change it should
 * catch: T moved by -0.1 .. +1.9 dB, the filtered frame A (three levels) by -1.8 .. +0.0 dB, and a static scene lost 0.1 .. 1.1 dB.
 * MEASURED with rt_reproject_shadow_planes and rt_atrous_planes on a CPU (tests/test_shadow_history_cpu.py), frames of this project's oracle alone:
 * 96x96, TWELVE frames of 2 passes, frame f on seed stream f with one record moved by (f - 1) steps, the camera still, two sides taking turns, the
 * defaults (keep 2), truth 512 oracle passes of the last frame's scene, PSNR over 8-bit channels as in the tables above; off -> on, dB:
 *     scene, moved record, step per frame        T                  A, 3 levels              A over the changed region (share)   flagged, last frame
 *     cornell, glass sphere 16, (-1.5, 0, 0)     19.52 -> 19.58     24.56 -> 25.52 (+0.97)   18.36 -> 21.19 (9.5 %)                   3.9 %
 *     Demo, sphere 4, (-2, 0, 0)                 22.72 -> 23.01     25.58 -> 26.65 (+1.07)   15.74 -> 19.45 (3.6 %)                   1.0 %
 *     simple, sphere 6, (-2.5, 0, 0)             26.52 -> 26.74     28.26 -> 28.53 (+0.27)   12.17 -> 13.14 (0.7 %)                   0.2 %
 * CHANGED REGION: pixels of the last view whose first hit is the same record as with the sphere where it stood six frames earlier, both truth
 * luminances below 1 and differing by more than 25 % of the larger.  (The numpy prototype that preceded the rules -- binary64, a square root, both
 * states at the new point, the sphere a step further in every frame -- gave A 24.76 -> 25.81, 25.43 -> 26.52 and 28.20 -> 28.57.)  T hardly moves
 * -- a flagged pixel trades a biased mean for a noisy one -- and the FILTER gains: it spreads the right two samples instead of the wrong
 * sixty-four, by 1 to 3.7 dB where the light changed.  `simple` gains less than 0.3 dB over the frame because 0.2 % of it is flagged.  The test
 * asserts half of the two larger whole-frame gains and, for `simple`, no more than 0.3 dB below "off".
 * MEASURED on an MI355X by tools/shadow_history_probe.py (profiles/r33_shadow_history.jsonl; device time of rt_reproject_async between two events,
 * the device idle before the first, the setting ON and OFF alternating call by call in one process, medians of 12; NO TIME IS PROMISED), the Demo
 * scene followed by small spheres buried in the ground, that many of them moved -- they shadow nothing, so no pixel is flagged and every pixel with
 * history walks the WHOLE list, the worst case -- from a source's colour plane, 800x600 / 1920x1080, on against off:
 *     1 pair       0.0262 against 0.0188 ms  /  0.0640 against 0.0555 ms
 *     16 pairs     0.0408 against 0.0189 ms  /  0.1069 against 0.0554 ms
 *     1024 pairs   1.0227 against 0.0181 ms  /  3.2008 against 0.0537 ms
 * The instance itself (one pair: the flag plane's byte, the LDS chunk, two barriers, lanes that stay) costs 0.008 ms at either size; a pair costs
 * 1.5 ps per pixel at 1920x1080 (2.0 ps at 800x600): two states -- two IEEE divisions and some forty other operations -- per pair and pixel with
 * history.  A few moved spheres under a light or two are a fraction of a pass (0.103 ms at 1920x1080); a moved LIGHT in a scene of a thousand records
 * costs thirty passes, and the caller who moves one should leave the setting off for that frame.  The quality table from rendered contexts,
 * reprojected and filtered on the device: the CPU table's T and A figures and flagged shares to the last digit, all three scenes.
 */
#define RT_SHADOW_PAIR_CHUNK 64     /* pairs of rule 29 that the kernels stage in LDS at a time (80 bytes each) */
typedef struct { float keep; uint32_t reserved[3]; } rt_shadow_history_params;   /* 16 bytes; keep finite and >= 0, reserved 0 */

/* {2.0f, {0, 0, 0}}.  Needs no device.                                                                                           */
RT_API void rt_shadow_history_defaults(rt_shadow_history_params *p);

/* The context's setting that rt_reproject_async INTO it consults, as rt_set_temporal_moments' is; NULL turns it off (the default).  Moves no plane and
 * ends none.  RT_ERR_ARG: a null, multi-device or sharded context, keep not finite or < 0, reserved words not 0.  A refused call changes nothing.   */
RT_API int rt_set_shadow_history(rt_ctx *ctx, const rt_shadow_history_params *params);

/* The context's flag plane K, one byte per pixel (0 or 1) in the colour plane's row order.  Blocking.  RT_ERR_STATE unless the temporal plane is
 * current and its last rt_reproject_async ran with the setting on; RT_ERR_ARG for a null, multi-device or sharded context or a null buffer.        */
RT_API int rt_read_history_flags(rt_ctx *ctx, uint8_t *k_host);

/* Rules 15-19, 25-27 and 29-32 as plain host loops: what the device is tested against bit for bit.  out_rgbn[h][w][4] always; out_m[h][w][4] (rules
 * 25-27) and out_k[h][w] (rule 31's flags) where not NULL; `src_m` as rt_reproject_moments_planes takes it (read only with out_m).  `sp` == NULL: no
 * shadow rules -- rt_reproject_planes and rt_reproject_moments_planes are calls of this function with sp NULL -- and out_k, if given, is all 0.
 * RT_ERR_ARG: whatever rt_reproject_planes refuses, and parameters rt_set_shadow_history refuses.                                                 */
RT_API int rt_reproject_shadow_planes(float *out_rgbn, float *out_m /* or NULL */, uint8_t *out_k /* or NULL */, const rt_reproject_view *dst,
                                       const rt_reproject_view *src, const float *src_m /* [h][w][4] or NULL */, uint32_t count, int w, int h,
                                       const rt_reproject_params *p, const rt_shadow_history_params *sp /* NULL = off */);

/* Rule 29's pair list of the records S (before) and D (after), `count` each, in rule 29's order: the indices (l, j) of up to `cap` pairs into
 * out_lj[2 * k], out_lj[2 * k + 1] (NULL with cap 0 to count).  Returns the number of pairs the records have, or -1 for a null argument.  Needs no
 * device.                                                                                                                                        */
RT_API int rt_shadow_history_pairs(const rt_sphere *src_spheres, const rt_sphere *dst_spheres, uint32_t count, uint32_t *out_lj, uint32_t cap);

RT_API int rt_get_stats(rt_ctx *ctx, rt_stats *out);
/* The kernel instance the context's last launch used, by its symbol (what a profiler lists): the library picks it
 * from the scene -- "rt_trace_parity_w1" (few spheres: one wavefront per workgroup), "..._coop_w1" / "..._coop"
 * (12 and more: wave-ballot any-hit sharing; with 4 to 11 spheres whichever of the two the scene's first launches timed
 * faster -- coop warm, coop timed, plain warm, plain timed: passes of the frame like any other), "..._pairs" (hundreds of
 * small spheres: a hierarchy, where it measured faster than the sweep on this scene; "..._pairs_m" / "..._pairs_g" when its
 * tables outgrow LDS), "..._g" (a plain sweep over a table beyond its LDS budget, read through the scalar cache), the same with "fast".  "" before the first launch.
 * Frames do not depend on it. */
RT_API const char *rt_last_kernel(const rt_ctx *ctx);
/* Hierarchy or plain sweep for the current scene (scenes with 56 to 1500 small spheres; larger ones always walk the
 * hierarchy).  rt_set_scene builds the tree on the host and with it a surface-area estimate of what a ray costs either
 * way; where the estimate is clear (predicted ratio outside 0.75 .. 1.33) it decides and nothing is measured, so a new
 * scene's first frame costs what a frame costs.  Inside that band -- and after device-resident updates that changed the
 * tree's size by a quarter -- the first launches time both forms (hierarchy warm, hierarchy timed, sweep warm, sweep timed;
 * passes of the frame like any other) and the faster one renders the rest.  Returns 0 = not decided (yet, or a scene that
 * has no choice), 1 = hierarchy, 2 = plain sweep, and the two MEASURED times per pass in milliseconds (0 when the estimate
 * decided or nothing was measured).  Never blocks; of a multi-device context, the first shard's. */
RT_API int rt_scene_choice(rt_ctx *ctx, double *hierarchy_ms_per_pass, double *sweep_ms_per_pass);

/* Identity of the sources and compiler flags this library was built from (16 hex digits).  tools/summarize_profile.py stamps
 * every profile record with it; bench.py prints a committed profile's counters only beside the library they were measured on. */
RT_API const char *rt_build_id(void);

/* Text of the calling thread's last failure ("" if none).                                    */
RT_API const char *rt_last_error(void);

/* ---- host-side helpers either side of the path ---------------------------- */

/* computeCameraVariables, Utility.cpp:71-85 (Vec::norm's double sqrt, Vec.cpp:28-30).        */
RT_API void rt_compute_camera(rt_camera *cam, int w, int h);

/* The seed initialisation of OpenCLConfig.cpp:676-680 without depending on the host libc:
 * glibc's never-seeded rand() stream restated, each value clamped to >= 2.                   */
RT_API void rt_default_seeds(uint32_t *seeds, size_t count);

/* Seed stream `stream_id` of this library (an extension: the reference has the one stream above).  stream_id == 0 is
 * rt_default_seeds.  Otherwise the pair of pixel i -- words 2i and 2i + 1, the flat order of rt_read_seeds -- is the splitmix64
 * finaliser of (stream_id, i), all arithmetic wrapping in uint64:
 *     z = stream_id * 0x9E3779B97F4A7C15 + i + 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;   z ^= z >> 31
 *     seeds[2i] = max(low32(z), 2),  seeds[2i + 1] = max(high32(z), 2)      -- the reference's clamp, OpenCLConfig.cpp:676-680
 * An odd `count` ends on a low half.  Needs no device; rt_seed_stream_async writes the same words on the device.        */
RT_API void rt_stream_seeds(uint64_t stream_id, uint32_t *seeds, size_t count);

/* DemoSpheres, Scene.cpp:5-12.  Returns the sphere count (6), or -count if cap is smaller.   */
RT_API int rt_demo_scene(rt_sphere *out, uint32_t cap);

/* readScene, Utility.cpp:90-160: "camera ox oy oz tx ty tz" / "size N" / N x "sphere rad
 * px py pz ex ey ez cx cy cz mat".  With reference_doubling != 0 the result is what the
 * reference's loader actually hands to the kernel: N value-initialised spheres followed by
 * the N parsed ones (:120,154).  Returns RT_OK and *count, or RT_ERR_ARG (rt_last_error).    */
RT_API int rt_read_scene(const char *path, rt_sphere *out, uint32_t cap, uint32_t *count,
                  rt_vec3 *orig, rt_vec3 *target, int reference_doubling);

/* ---- frame assembly on the gather root --------------------------------------
 * De-interleave kernel: `gathered` holds the ranks' local pixel blocks one after another, rank r
 * at gathered + r * pad_rows * w (its rows packed in order, as rt_create_sharded lays them out);
 * full[y * w + x] = the pixel of image row y.  Both are DEVICE pointers on `device`; asynchronous
 * on `hip_stream`.  Used by the in-library multi-GPU context and by process-per-GPU hosts after
 * their own gather (bench.py: torch.distributed over RCCL).                                    */
RT_API int rt_deinterleave_rows(uint32_t *full, const uint32_t *gathered, int w, int h, int nranks,
                                int tile_rows, int pad_rows, int device, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
