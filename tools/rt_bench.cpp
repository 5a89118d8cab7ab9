// rt_bench.cpp -- headless C++ host for the HIP render path: what the reference's Main.cpp
// does (SimpleRT/src/Main.cpp:18-113) minus the GLUT window, with an image writer instead.
//
//   rt_bench <framework ID> <CPU/GPU (0/1)> <mem (0/1/2)> [scene.scn]
//            [--w W] [--h H] [--spp N] [--passes-per-launch K] [--pin] [--readback-ms T] [--mode parity|fast]
//            [--no-doubling] [--out frame.ppm] [--oneshot K] [--gpus N]
//            [--stream N] [--save-state FILE] [--load-state FILE] [--until-psnr DB [--check-every N] [--adaptive [--min-passes M]]
//             [--denoise [--denoise-radius R]] [--filtered [--live-checks]] [--guided]] [--atrous [--atrous-levels N] [--moments [--moments-kmin K]]]
//            [--shadow-history [--shadow-keep N]]
//   --oneshot K   render through the headline call rt_render(scene, cam, out, w, h, spp) K times instead of a
//                 context (prints the wall time of every call: the first builds the device state, the rest reuse it)
//   --gpus N      a multi-device context (rt_create_multi: N GPUs of this process, one RCCL gather per frame)
//   --rehearse N  the same with all N shards on device 0 (rt_create_multi_on: the one-GPU rehearsal of that path)
//   --stream N    render on seed stream N of the library (rt_seed_stream_async; 0 = the reference's default stream)
//   --load-state FILE   continue the frame a checkpoint holds (rt_load_state): --spp is the number of passes to ADD
//   --save-state FILE   write the frame's state when the passes are done (rt_save_state)
//   --until-psnr DB     render two contexts on seed streams 1 and 2 in step (rt_render_converged) until the PSNR BETWEEN them reaches DB or
//                       each holds --spp passes, checking every --check-every N passes (default 8); then merge them (rt_merge_async) and
//                       write --out from the merged frame.  Prints passes per half, checks and the last PSNR of the pair -- the merged
//                       frame is better than that figure (include/rt_api.h, rt_render_converged)
//   --adaptive          with --until-psnr: DB is the target PER 8x8 TILE and only the groups of tiles still below it are rendered
//                       (rt_render_adaptive), after --min-passes M passes on every tile (default 16).  A second line gives the checks, the
//                       samples rendered against w * h * passes of both halves, and the smallest, median and largest tile pass count
//   --denoise           with --until-psnr: the halves are merged into a THIRD context, that frame is filtered (rt_denoise_async: non-local
//                       means steered by the difference of the halves) and --out is written from it; --denoise-radius R sets the search
//                       radius (0 .. 8, default 5).  A further line gives the parameters and the call's wall time (queue, kernels, pack, read-back)
//   --filtered          with --until-psnr: DB is the target for the FILTERED merge.  The check is the PSNR between the two cross-filtered halves
//                       (rt_render_converged_filtered; with --adaptive per tile, rt_render_adaptive_filtered) -- an estimate of the filtered
//                       frame's quality, not a bound -- and the halves are then merged and filtered as by --denoise, with the same parameters
//   --guided            with --denoise or --filtered: the feature planes of both halves are formed (rt_features_async) and the guide's defaults
//                       set on them (rt_set_denoise_guide), so that every filter of the run -- the checks and the final one -- restricts its
//                       weights by albedo, normal and depth
//   --live-checks       with --until-psnr DB --filtered --adaptive: every check after the first cross-filters only the groups that were just
//                       rendered (rt_render_adaptive_filtered_tiles): the same render bit for bit; the printed PSNR sums every group's
//                       figure of its own last check
//   --atrous            the context the frame ends in -- the one context, or with --until-psnr the merged (and filtered) one -- forms its
//                       feature plane and runs the edge-avoiding wavelet filter over its colour plane (rt_features_async, rt_atrous_async;
//                       --atrous-levels N: 0 .. 5, default 3); --out is written from the filtered frame.  A further line names the kernel that formed
//                       the plane and its device time between two events (a large .scn scene: what the plane cost beside the pass), and gives the
//                       parameters and the wall time of the two calls and the read-back.  Not with --gpus / --rehearse
//   --moments           with --atrous: the filter takes its variance from a pixel's history (rt_set_temporal_moments; --moments-kmin K: the
//                       frames a pixel needs, default 4).  A history has to exist for that: two helper contexts of the same scene, view and
//                       mode take turns for four frames of two passes each on seed streams of their own, reprojecting with the setting on;
//                       the frame's context then reprojects from the last of them, and the filter runs over ITS TEMPORAL PLANE -- the frame
//                       blended with those eight older passes -- not over its colour plane.  The line gains the setting and the history
//   --shadow-history    shadow-aware history (rt_set_shadow_history; --shadow-keep N: the samples a flagged pixel keeps, default 2).  A moved
//                       sphere has to exist for that: a helper context holds the scene as it was one step earlier -- its last record that is
//                       no light stands two units to the right -- at four passes of a seed stream of its own; the frame's context reprojects
//                       from it with the setting on, and --atrous then filters ITS TEMPORAL PLANE.  A further line gives the setting, the
//                       pairs of rule 29 and the share of pixels flagged.  Not with --moments, --until-psnr, --gpus, --rehearse or --oneshot
//
// The four positional arguments are the reference's; only framework ID 2 (the slot
// Config.cpp:63-65 leaves empty) is served, GPU = 1, memory type 0 (Buffer).
// Prints one JSON line with frame time and ray throughput.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_api.h"

static int die(const char* what) {
    fprintf(stderr, "%s: %s\n", what, rt_last_error());
    return 1;
}

// --moments: four frames of history in two helper contexts taking turns, then `ctx` reprojects from the last of them with the setting on
static int history_moments(rt_ctx* ctx, const rt_sphere* spheres, uint32_t n, const rt_camera& cam, int w, int h, int mode, const rt_moments_params& mp) {
    const int kFrames = 4, kPasses = 2;
    rt_ctx* hist[2] = { nullptr, nullptr };
    for (int k = 0; k < 2; ++k) {
        if (rt_create(&hist[k], w, h) != RT_OK) return die("rt_create");
        if (rt_set_scene(hist[k], spheres, n) != RT_OK) return die("rt_set_scene");
        if (rt_set_camera(hist[k], &cam) != RT_OK) return die("rt_set_camera");
        if (rt_set_mode(hist[k], mode) != RT_OK) return die("rt_set_mode");
        if (rt_set_temporal_moments(hist[k], &mp) != RT_OK) return die("rt_set_temporal_moments");
        if (rt_features_async(hist[k], rt_stream(hist[k])) != RT_OK) return die("rt_features_async");
    }
    for (int f = 0; f < kFrames; ++f) {
        rt_ctx* d = hist[f % 2];
        if (rt_seed_stream_async(d, 100 + (unsigned)f, rt_stream(d)) != RT_OK) return die("rt_seed_stream_async");
        if (rt_render_async(d, kPasses, rt_stream(d)) != RT_OK) return die("rt_render_async");
        if (f > 0 && rt_reproject_async(d, hist[(f - 1) % 2], nullptr, rt_stream(d)) != RT_OK) return die("rt_reproject_async");
    }
    if (rt_set_temporal_moments(ctx, &mp) != RT_OK) return die("rt_set_temporal_moments");
    if (rt_features_async(ctx, rt_stream(ctx)) != RT_OK) return die("rt_features_async");
    if (rt_reproject_async(ctx, hist[(kFrames - 1) % 2], nullptr, rt_stream(ctx)) != RT_OK) return die("rt_reproject_async");
    std::vector<float> m(4 * static_cast<size_t>(w) * h);
    if (rt_read_moments(ctx, m.data()) != RT_OK) return die("rt_read_moments");      // (blocking: the helpers may go)
    size_t reached = 0;
    for (size_t i = 0; i < m.size(); i += 4) reached += m[i + 2] >= mp.k_min;
    printf("{\"moments\": true, \"k_min\": %.3f, \"history_frames\": %d, \"history_passes\": %d, \"pixels_at_k_min\": %.4f}\n", (double)mp.k_min, kFrames, kPasses,
           (double)reached / (double)(m.size() / 4));
    rt_destroy(hist[0]);
    rt_destroy(hist[1]);
    return 0;
}

// --shadow-history: the scene one step earlier in a helper context, then `ctx` reprojects from it with the setting on
static int history_shadow(rt_ctx* ctx, const rt_sphere* spheres, uint32_t n, const rt_camera& cam, int w, int h, int mode, const rt_shadow_history_params& sp) {
    std::vector<rt_sphere> before(spheres, spheres + n);
    int moved = -1;
    for (uint32_t i = 0; i < n; ++i)
        if (spheres[i].rad != 0.0f && spheres[i].rad < 100.0f && spheres[i].e.x == 0.f && spheres[i].e.z == 0.f) moved = (int)i;
    if (moved < 0) {
        fprintf(stderr, "--shadow-history: the scene holds no record to move\n");
        return 1;
    }
    before[(size_t)moved].p.x += 2.0f;
    rt_ctx* was = nullptr;
    if (rt_create(&was, w, h) != RT_OK) return die("rt_create");
    const auto fail = [&](const char* what) {               // the helper goes on every way out
        const int rc = die(what);
        rt_destroy(was);
        return rc;
    };
    if (rt_set_scene(was, before.data(), n) != RT_OK) return fail("rt_set_scene");
    if (rt_set_camera(was, &cam) != RT_OK) return fail("rt_set_camera");
    if (rt_set_mode(was, mode) != RT_OK) return fail("rt_set_mode");
    if (rt_seed_stream_async(was, 100, rt_stream(was)) != RT_OK) return fail("rt_seed_stream_async");
    if (rt_render_async(was, 4, rt_stream(was)) != RT_OK) return fail("rt_render_async");
    if (rt_features_async(was, rt_stream(was)) != RT_OK) return fail("rt_features_async");
    if (rt_set_shadow_history(ctx, &sp) != RT_OK) return fail("rt_set_shadow_history");
    if (rt_features_async(ctx, rt_stream(ctx)) != RT_OK) return fail("rt_features_async");
    if (rt_reproject_async(ctx, was, nullptr, rt_stream(ctx)) != RT_OK) return fail("rt_reproject_async");
    std::vector<uint8_t> k(static_cast<size_t>(w) * h);
    if (rt_read_history_flags(ctx, k.data()) != RT_OK) return fail("rt_read_history_flags");      // (blocking: the helper may go)
    size_t flagged = 0;
    for (uint8_t v : k) flagged += v;
    printf("{\"shadow_history\": true, \"keep\": %.3f, \"moved_record\": %d, \"pairs\": %d, \"pixels_flagged\": %.4f}\n", (double)sp.keep, moved,
           rt_shadow_history_pairs(before.data(), spheres, n, nullptr, 0), (double)flagged / (double)k.size());
    rt_destroy(was);
    return 0;
}

// --atrous: the feature plane, the filter, and the filtered frame's packed words into `px`; prints its line -- with the kernel that formed the plane
// (rt_last_features_kernel: swept, or walked through the hierarchy) and its device time between two events, what the plane cost beside the pass
static int filter_atrous(rt_ctx* ctx, const rt_atrous_params& at, std::vector<uint32_t>& px) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t stream = static_cast<hipStream_t>(rt_stream(ctx));
    struct Events {                                     // (given back on every way out)
        hipEvent_t ev[2] = { nullptr, nullptr };
        ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
        hipEvent_t& operator[](int k) { return ev[k]; }
    } ev;
    float features_ms = 0.f;
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess || hipEventRecord(ev[0], stream) != hipSuccess) return die("hipEventRecord");
    if (rt_features_async(ctx, stream) != RT_OK) return die("rt_features_async");
    if (hipEventRecord(ev[1], stream) != hipSuccess) return die("hipEventRecord");
    if (rt_atrous_async(ctx, &at, stream) != RT_OK) return die("rt_atrous_async");
    if (rt_read_atrous(ctx, nullptr, px.data()) != RT_OK) return die("rt_read_atrous");
    if (hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&features_ms, ev[0], ev[1]) != hipSuccess) return die("hipEventElapsedTime");
    printf("{\"atrous\": true, \"levels\": %d, \"k_lum\": %.3f, \"k_normal\": %.3f, \"features_kernel\": \"%s\", \"features_device_ms\": %.4f, \"atrous_wall_ms\": %.4f}\n",
           at.levels, (double)at.k_lum, (double)at.k_normal, rt_last_features_kernel(ctx), (double)features_ms,
           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

static bool write_ppm(const std::string& path, const std::vector<uint32_t>& px, int w, int h) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    std::vector<unsigned char> row(static_cast<size_t>(w) * 3);
    for (int y = h - 1; y >= 0; --y) {          // buffer row 0 is the bottom of the image
        for (int x = 0; x < w; ++x) {
            uint32_t p = px[static_cast<size_t>(y) * w + x];
            row[3 * x] = p & 255;
            row[3 * x + 1] = (p >> 8) & 255;
            row[3 * x + 2] = (p >> 16) & 255;
        }
        fwrite(row.data(), 1, row.size(), f);
    }
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    int w = 800, h = 600, spp = 1, per_launch = 0, mode = RT_MODE_PARITY, oneshot = 0, gpus = 1, rehearse = 0;
    bool pin = false;
    double readback_ms = 0.0;   // > 0: copy the frame out only when the last copy is this old (the adapter's display cadence)   // SetupGL.cpp:32-33
    bool doubling = true;
    std::string out, scene_path, save_state, load_state;
    unsigned long long seed_stream = 0;
    double until_psnr = 0.0;
    bool until = false;
    int check_every = 8;
    bool adaptive = false;      // --until-psnr per 8x8 tile: rt_render_adaptive instead of rt_render_converged
    int min_passes = 16;
    bool denoise = false;       // --until-psnr: merge into a third context and filter it (rt_denoise_async)
    bool filtered = false;      // --until-psnr judged on the cross-filtered halves: the *_filtered loops, then merge and filter
    bool guided = false;        // --denoise / --filtered under the guide's defaults: feature planes formed, rt_set_denoise_guide on both halves
    bool live_checks = false;   // --filtered --adaptive: rt_render_adaptive_filtered_tiles instead of rt_render_adaptive_filtered
    bool atrous = false;        // --atrous: the frame --out is written from goes through rt_atrous_async first
    rt_denoise_params dn;
    rt_denoise_defaults(&dn);
    rt_atrous_params at;
    rt_atrous_defaults(&at);
    bool moments = false;       // --moments: with --atrous, the variance from a pixel's history (history_moments)
    rt_moments_params mp;
    rt_moments_defaults(&mp);
    bool shadow = false;        // --shadow-history: a moved sphere's shadows end a pixel's history (history_shadow)
    rt_shadow_history_params shp;
    rt_shadow_history_defaults(&shp);
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "--w") w = atoi(next());
        else if (a == "--h") h = atoi(next());
        else if (a == "--spp") spp = atoi(next());
        else if (a == "--passes-per-launch") per_launch = atoi(next());
        else if (a == "--pin") pin = true;
        else if (a == "--readback-ms") readback_ms = atof(next());
        else if (a == "--mode") mode = strcmp(next(), "fast") == 0 ? RT_MODE_FAST : RT_MODE_PARITY;
        else if (a == "--no-doubling") doubling = false;
        else if (a == "--oneshot") oneshot = atoi(next());
        else if (a == "--gpus") gpus = atoi(next());
        else if (a == "--rehearse") rehearse = atoi(next());
        else if (a == "--out") out = next();
        else if (a == "--stream") seed_stream = strtoull(next(), nullptr, 0);
        else if (a == "--save-state") save_state = next();
        else if (a == "--load-state") load_state = next();
        else if (a == "--until-psnr") { until_psnr = atof(next()); until = true; }
        else if (a == "--check-every") check_every = atoi(next());
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--min-passes") min_passes = atoi(next());
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-radius") dn.search_radius = atoi(next());
        else if (a == "--filtered") filtered = denoise = true;
        else if (a == "--guided") guided = true;
        else if (a == "--live-checks") live_checks = true;
        else if (a == "--atrous") atrous = true;
        else if (a == "--atrous-levels") at.levels = atoi(next());
        else if (a == "--moments") moments = true;
        else if (a == "--moments-kmin") mp.k_min = (float)atof(next());
        else if (a == "--shadow-history") shadow = true;
        else if (a == "--shadow-keep") shp.keep = (float)atof(next());
        else pos.push_back(argv[i]);
    }
    if (!pos.empty() && atoi(pos[0]) != 2) {
        fprintf(stderr, "Unsupported Framework Type (this host serves framework ID 2 = HIP)\n");
        return 1;
    }
    if (pos.size() >= 3 && atoi(pos[2]) != 0) {
        fprintf(stderr, "Unsupported Memory Type\n");
        return 1;
    }
    if (pos.size() >= 4) scene_path = pos[3];
    if (denoise && !until) {
        fprintf(stderr, "--denoise filters the merge of two halves: it needs --until-psnr\n");
        return 1;
    }
    if (guided && !denoise) {
        fprintf(stderr, "--guided guides a filter: it needs --denoise or --filtered\n");
        return 1;
    }
    if (live_checks && !(until && filtered && adaptive)) {
        fprintf(stderr, "--live-checks is a form of the filtered adaptive loop: it needs --until-psnr DB --filtered --adaptive\n");
        return 1;
    }
    if (moments && !atrous) {
        fprintf(stderr, "--moments steers the wavelet filter: it needs --atrous\n");
        return 1;
    }
    if (shadow && (moments || until || gpus > 1 || rehearse > 0 || oneshot > 0)) {
        fprintf(stderr, "--shadow-history reprojects into the frame's one context: not with --moments, --until-psnr, --gpus, --rehearse or --oneshot\n");
        return 1;
    }
    if (atrous && (gpus > 1 || rehearse > 0 || oneshot > 0)) {
        fprintf(stderr, "--atrous filters the frame of one context on one device: not with --gpus, --rehearse or --oneshot\n");
        return 1;
    }

    std::vector<rt_sphere> spheres(16384);
    uint32_t n = 0;
    rt_camera cam{};
    if (!scene_path.empty()) {
        if (rt_read_scene(scene_path.c_str(), spheres.data(), (uint32_t)spheres.size(), &n, &cam.orig,
                          &cam.target, doubling ? 1 : 0) != RT_OK)
            return die("readScene");
    } else {                                        // Main.cpp:80-86
        n = (uint32_t)rt_demo_scene(spheres.data(), (uint32_t)spheres.size());
        cam.orig = rt_vec3{ 20.f, 100.f, 120.f };
        cam.target = rt_vec3{ 0.f, 25.f, 0.f };
    }
    rt_compute_camera(&cam, w, h);

    if (oneshot > 0) {                               // the one call north_star names, as a host would use it per frame
        std::vector<uint32_t> px1(static_cast<size_t>(w) * h);
        const rt_scene scene{ spheres.data(), n };
        printf("{\"rt_render_wall_ms\": [");
        for (int k = 0; k < oneshot; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if (rt_render(&scene, &cam, px1.data(), w, h, spp) != RT_OK) return die("rt_render");
            printf("%s%.3f", k ? ", " : "", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        printf("], \"w\": %d, \"h\": %d, \"spp\": %d, \"spheres\": %u}\n", w, h, spp, n);
        if (!out.empty() && !write_ppm(out, px1, w, h)) fprintf(stderr, "cannot write %s\n", out.c_str());
        rt_release_cache();
        return 0;
    }

    if (until) {                                     // two halves on streams of their own, rendered until they agree, then merged
        rt_ctx* half[2] = { nullptr, nullptr };
        for (int k = 0; k < 2; ++k) {
            if (rt_create(&half[k], w, h) != RT_OK) return die("rt_create");
            if (rt_set_scene(half[k], spheres.data(), n) != RT_OK) return die("rt_set_scene");
            if (rt_set_camera(half[k], &cam) != RT_OK) return die("rt_set_camera");
            if (rt_set_mode(half[k], mode) != RT_OK) return die("rt_set_mode");
            if (rt_seed_stream_async(half[k], 1 + (unsigned)k, rt_stream(half[k])) != RT_OK) return die("rt_seed_stream_async");
            if (guided) {
                rt_guide_params guide;
                rt_guide_defaults(&guide);
                if (rt_set_denoise_guide(half[k], &guide) != RT_OK) return die("rt_set_denoise_guide");
                if (rt_features_async(half[k], rt_stream(half[k])) != RT_OK) return die("rt_features_async");
            }
        }
        rt_frame_error err{};
        int checks = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const int reached = filtered ? (adaptive ? (live_checks ? rt_render_adaptive_filtered_tiles : rt_render_adaptive_filtered)(half[0], half[1], until_psnr, min_passes, check_every, spp, &dn, &err, &checks)
                                                 : rt_render_converged_filtered(half[0], half[1], until_psnr, check_every, spp, &dn, &err, &checks))
                                     : (adaptive ? rt_render_adaptive(half[0], half[1], until_psnr, min_passes, check_every, spp, &err, &checks)
                                                 : rt_render_converged(half[0], half[1], until_psnr, check_every, spp, &err, &checks));
        if (reached < 0) return die(adaptive ? "rt_render_adaptive(_filtered)" : "rt_render_converged(_filtered)");
        const int per_half = rt_current_sample(half[0]);
        // adaptive: what was rendered against what whole frames to that pass number would have been, and the sample map
        rt_stats st_half[2];
        std::vector<uint32_t> tile_passes((size_t)rt_compare_tiles(half[0], nullptr, nullptr));
        if (adaptive) {
            for (int k = 0; k < 2; ++k)
                if (rt_get_stats(half[k], &st_half[k]) != RT_OK) return die("rt_get_stats");
            if (rt_tile_passes(half[0], tile_passes.data()) != RT_OK) return die("rt_tile_passes");
            std::sort(tile_passes.begin(), tile_passes.end());
        }
        rt_ctx* frame = half[0];                     // the context --out is written from: the first half, or with --denoise a third one
        double denoise_ms = 0.0;
        std::vector<uint32_t> merged(static_cast<size_t>(w) * h);
        if (denoise) {                               // the halves stay as they are: the filter reads them
            if (rt_create(&frame, w, h) != RT_OK) return die("rt_create");
            if (rt_set_scene(frame, spheres.data(), n) != RT_OK) return die("rt_set_scene");
            if (rt_set_camera(frame, &cam) != RT_OK) return die("rt_set_camera");
            if (rt_set_mode(frame, mode) != RT_OK) return die("rt_set_mode");
            if (rt_merge_async(frame, half, 2, rt_stream(frame)) != RT_OK) return die("rt_merge_async");
            if (rt_read_pixels(frame, merged.data()) != RT_OK) return die("rt_read_pixels");   // (the merge has finished: the filter is timed alone)
            const auto d0 = std::chrono::steady_clock::now();
            if (rt_denoise_async(frame, half[0], half[1], &dn, rt_stream(frame)) != RT_OK) return die("rt_denoise_async");
            if (rt_read_pixels(frame, merged.data()) != RT_OK) return die("rt_read_pixels");
            denoise_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - d0).count();
        } else if (rt_merge_async(half[0], &half[1], 1, rt_stream(half[0])) != RT_OK) {
            return die("rt_merge_async");
        }
        if (!denoise && rt_read_pixels(frame, merged.data()) != RT_OK) return die("rt_read_pixels");
        const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (moments && history_moments(frame, spheres.data(), n, cam, w, h, mode, mp) != 0) return 1;
        if (atrous && filter_atrous(frame, at, merged) != 0) return 1;
        if (!out.empty() && !write_ppm(out, merged, w, h)) fprintf(stderr, "cannot write %s\n", out.c_str());
        printf("{\"spheres\": %u, \"w\": %d, \"h\": %d, \"until_psnr\": %.3f, \"reached\": %s, \"passes_per_half\": %d, \"merged_passes\": %d, "
               "\"checks\": %d, \"check_every\": %d, \"%s\": %.3f, \"differing\": %llu, \"max_abs\": %u, \"wall_ms\": %.4f}\n",
               n, w, h, until_psnr, reached ? "true" : "false", per_half, rt_current_sample(frame), checks, check_every,
               filtered ? "cross_filtered_pair_psnr_db" : "pair_psnr_db", rt_error_psnr(&err),
               (unsigned long long)err.differing, err.max_abs, wall_ms);
        if (adaptive)
            printf("{\"adaptive\": true, \"min_passes\": %d, \"checks\": %d, \"samples_rendered\": %llu, \"samples_of_whole_frames\": %llu, "
                   "\"tile_passes_min\": %u, \"tile_passes_median\": %u, \"tile_passes_max\": %u}\n",
                   min_passes, checks, (unsigned long long)(st_half[0].samples + st_half[1].samples), 2ull * (unsigned long long)w * h * per_half,
                   tile_passes.front(), tile_passes[tile_passes.size() / 2], tile_passes.back());
        if (denoise) {
            printf("{\"denoise\": true, \"guided\": %s, \"search_radius\": %d, \"patch_radius\": %d, \"alpha\": %.3f, \"k\": %.3f, \"denoise_wall_ms\": %.4f}\n",
                   guided ? "true" : "false", dn.search_radius, dn.patch_radius, (double)dn.alpha, (double)dn.k, denoise_ms);
            rt_destroy(frame);
        }
        rt_destroy(half[0]);
        rt_destroy(half[1]);
        return 0;
    }

    rt_ctx* ctx = nullptr;
    if (rehearse > 0) {
        std::vector<int> dev(static_cast<size_t>(rehearse), 0);
        if (rt_create_multi_on(&ctx, w, h, dev.data(), rehearse, 8) != RT_OK) return die("rt_create_multi_on");
    } else if ((gpus > 1 ? rt_create_multi(&ctx, w, h, gpus) : rt_create(&ctx, w, h)) != RT_OK) {
        return die("rt_create");
    }
    if (rt_set_scene(ctx, spheres.data(), n) != RT_OK) return die("rt_set_scene");
    if (rt_set_camera(ctx, &cam) != RT_OK) return die("rt_set_camera");
    if (rt_set_mode(ctx, mode) != RT_OK) return die("rt_set_mode");
    if (seed_stream != 0 && rt_seed_stream_async(ctx, seed_stream, rt_stream(ctx)) != RT_OK) return die("rt_seed_stream_async");
    if (!load_state.empty() && rt_load_state(ctx, load_state.c_str()) != RT_OK) return die("rt_load_state");     // (its seeds replace the stream's)
    const int first_pass = rt_current_sample(ctx);

    std::vector<uint32_t> px(static_cast<size_t>(w) * h);
    if (per_launch <= 0) per_launch = spp;
    if (pin && rt_pin_output(ctx, px.data(), px.size()) != RT_OK) return die("rt_pin_output");
    auto t0 = std::chrono::steady_clock::now();
    auto last_copy = t0;
    double kernel_ms = 0.0;
    for (int done = 0; done < spp;) {
        int k = (spp - done < per_launch) ? spp - done : per_launch;
        const auto now = std::chrono::steady_clock::now();
        const bool last = done + k >= spp;
        const bool due = done == 0 || last || readback_ms <= 0.0 ||
                         std::chrono::duration<double, std::milli>(now - last_copy).count() >= readback_ms;
        if (readback_ms > 0.0) rt_set_pixel_write(ctx, due ? 1 : 0);
        if ((due ? rt_render_pass(ctx, px.data(), k) : rt_render_async(ctx, k, rt_stream(ctx))) != RT_OK)
            return die("rt_render_pass");
        if (due) {                       // (launches queued between two copies are not timed one by one)
            last_copy = now;
            rt_stats st;
            rt_get_stats(ctx, &st);
            kernel_ms += st.last_kernel_ms;
        }
        done += k;
    }
    double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    rt_stats st;
    if (rt_get_stats(ctx, &st) != RT_OK) return die("rt_get_stats");
    if (moments && history_moments(ctx, spheres.data(), n, cam, w, h, mode, mp) != 0) return 1;
    if (shadow && history_shadow(ctx, spheres.data(), n, cam, w, h, mode, shp) != 0) return 1;
    if (atrous && filter_atrous(ctx, at, px) != 0) return 1;
    if (!out.empty() && !write_ppm(out, px, w, h)) fprintf(stderr, "cannot write %s\n", out.c_str());
    if (!save_state.empty() && rt_save_state(ctx, save_state.c_str()) != RT_OK) return die("rt_save_state");

    const double rays = (double)(st.samples + st.shadow_rays);
    printf("{\"spheres\": %u, \"w\": %d, \"h\": %d, \"spp\": %d, \"first_pass\": %d, \"seed_stream\": %llu, \"launches\": %llu, \"kernel_ms\": %.4f, "
           "\"wall_ms_with_readback\": %.4f, \"samples\": %llu, \"closest_rays\": %llu, \"shadow_rays\": %llu, "
           "\"sphere_tests\": %llu, \"Mray_s_primary_shadow\": %.1f, \"Msample_s\": %.1f}\n",
           n, w, h, spp, first_pass, seed_stream, (unsigned long long)st.launches, kernel_ms, wall_ms, (unsigned long long)st.samples,
           (unsigned long long)st.closest_rays, (unsigned long long)st.shadow_rays,
           (unsigned long long)st.sphere_tests, rays / (kernel_ms * 1e3), (double)st.samples / (kernel_ms * 1e3));
    rt_destroy(ctx);
    return 0;
}
