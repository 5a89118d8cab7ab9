// rt_launch.hip -- what one launch of the render kernel is made of: which kernel instance (rt_device.h Instance: arithmetic mode x
// role x workgroup shape), its tables and LDS, the scheduling data it runs with (heavy-first tile order) and, for scenes
// that have a hierarchy, whether it is walked or the plain sweep runs -- settled by a
// surface-area estimate at rt_set_scene, by measurement inside the estimate's band.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_internal.h"

#ifndef RT_DIAGNOSTICS
#define RT_DIAGNOSTICS 0
#endif

using rt::fail;

// Heavy-first order of the tiles from the costs the last launch left (rt_trace.inc.h): ONE workgroup; a counting sort over
// 1024 cost classes (largest first; the order inside a class does not matter).
__global__ void __launch_bounds__(1024) rt_order_tiles_kernel(const uint32_t *cost, uint32_t *order, uint32_t n) {
    __shared__ unsigned s_max;
    __shared__ unsigned s_hist[1024];
    const unsigned tid = threadIdx.x;
    constexpr unsigned kCap = 0x1FFFFFu;            // 21 ms of ticks: cost * 1023 stays inside 32 bits
    auto key_of = [&](uint32_t i) -> unsigned { return cost[i] < kCap ? cost[i] : kCap; };
    if (tid == 0) s_max = 1u;
    s_hist[tid] = 0u;
    __syncthreads();
    unsigned m = 0;
    for (uint32_t i = tid; i < n; i += 1024) {
        const unsigned c_ = key_of(i);
        m = c_ > m ? c_ : m;
    }
    atomicMax(&s_max, m);
    __syncthreads();
    const unsigned top = s_max;
    for (uint32_t i = tid; i < n; i += 1024) atomicAdd(&s_hist[1023u - key_of(i) * 1023u / top], 1u);
    __syncthreads();
    if (tid == 0) {                     // exclusive prefix over the classes, most expensive class first
        unsigned run = 0;
        for (int k = 0; k < 1024; ++k) {
            const unsigned c_ = s_hist[k];
            s_hist[k] = run;
            run += c_;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024) order[atomicAdd(&s_hist[1023u - key_of(i) * 1023u / top], 1u)] = i;
}

namespace rt {

rt::LaunchParams make_params(rt_ctx *c, int n_samples) {
    rt::LaunchParams p{};
    p.scene = c->scene;
    p.cam = c->cam;
    p.seeds = c->d_seeds;
    p.seeds_in = c->frame.seeds_default ? c->d_seeds0 : c->d_seeds;
    p.colors = c->d_colors;
    p.pixels = frame_pixels(c);
    p.counters = c->d_counters;
    p.stats = c->d_stats;
    p.w = c->w;
    p.h = c->h;
    p.first_sample = c->frame.current_sample;
    p.n_samples = n_samples;
    p.rank = c->rank;
    p.nranks = c->nranks;
    p.tile_rows = c->tile_rows;
    p.local_rows = c->local_rows;
    p.skip_pixels = c->pixel_write ? 0 : 1;
    p.inv_w = 1.f / (float)c->w;          // correctly rounded on the host as on the device (-ffp-contract=off, IEEE division)
    p.inv_h = 1.f / (float)c->h;
    p.regen_gate = c->regen_gate > 0 ? c->regen_gate : (c->scene.n_spheres <= 512 ? 8 : 1);
    p.coop_kmax = c->coop_kmax;
    p.direct_max = c->direct_max;
    p.tiles_x = (int)tiles_per_row(c);
    p.n_tiles = (int)tile_count(c);
    return p;
}


// ---- which instance, and what it needs (rt_device.h Instance; the rows live next to the instantiations) ----

const rt::Instance *instances(bool fast, int *count) { return fast ? rt::fast_instances(count) : rt::parity_instances(count); }

// the row with this role and workgroup shape (null: this library has none)
static const rt::Instance *find_role(bool fast, int role, int waves) {
    int n = 0;
    const rt::Instance *t = instances(fast, &n);
    for (int k = 0; k < n; ++k)
        if (t[k].role == role && t[k].waves == waves) return &t[k];
    return nullptr;
}

// LDS the hierarchy's staged tables take for this scene
static size_t pairs_lds(const rt_ctx *c, bool mat, int n_samples, int waves = 4) {
    return rt::lds_bytes_pairs(c->scene.n_spheres, c->scene.n_lights, mat, n_samples, c->bvh.n_leaves, c->bvh.n_slots, c->bvh.stack_depth, 64 * waves);
}

// the plain sweep's tables (geometry and lights) fit LDS for this launch
bool tables_fit_lds(const rt_ctx *c, int n_samples) {
    return rt::lds_bytes(c->scene.n_spheres, c->scene.n_lights, false, n_samples) <= kLdsMax;
}
// ... and are staged there: while at least four workgroups of that size fit a CU.  Larger tables go through the scalar cache (rt_trace_*_g), which
// keeps six wavefronts per SIMD at any size: a sweep over 96 KB of staged tables runs ONE workgroup per CU and takes five times as long (rt_internal.h)
static bool sweep_stages_tables(const rt_ctx *c, int n_samples) {
    return rt::lds_bytes(c->scene.n_spheres, c->scene.n_lights, false, n_samples) <= (size_t)(c->sweep_lds_limit < (int)kLdsMax ? c->sweep_lds_limit : (int)kLdsMax);
}

// the hierarchy's tables fit the LDS budget given to them; otherwise the walk reads them from HBM / L2
static bool bvh_fits_lds(const rt_ctx *c, int n_samples) { return pairs_lds(c, false, n_samples) <= (size_t)c->bvh_lds_limit; }
// ... or at least its PAIRS do (header | pairs | stacks): the chain of dependent fetches a walk consists of then stays in LDS
static size_t pairs_only_lds(const rt_ctx *c, int n_samples, int waves = 4) {
    return rt::lds_bytes_pairs(0, 0, false, n_samples, c->bvh.n_leaves, 0, c->bvh.stack_depth, 64 * waves);
}
static bool bvh_pairs_fit_lds(const rt_ctx *c, int n_samples) { return c->bvh_mixed != 0 && pairs_only_lds(c, n_samples) <= (size_t)c->bvh_lds_limit; }

// the scene has a hierarchy and the context may use it
static bool bvh_usable(const rt_ctx *c) { return c->bvh_ok && c->wg_waves != 1 && c->persist == 0; }

// What the instance needs from the context, checked against what the context has: the ONE place that sizes the
// dynamic LDS and hands out the hierarchy.  An instance whose tables the context lacks is refused (RT_ERR_STATE),
// whatever route selected it -- the measured choice, a forced form, or a diagnostics mode.
static int bind_tables(rt_ctx *c, const rt::Instance &inst, int n_samples, rt::LaunchParams &p, size_t *lds_out) {
    p.bvh = rt::BvhTables{};
    if (rt::walks_hierarchy(inst.tables)) {
        if (!c->bvh_ok || !c->bvh.blob)
            return fail(RT_ERR_STATE, "%s walks a hierarchy and the scene has none (fewer than %d small spheres?)", inst.name, c->bvh_min);
        p.bvh = c->bvh;
    }
    size_t lds = 0;
    switch (inst.tables) {
        case rt::kTabSweepLds:
            lds = rt::lds_bytes(c->scene.n_spheres, c->scene.n_lights, p.mat_in_lds != 0, n_samples);
            break;
        case rt::kTabSweepGlobal:
            p.mat_in_lds = 0;
            lds = rt::lds_bytes(0, 0, false, n_samples);
            break;
        case rt::kTabPairsLds:
            p.mat_in_lds = 0;               // (the walk reads a hit's material by slot from the hierarchy's blob: nothing of it is staged)
            lds = pairs_lds(c, false, n_samples, inst.waves * ((inst.flags & rt::kInstTwoRays) ? 2 : 1));
            break;
        case rt::kTabPairsGlobal:
            p.mat_in_lds = 0;
            lds = rt::lds_bytes_pairs(0, 0, false, n_samples, 1, 0, c->bvh.stack_depth, 64 * inst.waves);
            break;
        case rt::kTabPairsLdsSlotsGlobal:
            p.mat_in_lds = 0;
            lds = pairs_only_lds(c, n_samples, inst.waves);
            break;
        case rt::kTabPairsPacked:           // header | the packed table's frame | stacks
            if (c->bvh.packed_at == 0 && c->bvh.n_leaves >= 2)      // (a tree of one leaf has no pairs: the walk starts at the leaf and the frame is never used)
                return fail(RT_ERR_STATE, "%s reads the packed pair table and this scene's hierarchy has none", inst.name);
            p.mat_in_lds = 0;
            lds = rt::lds_bytes_pairs(0, 0, false, n_samples, 1, 0, c->bvh.stack_depth, 64 * inst.waves) + 32;
            break;
        case rt::kTabPairsTopLds:           // header | the promoted top of the tree (n_top pairs = "n_top + 1 leaves") | stacks
            if (c->bvh.n_top == 0 && c->bvh.n_leaves >= 2)          // (without a promoted top the root is not pair 0: rt_debug_set_bvh_layout asks for one)
                return fail(RT_ERR_STATE, "%s stages the promoted top of the tree and this scene's hierarchy has none", inst.name);
            p.mat_in_lds = 0;
            lds = rt::lds_bytes_pairs(0, 0, false, n_samples, c->bvh.n_top + 1, 0, c->bvh.stack_depth, 64 * inst.waves);
            break;
        default:
            return fail(RT_ERR_STATE, "%s: unknown table kind %d", inst.name, inst.tables);
    }
#if RT_DIAGNOSTICS
    if (const char *pad = getenv("RT_LDS_PAD")) lds += (size_t)atoi(pad);       // occupancy experiments: fewer workgroups per CU
#endif
    if (lds > kLdsMax) return fail(RT_ERR_ARG, "%s needs %zu B of LDS for this scene (limit %zu)", inst.name, lds, kLdsMax);
    *lds_out = lds;
    return RT_OK;
}

// Which instance renders a launch of `form`, and the launch parameters that go with the choice.  Reads the context, changes nothing, calls nothing of HIP.
struct Chosen { const rt::Instance *inst = nullptr; int mat_in_lds = 0, regen_gate = 0; };      // (regen_gate 0: the context's, make_params)
static int choose_instance(const rt_ctx *c, int n_samples, Form form, Chosen *out) {
    const size_t lds_all = rt::lds_bytes(c->scene.n_spheres, c->scene.n_lights, true, n_samples);
    // materials ride along in LDS only while that keeps at least 6 workgroups per CU resident
    // (160 KiB / 24 KiB); larger scenes read them from L2 once per hit
    out->mat_in_lds = lds_all <= (size_t)c->mat_lds_limit;
    const size_t lds_sweep = rt::lds_bytes(c->scene.n_spheres, c->scene.n_lights, out->mat_in_lds != 0, n_samples);

    // which instance: arithmetic mode x role x workgroup shape.  Single-wavefront workgroups (8x8 tiles) keep the wave
    // slots of a CU full (a 4-wavefront workgroup waits for four free slots at once) and give the heavy-first order a
    // finer granule; each stages its own copy of the tables, so only while 24 copies fit a CU.
    bool fast = c->mode == RT_MODE_FAST;
    const bool coop = form == Form::SweepCoop ? true : (form == Form::SweepPlain ? false : (c->coop_min > 0 && c->scene.n_spheres >= (uint32_t)c->coop_min));
    const bool w1 = c->wg_waves == 1 || (c->wg_waves == 0 && lds_sweep + (coop ? 1536u : 256u) <= 6 * 1024);   // + the instance's static LDS
    int role = coop ? rt::kRoleCoop : rt::kRolePlain, waves = w1 ? 1 : 4;
    if (!sweeps(form) && bvh_usable(c)) {
        // large scenes: the walk over the hierarchy, from LDS while its tables leave room for five workgroups per CU
        role = bvh_fits_lds(c, n_samples) ? rt::kRolePairs : (bvh_pairs_fit_lds(c, n_samples) ? rt::kRolePairsMixed : rt::kRolePairsGlobal);
        waves = 4;
        if (c->regen_gate <= 0) out->regen_gate = c->walk_gate;
    } else if (!sweep_stages_tables(c, n_samples)) {
        // no hierarchy (or it lost the measurement) and a table beyond the sweep's LDS budget: the plain sweep over the table in HBM / L2
        role = rt::kRoleSweepGlobal;
        waves = 4;
    }
    const rt::Instance *inst = nullptr;
#if RT_DIAGNOSTICS
    if (c->persist != 0 && c->mode < 100) {
        role = coop ? rt::kRolePersistCoop : rt::kRolePersist;
        waves = 4;
    } else if (c->mode >= 100) {           // a row of the table by number (rt_set_mode checked the range)
        fast = c->mode >= 200;
        int n = 0;
        const rt::Instance *t = instances(fast, &n);
        inst = &t[c->mode - (fast ? 200 : 100)];
    }
#endif
    if (!inst) inst = find_role(fast, role, waves);
    // (the product library ships no 4-wavefront PLAIN sweep: below 12 spheres the tables always fit the single-wavefront budget above; should a
    // launch get here all the same, the cooperative instance of that shape renders any scene -- same bits, it only shares its shadow sweeps)
    if (!inst && role == rt::kRolePlain) inst = find_role(fast, rt::kRoleCoop, waves);
    if (!inst) return fail(RT_ERR_STATE, "this library holds no %s instance of role %d with %d wavefronts per workgroup", fast ? "fast" : "parity", role, waves);
    out->inst = inst;
    return RT_OK;
}

// What launch_form and launch_tiles refuse alike ...
static int check_launch_args(const rt_ctx *c, int n_samples) {
    if (!c->have_scene || !c->have_cam) return fail(RT_ERR_STATE, "rt_set_scene and rt_set_camera must precede rendering");
    if (n_samples < 0) return fail(RT_ERR_ARG, "n_samples < 0");
    if (n_samples > 0x7fffffff - c->frame.current_sample)
        return fail(RT_ERR_ARG, "pass counter would overflow (%d + %d)", c->frame.current_sample, n_samples);
    return RT_OK;
}

// ... and what both make of `form` once something is to be launched: the instance, its parameters, its tables and its LDS.  `from_list`: the launch
// takes its tiles from a subset launch's list, which an instance of a wider tile, or one that walks no list at all, cannot render.
struct Prepared { const rt::Instance *inst = nullptr; rt::LaunchParams p{}; size_t lds = 0; };
static int prepare_launch(rt_ctx *c, int n_samples, Form form, bool from_list, Prepared *out) {
    Chosen chosen;
    int rc = choose_instance(c, n_samples, form, &chosen);
    if (rc != RT_OK) return rc;
    const rt::Instance *inst = out->inst = chosen.inst;
    if (from_list && ((inst->flags & (rt::kInstTwoRays | rt::kInstPersistent | rt::kInstNoTileCost)) != 0 || (inst->waves != 1 && inst->waves != 4)))
        return fail(RT_ERR_STATE, "rt_render_tiles_async: %s does not render a 32x8 group from a tile list (a wider tile, or no list at all)", inst->name);
    out->p = make_params(c, n_samples);
    out->p.mat_in_lds = chosen.mat_in_lds;
    if (chosen.regen_gate) out->p.regen_gate = chosen.regen_gate;
    out->p.walk_round = (c->walk_round & 0xff) | (c->walk_tail << 8);       // (one kernel argument: pair steps in a row | tail lanes << 8)
    return bind_tables(c, *inst, n_samples, out->p, &out->lds);
}

// The launch is queued: the frame has its passes, and the form choice knows what rendered them
static void after_launch(rt_ctx *c, const rt::Instance &inst, int n_samples, const bool *all_groups) {
    if (all_groups) c->frame.launched_subset(n_samples, c->pixel_write != 0, *all_groups);
    else c->frame.launched(n_samples, c->pixel_write != 0);
    c->choice.scene_launches += 1;
    c->last_kernel = inst.name;
    const bool coop = inst.role == rt::kRoleCoop || inst.role == rt::kRolePersistCoop;
    c->choice.last = rt::walks_hierarchy(inst.tables) ? Form::Walk : (coop ? Form::SweepCoop : Form::SweepPlain);
}

// persistent instances: just enough workgroups to fill the machine; the tile queue (counters[30]) does the rest
static int persist_grid(rt_ctx *c, int n_tiles, size_t lds_use, hipStream_t stream, dim3 *grid) {
    size_t per_cu = lds_use > 0 ? (160 * 1024) / (lds_use + 6 * 1024) : 6;
    if (per_cu > 6) per_cu = 6;
    if (per_cu < 1) per_cu = 1;
    size_t blocks = (size_t)c->n_cus * per_cu;
    const size_t needed = ((size_t)n_tiles + 3) / 4;
    if (blocks > needed) blocks = needed;
    *grid = dim3((unsigned)blocks, 1, 1);
    HIP_TRY(hipMemsetAsync(c->d_counters + 30, 0, sizeof(unsigned long long), stream));
    return RT_OK;
}

// One launch of `form` (Form::Auto: whatever the context's thresholds and diagnostics knobs say).  `natural_order`: in image order whatever the
// tile schedule holds (rt_tile_order.h) -- the hierarchy's probe only.
static int launch_form(rt_ctx *c, int n_samples, hipStream_t stream, Form form, bool natural_order = false) {
    int rc = check_launch_args(c, n_samples);
    if (rc != RT_OK || n_samples == 0 || c->local_rows == 0) return rc;
    rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    Prepared prep;
    rc = prepare_launch(c, n_samples, form, false, &prep);
    if (rc != RT_OK) return rc;
    const rt::Instance *inst = prep.inst;
    rt::LaunchParams &p = prep.p;
    const size_t lds_use = prep.lds;

    const int tile_w = 8 * inst->waves * ((inst->flags & rt::kInstTwoRays) ? 2 : 1);
    dim3 grid((unsigned)((c->w + tile_w - 1) / tile_w), tile_row_count(c));
    const uint32_t n_tiles = grid.x * grid.y;
    const rt::TileOrder::Plan plan = c->order.plan(n_tiles, n_samples, natural_order, (inst->flags & rt::kInstNoTileCost) == 0);
    if (plan.sort_now) {
        hipLaunchKernelGGL(rt_order_tiles_kernel, dim3(1), dim3(1024), 0, stream, c->order.d_tile_cost, c->order.d_order, n_tiles);
        if (hipPeekAtLastError() != hipSuccess) c->order.forget();      // (no order from a sort that was not queued)
        HIP_TRY(hipGetLastError());
        c->frame.order_resorted();                                      // (a subset launch's list follows the order: launch_tiles builds it again)
    }
    if (plan.use_order) p.order = c->order.d_order;
    if (plan.write_costs) p.tile_cost = c->order.d_tile_cost;
    if (plan.accumulate) p.skip_pixels |= 2;
    if (inst->flags & rt::kInstPersistent) {
        rc = persist_grid(c, p.n_tiles, lds_use, stream, &grid);
        if (rc != RT_OK) return rc;
    }
#if RT_DIAGNOSTICS
    if (inst->role == rt::kRoleTimelog && c->d_timelog && c->timelog_used < c->timelog_cap) {
        p.timelog = c->d_timelog;
        p.seq = c->timelog_used++;
        p.tl_tag = c->timelog_tag;
        p.wavelog = ((size_t)grid.x * grid.y * 4 <= c->wavelog_cap) ? c->d_wavelog : nullptr;
    }
#endif
    const hipError_t e = rt::launch_instance(*inst, p, grid, lds_use, stream);
    if (e != hipSuccess)
        return fail(RT_ERR_HIP, "kernel launch failed: %s (%s, grid %ux%u, lds %zu B)", hipGetErrorString(e), inst->name, grid.x, grid.y, lds_use);
    c->order.launched(plan, n_samples, n_tiles);
    after_launch(c, *inst, n_samples, nullptr);
    return RT_OK;
}

// rt_render_tiles_async: n_samples passes on the groups rt_select_tiles selected, and on nothing else (rt_tiles.hip).  The render kernels take their
// tile from LaunchParams::order, so the launch is a list of the selected groups' tiles and a grid just large enough for it: (tiles_x, ceil(m / tiles_x))
// -- grid.x stays the instance's tiles per row, because the kernels form tile_by and tile_bx with gridDim.x -- the list padded to whole grid rows with
// the SENTINEL id tiles_x * tiles_y.  A workgroup that draws the sentinel has tile_by = tiles_y, so lrow >= local_rows in every lane: no lane is valid,
// nothing is loaded or stored, zeros are added to the counters, and with tile_cost null there is no other store (rt_trace.inc.h, rt_walk.inc.h: the
// `valid` / `valid_e` tests and the epilogue).  The instance is the one the context's last launch used (choice.last; before any launch what the thresholds
// say); no probe is started, advanced or timed, and the heavy-first schedule is read, never written: no plan(), no launched(), no costs.
int launch_tiles(rt_ctx *c, int n_samples, hipStream_t stream) {
    int rc = check_launch_args(c, n_samples);
    if (rc != RT_OK) return rc;
    const rt::FrameState &frame = c->frame;
    if (!frame.have_selection) return fail(RT_ERR_STATE, "rt_render_tiles_async: no selection (rt_select_tiles comes first; a reset drops it)");
    if (n_samples == 0 || frame.counts[0] == 0) return RT_OK;
    if (c->tables_stale) {
        rc = refresh_tables(c, stream);
        if (rc != RT_OK) return rc;
    }
    rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    Prepared prep;
    rc = prepare_launch(c, n_samples, c->choice.last, true, &prep);
    if (rc != RT_OK) return rc;
    const rt::Instance *inst = prep.inst;
    rt::LaunchParams &p = prep.p;
    const size_t lds_use = prep.lds;

    const uint32_t tiles_x = (uint32_t)((c->w + 8 * inst->waves - 1) / (8 * inst->waves)), tiles_y = tile_row_count(c);
    const uint32_t n_launch = tiles_x * tiles_y;
    const uint32_t m = inst->waves == 4 ? frame.counts[0] : frame.counts[1];       // launch tiles kept: a group is one 32x8 tile, or the 8x8 tiles it covers
    dim3 grid(tiles_x, (m + tiles_x - 1) / tiles_x);
    const bool by_order = c->order.use_order != 0 && c->order.has_order() && c->order.cost_tiles == n_launch;      // a schedule sorted for this tile shape
    if (frame.list_is_stale(by_order, n_launch)) {
        rc = tiles_build_list(c, inst->waves, by_order, n_launch, grid.x * grid.y, stream);
        if (rc != RT_OK) return rc;
    }
    const bool all = frame.counts[0] == group_count(c);       // every group selected means every group at the front: the frame stays (or is again) whole
    if (frame.seeds_default && !all) {
        // after rt_reset_async the first launch reads the pristine stream in place and writes the context's buffer; the tiles this launch leaves out
        // must hold that stream too (a tile at 0 passes holds the seeds of a 0-pass render): the copy rt_reset makes, now
        HIP_TRY(hipMemcpyAsync(c->d_seeds, c->d_seeds0, 2 * image_pixels(c) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        c->frame.default_seeds_copied();
        p.seeds_in = c->d_seeds;
    }
    p.order = c->tiles.d_list;
    p.tile_cost = nullptr;
    const hipError_t e = rt::launch_instance(*inst, p, grid, lds_use, stream);
    if (e != hipSuccess)
        return fail(RT_ERR_HIP, "kernel launch failed: %s (%s, grid %ux%u, lds %zu B)", hipGetErrorString(e), inst->name, grid.x, grid.y, lds_use);
    if (!all) {
        rc = tiles_advance(c, n_samples, stream);           // (reads current_sample as it was: the count the selected groups come from)
        if (rc != RT_OK) return rc;
    }
    // (a timed step of the cooperative-or-plain measurement that is open lies between an event and the full launches still to come: this launch
    // would be timed with them, so the step starts again with the next full launch -- nothing of the measurement is started, advanced or timed here)
    if ((c->probe.state & 1) != 0 && c->probe.acc > 0) c->probe.acc = 0;
    after_launch(c, *inst, n_samples, &all);
    return RT_OK;
}

// A long launch that would walk its tiles in image order although their costs can be had -- the first frame of a scene --
// renders 4 of its passes first (they are passes of the frame like any other: progressive launches equal one launch bit for bit),
// which prices the tiles, and the rest heavy first.
// A renderer that draws one frame per scene would otherwise never leave image order ("Heavy tiles first").
static int launch_priced(rt_ctx *c, int n_samples, hipStream_t stream, Form form) {
    bool priced = false;
    if (form != Form::Auto && c->order.wants_pricing(n_samples)) {
        const int rc = launch_form(c, rt::TileOrder::kPricePasses, stream, form);
        if (rc != RT_OK) return rc;
        n_samples -= rt::TileOrder::kPricePasses;
        priced = true;
    }
    const int rc = launch_form(c, n_samples, stream, form);
    if (rc == RT_OK && priced) c->order.sort_again_from_whole_frame();
    return rc;
}

// ---- the two measurements ----
// Both run as four steps on the context's launches (rt_internal.h Probe): arm 0 warm, arm 0 timed, arm 1 warm, arm 1 timed.
constexpr int kProbeSteps = 4;

// what arm 0 / arm 1 of the measurement in flight renders with
static Form probe_arm(const rt::Probe &pr, int arm) {
    if (pr.which == rt::Probe::CoopVsPlain) return arm == 0 ? Form::SweepCoop : Form::SweepPlain;
    return arm == 0 ? Form::Walk : Form::Sweep;
}

// Before a launch of the step that is open: `stream` joins the context's work, and a timed step that holds no passes yet gets its opening event.
// `skip_warm`: this launch is long enough to warm itself -- an open warm step counts as done.  Yields the arm the launch belongs to.
static int probe_begin_step(rt_ctx *c, hipStream_t stream, bool skip_warm, int *arm) {
    rt::Probe &pr = c->probe;
    if (skip_warm && (pr.state & 1) == 0) pr.state += 1;
    const int rc = chain(c, stream);
    if (rc != RT_OK) return rc;
    *arm = pr.state >> 1;
    if ((pr.state & 1) != 0 && pr.acc == 0) HIP_TRY(hipEventRecord(pr.ev[2 * *arm], stream));
    return RT_OK;
}

// After that launch: a warm step ends with it; a timed step ends, with its closing event, once it holds `passes_needed` passes.
static int probe_end_step(rt_ctx *c, hipStream_t stream, int n_samples, int passes_needed) {
    rt::Probe &pr = c->probe;
    const int arm = pr.state >> 1;
    if ((pr.state & 1) != 0) {
        pr.acc += n_samples;
        if (pr.acc < passes_needed) return RT_OK;
        HIP_TRY(hipEventRecord(pr.ev[2 * arm + 1], stream));
        pr.samples[arm] = pr.acc;
        pr.acc = 0;
    }
    pr.state += 1;
    return RT_OK;
}

// hierarchy or sweep is settled, by the estimate or by measurement: the tree the verdict is about (rearm_probe_if_changed)
static void verdict_is_of_this_tree(rt_ctx *c, bool estimated) {
    c->choice.pick_estimated = estimated;
    c->choice.probe_tree = c->bvh_n_tree;
    c->choice.probe_always = c->bvh.n_always;
    c->choice.probe_updates = 0;
}

// the verdict of the measurement in flight, if all four steps are queued and the last event has completed (wait: block for it)
void probe_poll(rt_ctx *c, bool wait) {
    rt::Probe &pr = c->probe;
    const bool coop = pr.which == rt::Probe::CoopVsPlain;
    if ((coop ? c->choice.coop_pick : c->choice.bvh_pick) != Form::Auto || pr.state < kProbeSteps) return;
    if (wait) {
        if (hipEventSynchronize(pr.ev[3]) != hipSuccess) return;
    } else if (hipEventQuery(pr.ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, pr.ev[0], pr.ev[1]) != hipSuccess || hipEventElapsedTime(&b, pr.ev[2], pr.ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    const double ta = (double)a / pr.samples[0], tb = (double)b / pr.samples[1];
    if (coop) {
        // arm 0 = cooperative any-hit, arm 1 = plain.  The plain instance -- what the threshold says -- keeps anything inside 4 %: the scenes the
        // sharing is for gain 7-14 %, the Demo scene loses 2-10 %, and a timed probe of a 1/8 shard of a 1080p frame lasts 65 microseconds (two of the
        // eight shards of profiles/r06_shard_prediction.jsonl's first run picked the slower form on a 2 % dead band)
        c->choice.coop_pick = ta < 0.96 * tb ? Form::SweepCoop : Form::SweepPlain;
        return;
    }
    c->choice.probe_ms[0] = ta;
    c->choice.probe_ms[1] = tb;
    c->choice.bvh_pick = ta <= 1.05 * tb ? Form::Walk : Form::Sweep;      // (a dead band of 5 % towards the usual winner: no flipping on a tie)
    verdict_is_of_this_tree(c, false);
}

void rearm_probe(rt_ctx *c) {
    c->choice.scene_frames = 0;
    c->choice.scene_launches = 0;
    c->choice.coop_pick = c->choice.bvh_pick = Form::Auto;
    c->choice.pick_estimated = false;
    c->choice.probe_ms[0] = c->choice.probe_ms[1] = 0.0;
    c->choice.probe_updates = 0;
    c->probe.which = rt::Probe::None;
    c->probe.state = c->probe.acc = 0;
}

// after a device-resident update rebuilt the hierarchy: is the verdict still about this tree?
void rearm_probe_if_changed(rt_ctx *c) {
    if (c->probe.which == rt::Probe::CoopVsPlain) return;       // (coop against plain on a scene without a hierarchy: an update cannot change the sphere count -- the verdict stays)
    if (c->choice.bvh_pick == Form::Auto && c->probe.state == 0) return;
    if (!c->bvh_ok) {
        rearm_probe(c);
        return;
    }
    const uint32_t tree = c->bvh_n_tree, always = c->bvh.n_always;        // spheres, not padded slots: the shaped tree of an upload has partial leaves
    auto moved = [](uint32_t now, uint32_t then) { return 4u * (now > then ? now - then : then - now) > then + 8u; };
    if (moved(tree, c->choice.probe_tree) || moved(always, c->choice.probe_always) || ++c->choice.probe_updates >= 256) {
        rearm_probe(c);
        c->bvh_est_valid = false;               // (the areas were the uploaded tree's: the changed scene is measured)
    }
}

// Hierarchy or plain sweep for this scene?  The walk wins by 5x on a thousand spheres scattered over a plane and
// loses on a box packed with overlapping glass -- so it is measured, once per scene: four launches in the same
// (natural) tile order -- the hierarchy warm, the hierarchy timed, the sweep warm, the sweep timed, each timed one
// between two events -- and when both timings have arrived (asked without blocking) the form that took less time per
// pass renders the rest.  A blocking call with enough passes splits off 1 + 2 + 1 + 2 passes for the probes and waits
// for the verdict before it queues the rest (progressive passes equal one launch bit for bit).  The verdict is kept
// for the scene; device-resident updates keep it until the tree has changed size by a quarter or 256 updates have
// gone by (rearm_probe_if_changed).  In a multi-device context only the first shard measures; the others follow it.
static int launch_probe(rt_ctx *c, int n_samples, hipStream_t stream) {
    if (c->probe.which == rt::Probe::None) c->probe.which = rt::Probe::WalkVsSweep;
    int arm = 0;
    int rc = probe_begin_step(c, stream, false, &arm);
    if (rc != RT_OK) return rc;
    rc = launch_form(c, n_samples, stream, probe_arm(c->probe, arm), true);
    if (rc != RT_OK) return rc;
    return probe_end_step(c, stream, n_samples, 1);             // (any launch is a whole step)
}

// The same question answered WITHOUT a launch, from the surface areas of the tree the host built at rt_set_scene (rt_bvh.hip):
// a random line through the root box is expected to visit  P = sum of area(inner node) / area(root)  pairs (and leaves in
// proportion), each ray sweeps the always-list besides, and the plain sweep tests all n spheres.  Predicted time per ray of
// the walk over that of the sweep, in units of one sphere test of the sweep:
//     ratio = (kEstPair * P + kEstAlways * n_always) / (n + kEstSweepFixed)
// The three weights are a least-squares fit (log ratio) to the probe's own timings of both forms on 32 scenes of four
// families -- spheres scattered on a plane, a closed box packed with mirror / glass spheres, a cloud in the air, the Demo
// scene plus scattered spheres; 64 to 1400 spheres -- tools/choice_calibration.py, profiles/r04k_choice_calibration.jsonl
// (this round's walk kernel): rms error 11 %, 9 % at worst between 0.55 and 1.8.  (A term for the expected leaf visits fitted to zero: they go with P.)
// Outside a band around 1 the estimate decides and nothing is measured -- a new scene's first frame then costs what a frame
// costs; inside it the four probe launches run as before.
constexpr double kEstPair = 18.7, kEstAlways = 8.9, kEstSweepFixed = 17.9;
constexpr double kEstBandLo = 0.75, kEstBandHi = 1.33;
double estimate_ratio(const rt_ctx *c) {
    return (kEstPair * c->bvh_est_pairs + kEstAlways * (double)c->bvh.n_always) / ((double)c->scene.n_spheres + kEstSweepFixed);
}

// Cooperative any-hit or not for a scene of fewer than coop_min spheres (rt_internal.h Choice::coop_pick): MEASURED, on the host's own launches as they
// come -- never split, never reordered, scheduled like any other (heavy tiles first): the sharing's worth depends on the order the tiles run in, so
// it is timed under the order the frames will run in.  Four steps: coop warm, coop timed, plain warm, plain timed; a step takes whole launches and
// ends once it holds enough passes -- a warm step one launch, a timed step 16 passes between its two events; a launch of 16 passes or more needs no
// warm step (it warms itself), so a host that renders whole frames spends its second frame on the cooperative instance, its third on the plain
// one, and has the verdict for the fourth; a host that queues a pass per call has it after 34 passes.  A scene's FIRST long blocking frame is not
// part of it (a new scene's first frame prices its tiles and runs partly in image order: it measures neither form's steady state), so a host that
// renders one frame per scene never runs the form the threshold would not have picked.  (The first version of this round split a long call into
// four short probe launches in natural tile order, as the hierarchy's probe does: +6 ... +8 % on that frame, and on shards of a frame, 65
// microseconds per timed probe, it picked the slower form on two shards of eight -- profiles/r06_coop_probe_first_frame.jsonl.)
constexpr uint32_t kCoopProbeFrom = 4;          // (below four spheres a shadow sweep has nothing to share out)
constexpr int kCoopTimedPasses = 16;
static int launch_small(rt_ctx *c, int n_samples, hipStream_t stream, bool may_block) {
    if (c->choice.leader)                       // a shard of a multi-device context: the form the first shard just launched
        return launch_priced(c, n_samples, stream, c->choice.leader->choice.last == Form::SweepCoop ? Form::SweepCoop : Form::SweepPlain);
    const uint32_t n = c->scene.n_spheres;
    const bool open = c->choice.coop_probe != 0 && c->coop_min > 0 && n >= kCoopProbeFrom && n < (uint32_t)c->coop_min && c->wg_waves == 0 && c->persist == 0 &&
                      tables_fit_lds(c, n_samples);
    if (!open) return launch_priced(c, n_samples, stream, Form::Sweep);
    c->probe.which = rt::Probe::CoopVsPlain;
    probe_poll(c, false);
    if (c->choice.coop_pick != Form::Auto) return launch_priced(c, n_samples, stream, c->choice.coop_pick);
    if (c->probe.state == kProbeSteps) return launch_priced(c, n_samples, stream, Form::SweepPlain);   // both timings queued, not back yet: what the threshold says meanwhile
    const bool whole_frame = may_block && n_samples >= kCoopTimedPasses;        // (a long launch warms itself)
    if (whole_frame && c->choice.scene_frames == 0 && c->probe.state == 0) return launch_priced(c, n_samples, stream, Form::Sweep);
    int arm = 0;
    int rc = probe_begin_step(c, stream, whole_frame, &arm);
    if (rc != RT_OK) return rc;
    rc = launch_priced(c, n_samples, stream, probe_arm(c->probe, arm));
    if (rc != RT_OK) return rc;
    return probe_end_step(c, stream, n_samples, kCoopTimedPasses);
}

int launch(rt_ctx *c, int n_samples, hipStream_t stream, bool may_block) {
    if (c->tables_stale) {              // records updated on the device since the tables were built: build them now, once
        const int rc = refresh_tables(c, stream);
        if (rc != RT_OK) return rc;
    }
    if (c->walk_forced != 0 || c->mode >= 100) return launch_form(c, n_samples, stream, Form::Auto);      // diagnostics: nothing is measured
    if (n_samples <= 0 || c->local_rows == 0 || !c->have_scene || !c->have_cam) return launch_priced(c, n_samples, stream, Form::Sweep);   // (nothing to render, or the error)
    if (!bvh_usable(c)) return launch_small(c, n_samples, stream, may_block);
    // no probe where the answer is known and asking is dear: from 1500 spheres in the tree on the hierarchy won on every
    // scene measured, open or packed, and one pass of the sweep at 1080p costs 2.6 ms at 1024 spheres,
    // 28 ms at 4096, 138 ms at 8192 from staged tables (through the scalar cache, round 6: a fifth of that at 8192 -- still tens of milliseconds a pass)
    if (c->bvh_n_tree >= kAlwaysWalkFrom || !tables_fit_lds(c, n_samples)) return launch_priced(c, n_samples, stream, Form::Walk);
    if (c->choice.leader)                       // a shard of a multi-device context: the form the first shard just launched
        return launch_priced(c, n_samples, stream, sweeps(c->choice.leader->choice.last) ? Form::Sweep : Form::Walk);
    probe_poll(c, false);
    if (c->choice.bvh_pick == Form::Auto && c->probe.state == 0 && c->choice.use_estimate && c->bvh_est_valid) {
        const double r = estimate_ratio(c);
        c->choice.est_ratio = r;
        if (r < kEstBandLo || r > kEstBandHi) {
            c->choice.bvh_pick = r < 1.0 ? Form::Walk : Form::Sweep;
            verdict_is_of_this_tree(c, true);
        }
    }
    if (c->choice.bvh_pick != Form::Auto) return launch_priced(c, n_samples, stream, c->choice.bvh_pick);
    if (c->probe.state == kProbeSteps) return launch_form(c, n_samples, stream, Form::Walk);    // probes in flight: the usual winner meanwhile
    if (may_block && n_samples >= 16) {
        int done = 0;
        while (c->probe.state < kProbeSteps) {
            const int k = (c->probe.state & 1) ? 2 : 1;
            const int rc = launch_probe(c, k, stream);
            if (rc != RT_OK) return rc;
            done += k;
        }
        probe_poll(c, true);
        return launch_priced(c, n_samples - done, stream, c->choice.bvh_pick != Form::Auto ? c->choice.bvh_pick : Form::Walk);
    }
    return launch_probe(c, n_samples, stream);
}

// a shard's launch on its own stream, for the multi-device context (rt_multi.hip)
int render_shard(rt_ctx *c, int n_samples, bool may_block) {
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    return launch(c, n_samples, c->stream, may_block);
}

}  // namespace rt
