// rt_launch.hip -- what one launch of the render kernel is made of: which kernel instance (rt_device.h Instance: arithmetic mode x
// role x workgroup shape; the rule that picks role and shape and sizes the LDS is rt_instance.h), its tables, the scheduling data it runs with (heavy-first tile order) and, for scenes
// that have a hierarchy, whether it is walked or the plain sweep runs -- settled by a
// surface-area estimate at rt_set_scene, by measurement inside the estimate's band (rt_choice.h holds the rules; launch() carries them out).
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
    p.scene = c->scene.tables;
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
    p.coop_kmax = c->knobs.coop_kmax;
    p.direct_max = c->knobs.direct_max;
    p.tiles_x = (int)tiles_per_row(c);
    p.n_tiles = (int)tile_count(c);
    return p;
}


// ---- which instance, and what it needs (rt_device.h Instance; the rows live next to the instantiations; the rule is rt_instance.h) ----

const rt::Instance *instances(bool fast, int *count) { return fast ? rt::fast_instances(count) : rt::parity_instances(count); }

// the row with this role and workgroup shape (null: this library has none)
static const rt::Instance *find_role(bool fast, int role, int waves) {
    int n = 0;
    const rt::Instance *t = instances(fast, &n);
    for (int k = 0; k < n; ++k)
        if (t[k].role == role && t[k].waves == waves) return &t[k];
    return nullptr;
}

// what the rule (rt_instance.h) reads of the context's scene
rt::SceneFacts scene_facts(const rt_ctx *c) {
    rt::SceneFacts s;
    s.n_spheres = c->scene.tables.n_spheres;
    s.n_lights = c->scene.tables.n_lights;
    s.has_hierarchy = c->scene.state.has_hierarchy();
    s.n_leaves = c->scene.bvh.n_leaves;
    s.n_slots = c->scene.bvh.n_slots;
    s.stack_depth = c->scene.bvh.stack_depth;
    s.n_top = c->scene.bvh.n_top;
    s.packed_at = c->scene.bvh.packed_at;
    return s;
}

// the plain sweep's tables (geometry and lights) fit LDS for this launch
bool tables_fit_lds(const rt_ctx *c, int n_samples) { return rt::sweep_tables_fit(scene_facts(c), n_samples); }

// What the instance needs from the context, checked against what the context has: the ONE place that hands out the hierarchy and
// the dynamic LDS (sized by instance_lds).  An instance whose tables the context lacks is refused (RT_ERR_STATE),
// whatever route selected it -- the measured choice, a forced form, or a diagnostics mode.
static int bind_tables(rt_ctx *c, const rt::Instance &inst, const rt::SceneFacts &facts, int n_samples, rt::LaunchParams &p, size_t *lds_out) {
    size_t lds = 0;
    const int rc = rt::instance_lds(inst.tables, inst.waves, inst.flags, facts, p.mat_in_lds != 0, n_samples, &lds);
    p.bvh = rt::BvhTables{};
    if (rt::walks_hierarchy(inst.tables)) {
        if (rc == rt::kLdsNoHierarchy || !c->scene.bvh.blob)
            return fail(RT_ERR_STATE, "%s walks a hierarchy and the scene has none (fewer than %d small spheres?)", inst.name, c->knobs.bvh_min);
        p.bvh = c->scene.bvh;
    }
    if (rc == rt::kLdsNoPackedTable) return fail(RT_ERR_STATE, "%s reads the packed pair table and this scene's hierarchy has none", inst.name);
    if (rc == rt::kLdsNoPromotedTop) return fail(RT_ERR_STATE, "%s stages the promoted top of the tree and this scene's hierarchy has none", inst.name);
    if (rc == rt::kLdsUnknownKind) return fail(RT_ERR_STATE, "%s: unknown table kind %d", inst.name, inst.tables);
    if (inst.tables != rt::kTabSweepLds) p.mat_in_lds = 0;      // (only the staged sweep takes the materials along)
#if RT_DIAGNOSTICS
    if (const char *pad = getenv("RT_LDS_PAD")) lds += (size_t)atoi(pad);       // occupancy experiments: fewer workgroups per CU
#endif
    if (lds > kLdsMax) return fail(RT_ERR_ARG, "%s needs %zu B of LDS for this scene (limit %zu)", inst.name, lds, kLdsMax);
    *lds_out = lds;
    return RT_OK;
}

// Which instance renders a launch of `form`: the row of the shape the rule picks (rt_instance.h pick_shape), or -- diagnostics -- the row the mode names.
// Reads the context, changes nothing, calls nothing of HIP.
static int choose_instance(const rt_ctx *c, const rt::Shape &shape, const rt::Instance **out) {
    const rt::Knobs &k = c->knobs;
    const rt::Instance *inst = nullptr;
#if RT_DIAGNOSTICS
    if (k.by_row()) {                       // a row of the table by number (rt_set_mode checked the range)
        int n = 0;
        inst = &instances(k.fast(), &n)[k.row()];
    }
#endif
    if (!inst) inst = find_role(k.fast(), shape.role, shape.waves);
    // (the product library ships no 4-wavefront PLAIN sweep: below 12 spheres the tables always fit the single-wavefront budget; should a
    // launch get here all the same, the cooperative instance of that shape renders any scene -- same bits, it only shares its shadow sweeps)
    if (!inst && shape.role == rt::kRolePlain) inst = find_role(k.fast(), rt::kRoleCoop, shape.waves);
    if (!inst) return fail(RT_ERR_STATE, "this library holds no %s instance of role %d with %d wavefronts per workgroup", k.fast() ? "fast" : "parity", shape.role, shape.waves);
    *out = inst;
    return RT_OK;
}

// What launch_form and launch_tiles refuse alike ...
static int check_launch_args(const rt_ctx *c, int n_samples) {
    if (!c->scene.state.renderable()) return fail(RT_ERR_STATE, "rt_set_scene and rt_set_camera must precede rendering");
    if (n_samples < 0) return fail(RT_ERR_ARG, "n_samples < 0");
    if (n_samples > 0x7fffffff - c->frame.current_sample)
        return fail(RT_ERR_ARG, "pass counter would overflow (%d + %d)", c->frame.current_sample, n_samples);
    return RT_OK;
}

// ... and what both make of `form` once something is to be launched: the instance, its parameters, its tables and its LDS.  `from_list`: the launch
// takes its tiles from a subset launch's list, which an instance of a wider tile, or one that walks no list at all, cannot render.
struct Prepared { const rt::Instance *inst = nullptr; rt::LaunchParams p{}; size_t lds = 0; };
static int prepare_launch(rt_ctx *c, int n_samples, Form form, bool from_list, Prepared *out) {
    const rt::SceneFacts facts = scene_facts(c);
    const rt::Shape shape = rt::pick_shape(c->knobs, facts, n_samples, form);
    RT_TRY(choose_instance(c, shape, &out->inst));
    const rt::Instance *inst = out->inst;
    if (from_list && ((inst->flags & (rt::kInstTwoRays | rt::kInstPersistent | rt::kInstNoTileCost)) != 0 || (inst->waves != 1 && inst->waves != 4)))
        return fail(RT_ERR_STATE, "rt_render_tiles_async: %s does not render a 32x8 group from a tile list (a wider tile, or no list at all)", inst->name);
    out->p = make_params(c, n_samples);
    out->p.mat_in_lds = shape.mat_in_lds ? 1 : 0;
    out->p.regen_gate = shape.regen_gate;
    out->p.walk_round = (c->knobs.walk_round & 0xff) | (c->knobs.walk_tail << 8);       // (one kernel argument: pair steps in a row | tail lanes << 8)
    return bind_tables(c, *inst, facts, n_samples, out->p, &out->lds);
}

// The launch is queued: the frame has its passes, and the form choice knows what rendered them
static void after_launch(rt_ctx *c, const rt::Instance &inst, int n_samples, const bool *all_groups) {
    c->last_kernel = inst.name;
    const bool coop = inst.role == rt::kRoleCoop || inst.role == rt::kRolePersistCoop;
    const Form what = rt::walks_hierarchy(inst.tables) ? Form::Walk : (coop ? Form::SweepCoop : Form::SweepPlain);
    if (all_groups) {
        c->frame.launched_subset(n_samples, c->pixel_write != 0, *all_groups);
        c->choice.subset_launch_queued(what);
    } else {
        c->frame.launched(n_samples, c->pixel_write != 0);
        c->choice.launch_queued(what);
    }
}

// persistent instances: just enough workgroups to fill the machine; the tile queue (counters[30]) does the rest
static int persist_grid(rt_ctx *c, int n_tiles, size_t lds_use, hipStream_t stream, dim3 *grid) {
    size_t per_cu = lds_use > 0 ? (160 * 1024) / (lds_use + 6 * 1024) : 6;
    if (per_cu > 6) per_cu = 6;
    if (per_cu < 1) per_cu = 1;
    size_t blocks = (size_t)c->knobs.n_cus * per_cu;
    const size_t needed = ((size_t)n_tiles + 3) / 4;
    if (blocks > needed) blocks = needed;
    *grid = dim3((unsigned)blocks, 1, 1);
    HIP_TRY(hipMemsetAsync(c->d_counters + 30, 0, sizeof(unsigned long long), stream));
    return RT_OK;
}

// the instance goes into `stream` -- or the launch is reported as failed
static int queue_instance(const rt::Instance &inst, const rt::LaunchParams &p, dim3 grid, size_t lds, hipStream_t stream) {
    const hipError_t e = rt::launch_instance(inst, p, grid, lds, stream);
    if (e != hipSuccess)
        return fail(RT_ERR_HIP, "kernel launch failed: %s (%s, grid %ux%u, lds %zu B)", hipGetErrorString(e), inst.name, grid.x, grid.y, lds);
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

    const int tile_w = rt::tile_width(inst->waves, inst->flags);
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
    RT_TRY(queue_instance(*inst, p, grid, lds_use, stream));
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
    if (c->scene.state.tables_stale) {
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

    const int tile_w = rt::tile_width(inst->waves, inst->flags);       // (8 per wavefront: prepare_launch refused the wider tile)
    const uint32_t tiles_x = (uint32_t)((c->w + tile_w - 1) / tile_w), tiles_y = tile_row_count(c);
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
    if (frame.current_sample == 0 && !all) {
        // ... and the colours of a 0-pass render, zeros: rt_reset_async, rt_seed_stream_async and a state written at pass 0 leave an old frame in the
        // plane, and pass 0 overwrites it in the tiles this launch renders only.  (The packed pixels of those tiles stay unspecified: include/rt_api.h.)
        HIP_TRY(hipMemsetAsync(c->d_colors, 0, color_floats(c) * sizeof(float), stream));
    }
    p.order = c->tiles.d_list;
    p.tile_cost = nullptr;
    RT_TRY(queue_instance(*inst, p, grid, lds_use, stream));
    if (!all) {
        rc = tiles_advance(c, n_samples, stream);           // (reads current_sample as it was: the count the selected groups come from)
        if (rc != RT_OK) return rc;
    }
    after_launch(c, *inst, n_samples, &all);        // (an open timed step of the small-scene measurement starts again: Choice::subset_launch_queued)
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

// ---- which form renders the scene: rt_choice.h decides, this carries it out ----

// the verdict of the measurement in flight, if all four steps are queued and the last event has completed (wait: block for it)
void probe_poll(rt_ctx *c, bool wait) {
    if (!c->choice.awaiting_times()) return;
    hipEvent_t *ev = c->probe_ev;
    if (wait) {
        if (hipEventSynchronize(ev[3]) != hipSuccess) return;
    } else if (hipEventQuery(ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, ev[0], ev[1]) != hipSuccess || hipEventElapsedTime(&b, ev[2], ev[3]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    c->choice.times_arrived(a, b, c->scene.state.n_tree, c->scene.bvh.n_always);
}

int launch(rt_ctx *c, int n_samples, hipStream_t stream, bool may_block) {
    if (c->scene.state.tables_stale) {              // records updated on the device since the tables were built: build them now, once
        const int rc = refresh_tables(c, stream);
        if (rc != RT_OK) return rc;
    }
    using Next = rt::Choice::Next;
    const rt::Choice::Facts facts = rt::choice_facts(c->knobs, scene_facts(c), n_samples, c->local_rows != 0 && c->scene.state.renderable(),
                                                    c->scene.state.n_tree, c->scene.bvh.n_always);
    Next nx, prev;
    for (bool first = true;; first = false, prev = nx) {
        nx = c->choice.next_launch(facts, n_samples, may_block, first ? nullptr : &prev);
        if (nx.ask != Next::Launch) {
            probe_poll(c, nx.ask == Next::TimesBlocking);
            continue;
        }
        if (nx.record_before >= 0) {    // a timed step opens: `stream` joins the context's work first
            RT_TRY(chain(c, stream));
            HIP_TRY(hipEventRecord(c->probe_ev[nx.record_before], stream));
        }
        RT_TRY(nx.priced ? launch_priced(c, nx.passes, stream, nx.form) : launch_form(c, nx.passes, stream, nx.form, nx.natural_order));
        if (nx.record_after >= 0) HIP_TRY(hipEventRecord(c->probe_ev[nx.record_after], stream));
        if (nx.step) c->choice.step_queued(nx);
        if (!nx.more) return RT_OK;
        n_samples -= nx.passes;
    }
}

// a shard's launch on its own stream, for the multi-device context (rt_multi.hip)
int render_shard(rt_ctx *c, int n_samples, bool may_block) {
    int rc = select_device(c);
    if (rc != RT_OK) return rc;
    return launch(c, n_samples, c->stream, may_block);
}

}  // namespace rt
