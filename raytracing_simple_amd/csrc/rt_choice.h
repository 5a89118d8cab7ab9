// rt_choice.h -- which form renders a scene: the verdicts a context holds for its scene, the measurement behind them while one runs, the
// surface-area estimate that can stand in for it, and what the next launch is.  Host bookkeeping only: rt_launch.hip launch() asks
// next_launch(), carries out the HIP part (events, the launch itself, the query for the elapsed times) and reports back; the other units
// report what happened to the scene through the named transitions below; nothing else edits this record.  No HIP in here --
// tests/test_choice_cpu.py drives it through its sequences with the host compiler alone (tools/sanitize/choice_main.cpp).
// DESIGN.md section 5.12 lists the transitions, who calls them, and where each constant comes from.
#pragma once

#include <cstdint>

namespace rt {

// What a launch renders with: asked of launch_form() (rt_launch.hip), kept as a scene's verdicts, recorded of the last launch.
//   Auto        the context's own choice from its thresholds.  As a verdict: not decided yet; as the last launch: nothing launched yet
//   Walk        the hierarchy (if the scene has one)
//   Sweep       the plain sweep; cooperative any-hit or not as the sphere count says
//   SweepCoop   the sweep WITH cooperative any-hit whatever the sphere count says (the small-scene measurement); SweepPlain: WITHOUT
enum class Form : uint8_t { Auto, Walk, Sweep, SweepCoop, SweepPlain };
inline bool sweeps(Form f) { return f >= Form::Sweep; }
// the C ABI's number for a hierarchy verdict (rt_scene_choice, rt_debug_bvh_pick): 0 = not decided yet, 1 = hierarchy, 2 = plain sweep
inline int verdict_number(Form f) { return f == Form::Auto ? 0 : (f == Form::Walk ? 1 : 2); }

struct Choice {
    // ---- the rules' numbers ----
    // Both measurements run as four steps on the context's launches: arm 0 warm, arm 0 timed, arm 1 warm, arm 1 timed; a timed step lies
    // between probe event 2 * arm and probe event 2 * arm + 1 (rt_ctx::probe_ev).  They differ in what the arms are and in how many passes a step takes.
    static constexpr int kSteps = 4;
    // hierarchy against sweep: any launch is a whole step; a blocking call of kWalkSplitFrom passes or more splits off 1 + 2 + 1 + 2 passes
    static constexpr int kWalkSplitFrom = 16, kWalkWarmPasses = 1, kWalkTimedPasses = 2;
    static constexpr double kWalkBand = 1.05;           // a dead band of 5 % towards the usual winner: no flipping on a tie
    // no probe where the answer is known and asking is dear: from 1500 spheres in the tree on the hierarchy won on every scene measured, open
    // or packed, and one pass of the sweep at 1080p costs 2.6 ms at 1024 spheres, 28 ms at 4096, 138 ms at 8192 from
    // staged tables (through the scalar cache, round 6: a fifth of that at 8192 -- still tens of milliseconds a pass)
    static constexpr uint32_t kAlwaysWalkFrom = 1500;
    // a verdict outlives device-resident updates until the tree or the always-list has moved by a quarter, or this many updates have gone by
    static constexpr int kRearmUpdates = 256;
    static constexpr bool moved(uint32_t now, uint32_t then) { return 4u * (now > then ? now - then : then - now) > then + 8u; }
    // The same question answered WITHOUT a launch, from the surface areas of the tree the host built at rt_set_scene (rt_bvh.hip):
    // a random line through the root box is expected to visit  P = sum of area(inner node) / area(root)  pairs (and leaves in
    // proportion), each ray sweeps the always-list besides, and the plain sweep tests all n spheres.  Predicted time per ray of
    // the walk over that of the sweep, in units of one sphere test of the sweep:
    //     ratio = (kEstPair * P + kEstAlways * n_always) / (n + kEstSweepFixed)
    // The three weights are a least-squares fit (log ratio) to the probe's own timings of both forms on 32 scenes of four
    // families -- spheres scattered on a plane, a closed box packed with mirror / glass spheres, a cloud in the air, the Demo
    // scene plus scattered spheres; 64 to 1400 spheres -- tools/choice_calibration.py, profiles/r04k_choice_calibration.jsonl
    // (that round's walk kernel): rms error 11 %, 9 % at worst between 0.55 and 1.8.  (A term for the expected leaf visits fitted to zero: they go with P.)
    // Outside a band around 1 the estimate decides and nothing is measured -- a new scene's first frame then costs what a frame
    // costs; inside it the four probe launches run as before.
    static constexpr double kEstPair = 18.7, kEstAlways = 8.9, kEstSweepFixed = 17.9;
    static constexpr double kEstBandLo = 0.75, kEstBandHi = 1.33;
    // cooperative any-hit against plain: a warm step is one launch, a timed step kCoopTimedPasses passes between its two events; a blocking
    // launch that long needs no warm step (it warms itself)
    static constexpr uint32_t kCoopProbeFrom = 4;       // (below four spheres a shadow sweep has nothing to share out)
    static constexpr int kCoopTimedPasses = 16;
    // arm 0 = cooperative any-hit, arm 1 = plain.  The plain instance -- what the threshold says -- keeps anything inside 4 %: the scenes the
    // sharing is for gain 7-14 %, the Demo scene loses 2-10 %, and a timed probe of a 1/8 shard of a 1080p frame lasts 65 microseconds (two of the
    // eight shards of profiles/r06_shard_prediction.jsonl's first run picked the slower form on a 2 % dead band)
    static constexpr double kCoopBand = 0.96;

    // ---- the verdicts ----
    // hierarchy or plain sweep?  Decided per scene by the estimate or by measurement: each form once warm and once
    // timed between events, in the same tile order; whichever took less time per pass renders the rest
    Form bvh_pick = Form::Auto;         // Auto = not decided yet, Walk, Sweep
    bool pick_estimated = false;        // ... and it came from the surface-area estimate, not from a measurement
    int use_estimate = 1;               // diagnostics knob: 0 = every undecided scene is measured
    double est_ratio = 0.0;             // the estimate's predicted walk / sweep time (0 = none made)
    uint32_t probe_tree = 0, probe_always = 0;   // the tree the verdict is about
    int probe_updates = 0;              // device-resident updates since the verdict
    double probe_ms[2] = { 0.0, 0.0 };  // measured time per pass: hierarchy, plain sweep (0 = not measured)
    // ... and for a scene WITHOUT a hierarchy and fewer spheres than coop_min: cooperative any-hit or not, timed on the host's own launches.
    // Below 12 spheres the threshold alone picks wrongly either way -- the Demo scene is 2 % faster without the sharing, the reference's simple.scn,
    // caustic.scn and caustic3.scn (6 and 10 records) 7-11 % faster with it (profiles/r06_reference_scenes.jsonl) -- so it is measured.
    Form coop_pick = Form::Auto;        // Auto = not decided yet, SweepCoop, SweepPlain
    int coop_probe = 1;                 // diagnostics knob: 0 = the threshold alone decides (round 5's behaviour)
    uint32_t scene_frames = 0;          // resets since rt_set_scene that followed at least one launch OF THAT SCENE: frames of it already rendered
    uint64_t scene_launches = 0;        // launches since rt_set_scene
    const Choice *leader = nullptr;     // a shard of a multi-device context: the shard whose launches it follows (null: its own verdicts); only leader->last is read
    Form last = Form::Auto;             // what the last launch was: Walk, SweepCoop (a cooperative any-hit instance) or SweepPlain (any other sweep) --
                                        // what a multi-device context's other shards follow
    // ---- the measurement in flight, if any ----
    enum Which : uint8_t { None, WalkVsSweep, CoopVsPlain };
    Which which = None;
    int state = 0;                      // steps finished (0..4)
    int acc = 0;                        // passes launched so far inside the timed step that is open
    int samples[2] = { 0, 0 };          // passes between the events of arm 0, arm 1
    // ---- surface-area sums of a host-built tree (rt_bvh_host.cpp bvh_estimate): what a random line through the root box is expected to visit --
    // pair steps (inner nodes, the root counted once) and leaves
    double est_pairs = 0.0, est_leaves = 0.0;
    bool est_valid = false;

    // What the caller knows of context and scene when it asks for the next launch (rt_launch.hip choice_facts)
    struct Facts {
        bool diagnostics = false;       // a forced walk or an instance by number (mode >= 100): nothing is measured
        bool nothing_to_render = false; // no passes, no rows, no scene or no camera: launch_form says which
        bool hierarchy = false;         // the scene has one and the context may use it
        bool tables_fit = false;        // the plain sweep's tables fit LDS for this launch
        uint32_t n_tree = 0, n_always = 0, n_spheres = 0;
        int coop_min = 0, wg_waves = 0, persist = 0;
    };

    // What the caller does next.  Launch: `passes` passes of `form` through launch_priced (priced) or launch_form (natural_order as given), between
    // the probe events named (-1: none); a launch with `step` set is reported by step_queued(); `more`: ask again for the passes left.  Times /
    // TimesBlocking: launch nothing yet -- query (wait for) probe event 3, report times_arrived() if both times can be read, and ask again.
    // Either way the answer goes back in as `prev`.
    struct Next {
        enum Ask : uint8_t { Launch, Times, TimesBlocking };
        Ask ask = Launch;
        Form form = Form::Auto;
        int passes = 0;
        bool natural_order = false, priced = false;
        int record_before = -1, record_after = -1;
        bool step = false, closes = false;      // part of the step that is open; ... and its last launch
        bool more = false;
    };

    // ---- what happened ----
    // rt_set_scene with other records: everything about the old scene goes; the knobs, the estimate's last ratio, `last` and `leader` stay
    void new_scene() {
        scene_frames = 0;
        scene_launches = 0;
        coop_pick = bvh_pick = Form::Auto;
        pick_estimated = false;
        probe_ms[0] = probe_ms[1] = 0.0;
        probe_updates = 0;
        which = None;
        state = acc = 0;
    }
    // diagnostics: a knob that changes what the verdicts are about (the hierarchy's threshold or shape, a forced walk) -- undecided again
    void knob_set() { new_scene(); }
    void coop_threshold_set_by_hand() { coop_probe = 0; new_scene(); }      // (it decides alone from now on: no measurement)
    void estimate_switched(bool on) { use_estimate = on ? 1 : 0; new_scene(); }
    // a multi-device context's shard other than the first: ONE decision per context, the first shard's
    void follow(const Choice *first_shard) { leader = first_shard; }
    // rt_reset / rt_reset_async / a written state: a frame of the current scene has been rendered, if anything of it was launched
    void frame_ended() { if (scene_launches > 0) scene_frames += 1; }
    // a full upload begins: the estimate was another scene's ... (a device-resident update keeps the upload's estimate until tables_rebuilt says it is stale)
    void uploading_without_estimate() { est_valid = false; }
    // ... and the host has shaped this scene's tree (rt_bvh.hip upload_host_tree)
    void tree_uploaded(bool valid, double pairs, double leaves) { est_valid = valid; est_pairs = pairs; est_leaves = leaves; }
    // a device-resident update rebuilt tables and hierarchy: is the verdict still about this tree?
    void tables_rebuilt(bool have_tree, uint32_t n_tree, uint32_t n_always) {       // spheres, not padded slots: the shaped tree of an upload has partial leaves
        if (which == CoopVsPlain) return;       // (coop against plain on a scene without a hierarchy: an update cannot change the sphere count -- the verdict stays)
        if (bvh_pick == Form::Auto && state == 0) return;
        if (!have_tree) {
            new_scene();
            return;
        }
        if (moved(n_tree, probe_tree) || moved(n_always, probe_always) || ++probe_updates >= kRearmUpdates) {
            new_scene();
            est_valid = false;                  // (the areas were the uploaded tree's: the changed scene is measured)
        }
    }
    // a full launch is queued (every launch_form, pricing launches included)
    void launch_queued(Form what) { scene_launches += 1; last = what; }
    // ... or a subset launch (rt_render_tiles_async).  A timed step of the cooperative-or-plain measurement that is open lies between an event and
    // the full launches still to come: this launch would be timed with them, so the step starts again with the next full launch -- nothing of the
    // measurement is started, advanced or timed by it
    void subset_launch_queued(Form what) {
        if ((state & 1) != 0 && acc > 0) acc = 0;
        launch_queued(what);
    }
    // the launch next_launch() marked `step` is queued, its events recorded: a warm step ends with it, a timed step with the launch that `closes` it
    void step_queued(const Next &nx) {
        if ((state & 1) != 0) {
            acc += nx.passes;
            if (!nx.closes) return;
            samples[state >> 1] = acc;
            acc = 0;
        }
        state += 1;
    }
    // all four steps are queued and no verdict yet: the elapsed times are worth asking for
    bool awaiting_times() const { return (which == CoopVsPlain ? coop_pick : bvh_pick) == Form::Auto && state >= kSteps; }
    // both elapsed times (ms between the events of arm 0, of arm 1) have arrived: the verdict, per pass
    void times_arrived(double a_ms, double b_ms, uint32_t n_tree, uint32_t n_always) {
        const double ta = a_ms / samples[0], tb = b_ms / samples[1];
        if (which == CoopVsPlain) {
            coop_pick = ta < kCoopBand * tb ? Form::SweepCoop : Form::SweepPlain;
            return;
        }
        probe_ms[0] = ta;
        probe_ms[1] = tb;
        bvh_pick = ta <= kWalkBand * tb ? Form::Walk : Form::Sweep;
        verdict_is_of_this_tree(false, n_tree, n_always);
    }

    double estimate_ratio(uint32_t n_always, uint32_t n_spheres) const {
        return (kEstPair * est_pairs + kEstAlways * (double)n_always) / ((double)n_spheres + kEstSweepFixed);
    }

    // ---- the decision ----
    // What the next launch of a call for `n_samples` passes is (what is LEFT of the call, when `prev` said `more`).  `may_block`: the call waits for
    // its frame anyway, so it may wait for a verdict.  `prev`: this call's previous answer (null: the first).  The order of the checks is the order
    // in which the answers are known and cheap.
    Next next_launch(const Facts &f, int n_samples, bool may_block, const Next *prev = nullptr) {
        if (f.diagnostics) return render(Form::Auto, n_samples, false);
        if (f.nothing_to_render) return render(Form::Sweep, n_samples, true);
        if (!f.hierarchy) return next_small(f, n_samples, may_block, prev);
        if (f.n_tree >= kAlwaysWalkFrom || !f.tables_fit) return render(Form::Walk, n_samples, true);
        if (leader) return render(sweeps(leader->last) ? Form::Sweep : Form::Walk, n_samples, true);       // the form the first shard just launched
        // Hierarchy or plain sweep for this scene?  The walk wins by 5x on a thousand spheres scattered over a plane and
        // loses on a box packed with overlapping glass -- so it is measured, once per scene: four launches in the same
        // (natural) tile order -- the hierarchy warm, the hierarchy timed, the sweep warm, the sweep timed, each timed one
        // between two events -- and when both timings have arrived (asked without blocking) the form that took less time per
        // pass renders the rest.  A blocking call with enough passes splits off 1 + 2 + 1 + 2 passes for the probes and waits
        // for the verdict before it queues the rest (progressive passes equal one launch bit for bit).  The verdict is kept
        // for the scene; device-resident updates keep it until the tree has changed size by a quarter or 256 updates have
        // gone by (tables_rebuilt).  In a multi-device context only the first shard measures; the others follow it.
        if (prev && prev->more) {               // inside a blocking call's split
            if (state < kSteps) return walk_step((state & 1) ? kWalkTimedPasses : kWalkWarmPasses, true);
            return ask(Next::TimesBlocking);
        }
        if (prev && prev->ask == Next::TimesBlocking) return render(bvh_pick != Form::Auto ? bvh_pick : Form::Walk, n_samples, true);
        if (!prev && awaiting_times()) return ask(Next::Times);
        if (bvh_pick == Form::Auto && state == 0 && use_estimate && est_valid) {
            const double r = est_ratio = estimate_ratio(f.n_always, f.n_spheres);
            if (r < kEstBandLo || r > kEstBandHi) {
                bvh_pick = r < 1.0 ? Form::Walk : Form::Sweep;
                verdict_is_of_this_tree(true, f.n_tree, f.n_always);
            }
        }
        if (bvh_pick != Form::Auto) return render(bvh_pick, n_samples, true);
        if (state == kSteps) return render(Form::Walk, n_samples, false);      // probes in flight: the usual winner meanwhile
        if (may_block && n_samples >= kWalkSplitFrom) return walk_step((state & 1) ? kWalkTimedPasses : kWalkWarmPasses, true);
        return walk_step(n_samples, false);
    }

private:
    // Cooperative any-hit or not for a scene of fewer than coop_min spheres: MEASURED, on the host's own launches as they
    // come -- never split, never reordered, scheduled like any other (heavy tiles first): the sharing's worth depends on the order the tiles run in, so
    // it is timed under the order the frames will run in.  Four steps: coop warm, coop timed, plain warm, plain timed; a step takes whole launches and
    // ends once it holds enough passes -- a warm step one launch, a timed step 16 passes between its two events; a launch of 16 passes or more needs no
    // warm step (it warms itself), so a host that renders whole frames spends its second frame on the cooperative instance, its third on the plain
    // one, and has the verdict for the fourth; a host that queues a pass per call has it after 34 passes.  A scene's FIRST long blocking frame is not
    // part of it (a new scene's first frame prices its tiles and runs partly in image order: it measures neither form's steady state), so a host that
    // renders one frame per scene never runs the form the threshold would not have picked.  (The first version of round 6 split a long call into
    // four short probe launches in natural tile order, as the hierarchy's probe does: +6 ... +8 % on that frame, and on shards of a frame, 65
    // microseconds per timed probe, it picked the slower form on two shards of eight -- profiles/r06_coop_probe_first_frame.jsonl.)
    Next next_small(const Facts &f, int n_samples, bool may_block, const Next *prev) {
        if (leader) return render(leader->last == Form::SweepCoop ? Form::SweepCoop : Form::SweepPlain, n_samples, true);
        const bool open = coop_probe != 0 && f.coop_min > 0 && f.n_spheres >= kCoopProbeFrom && f.n_spheres < (uint32_t)f.coop_min && f.wg_waves == 0 &&
                          f.persist == 0 && f.tables_fit;
        if (!open) return render(Form::Sweep, n_samples, true);
        which = CoopVsPlain;
        if (!prev && awaiting_times()) return ask(Next::Times);
        if (coop_pick != Form::Auto) return render(coop_pick, n_samples, true);
        if (state == kSteps) return render(Form::SweepPlain, n_samples, true);     // both timings queued, not back yet: what the threshold says meanwhile
        const bool whole_frame = may_block && n_samples >= kCoopTimedPasses;
        if (whole_frame && scene_frames == 0 && state == 0) return render(Form::Sweep, n_samples, true);
        if (whole_frame && (state & 1) == 0) state += 1;                            // (a long launch warms itself: an open warm step counts as done)
        return step(n_samples, kCoopTimedPasses, false, true, false);
    }

    static Next ask(Next::Ask what) { Next nx; nx.ask = what; return nx; }
    static Next render(Form form, int passes, bool priced) { Next nx; nx.form = form; nx.passes = passes; nx.priced = priced; return nx; }
    // a launch of the step that is open: its arm's form, the opening event if it is the timed step's first launch, the closing one if it holds `passes_needed` with it
    Next step(int passes, int passes_needed, bool natural_order, bool priced, bool more) const {
        const int arm = state >> 1;
        const bool timed = (state & 1) != 0;
        Next nx = render(which == CoopVsPlain ? (arm == 0 ? Form::SweepCoop : Form::SweepPlain) : (arm == 0 ? Form::Walk : Form::Sweep), passes, priced);
        nx.natural_order = natural_order;
        nx.step = true;
        nx.closes = !timed || acc + passes >= passes_needed;
        if (timed && acc == 0) nx.record_before = 2 * arm;
        if (timed && nx.closes) nx.record_after = 2 * arm + 1;
        nx.more = more;
        return nx;
    }
    Next walk_step(int passes, bool more) {                                         // (any launch is a whole step)
        if (which == None) which = WalkVsSweep;
        return step(passes, 1, true, false, more);
    }
    // hierarchy or sweep is settled, by the estimate or by measurement: the tree the verdict is about (tables_rebuilt)
    void verdict_is_of_this_tree(bool estimated, uint32_t n_tree, uint32_t n_always) {
        pick_estimated = estimated;
        probe_tree = n_tree;
        probe_always = n_always;
        probe_updates = 0;
    }
};

}  // namespace rt
