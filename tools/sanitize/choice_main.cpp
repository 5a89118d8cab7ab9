// The record of which form renders a scene (csrc/rt_choice.h) alone, under AddressSanitizer + UndefinedBehaviorSanitizer: a host that does what
// rt_launch.hip launch() does with the record's answers -- minus HIP: a launch is a line in a log, an event an index, the elapsed times two numbers
// the case hands in when it wants them to have arrived.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I raytracing_simple_amd/csrc tools/sanitize/choice_main.cpp -o choice_san && ./choice_san
// One line per case ("ok <case>" / "FAILED <case>: ..."), then "choice: clean"; the exit status is the number of failed cases.
// The expectations are literals: read off rt_launch.hip as it stood before the record existed, and off the GPU tests that describe it.
#include <cstdio>
#include <string>
#include <vector>

#include "rt_choice.h"

using rt::Choice;
using rt::Form;
using Facts = rt::Choice::Facts;
using Next = rt::Choice::Next;

namespace {
int g_failed = 0;
void check(const char *name, bool ok, const char *what) {
    if (ok) printf("ok %s\n", name);
    else { printf("FAILED %s: %s\n", name, what); g_failed += 1; }
}

struct Launch { Form form; int passes; bool priced, natural; int before, after; bool step; };

// launch() of rt_launch.hip without the device
struct Host {
    Choice ch;
    Facts f;
    std::vector<Launch> log;
    bool times_in = false;
    double a_ms = 0.0, b_ms = 0.0;      // between the events of arm 0, of arm 1
    int asked = 0, asked_blocking = 0;

    // what after_launch makes of the instance that rendered `form`
    Form rendered(Form form) const {
        if (form == Form::Walk || form == Form::SweepCoop || form == Form::SweepPlain) return form;
        return f.coop_min > 0 && f.n_spheres >= (uint32_t)f.coop_min ? Form::SweepCoop : Form::SweepPlain;
    }
    void call(int n_samples, bool may_block) {
        Next nx, prev;
        for (bool first = true;; first = false, prev = nx) {
            nx = ch.next_launch(f, n_samples, may_block, first ? nullptr : &prev);
            if (nx.ask != Next::Launch) {
                (nx.ask == Next::TimesBlocking ? asked_blocking : asked) += 1;
                if (ch.awaiting_times() && (times_in || nx.ask == Next::TimesBlocking)) ch.times_arrived(a_ms, b_ms, f.n_tree, f.n_always);
                continue;
            }
            log.push_back(Launch{ nx.form, nx.passes, nx.priced, nx.natural_order, nx.record_before, nx.record_after, nx.step });
            ch.launch_queued(rendered(nx.form));
            if (nx.step) ch.step_queued(nx);
            if (!nx.more) return;
            n_samples -= nx.passes;
        }
    }
    void frame(int n_samples) { call(n_samples, true); ch.frame_ended(); }
    // the forms of launches [from, to) are all `form`
    bool all(size_t from, size_t to, Form form) const {
        if (to > log.size()) return false;
        for (size_t i = from; i < to; ++i)
            if (log[i].form != form) return false;
        return true;
    }
};

bool is(const Launch &l, Form form, int passes, bool priced, bool natural, int before, int after, bool step) {
    return l.form == form && l.passes == passes && l.priced == priced && l.natural == natural && l.before == before && l.after == after && l.step == step;
}

Host small_scene(uint32_t n_spheres = 9) {
    Host h;
    h.f.tables_fit = true;
    h.f.n_spheres = n_spheres;
    h.f.coop_min = 12;
    return h;
}
Host tree_scene(uint32_t n_tree = 200, bool estimate = false) {
    Host h;
    h.f.hierarchy = h.f.tables_fit = true;
    h.f.n_tree = h.f.n_spheres = n_tree;
    h.f.coop_min = 12;
    if (!estimate) h.ch.estimate_switched(false);
    return h;
}
// a host that has queued the small scene's four steps a pass per call (17 + 17 launches), times not in yet
Host small_scene_measured() {
    Host h = small_scene();
    for (int k = 0; k < 34; ++k) h.call(1, false);
    return h;
}
// a tree scene whose verdict was measured a launch per step
Host tree_scene_measured(uint32_t n_tree, double walk_ms, double sweep_ms, bool est_valid = false) {
    Host h = tree_scene(n_tree);
    if (est_valid) h.ch.tree_uploaded(true, 11.0, 30.0);
    for (int k = 0; k < 4; ++k) h.call(1, false);
    h.times_in = true;
    h.a_ms = walk_ms;
    h.b_ms = sweep_ms;
    h.call(1, false);
    return h;
}
}  // namespace

int main() {
    // 1. whole frames of 40 passes, blocking, 4 to 11 spheres, no hierarchy
    for (uint32_t n : { 4u, 9u, 11u }) {
        Host h = small_scene(n);
        h.frame(40);
        h.frame(40);
        h.frame(40);
        bool ok = h.log.size() == 3 && h.asked == 0 &&
                  is(h.log[0], Form::Sweep, 40, true, false, -1, -1, false) &&          // the scene's first frame: priced, no part of the measurement
                  is(h.log[1], Form::SweepCoop, 40, true, false, 0, 1, true) &&
                  is(h.log[2], Form::SweepPlain, 40, true, false, 2, 3, true);
        ok = ok && h.ch.samples[0] == 40 && h.ch.samples[1] == 40 && h.ch.state == 4 && h.ch.coop_pick == Form::Auto;
        h.times_in = true;
        h.a_ms = 40.0;
        h.b_ms = 48.0;
        h.frame(40);
        h.frame(40);
        ok = ok && h.log.size() == 5 && h.asked == 1 && h.asked_blocking == 0 && is(h.log[3], Form::SweepCoop, 40, true, false, -1, -1, false) &&
             is(h.log[4], Form::SweepCoop, 40, true, false, -1, -1, false) && h.ch.coop_pick == Form::SweepCoop && h.ch.bvh_pick == Form::Auto;
        check(n == 4 ? "whole_frames_small_scene_4" : (n == 9 ? "whole_frames_small_scene_9" : "whole_frames_small_scene_11"), ok,
              "not Sweep priced, SweepCoop, SweepPlain, then the verdict, one launch a frame");
    }
    // 2. the same scene a pass per non-blocking call
    {
        Host h = small_scene_measured();
        bool ok = h.log.size() == 34 && h.all(0, 17, Form::SweepCoop) && h.all(17, 34, Form::SweepPlain);
        for (size_t i = 0; ok && i < 34; ++i) {
            const int before = i == 1 ? 0 : (i == 18 ? 2 : -1), after = i == 16 ? 1 : (i == 33 ? 3 : -1);
            ok = is(h.log[i], i < 17 ? Form::SweepCoop : Form::SweepPlain, 1, true, false, before, after, true);
        }
        ok = ok && h.ch.samples[0] == 16 && h.ch.samples[1] == 16 && h.ch.state == 4;
        for (int k = 0; k < 3; ++k) h.call(1, false);           // times not in: what the threshold says meanwhile
        ok = ok && h.log.size() == 37 && h.asked == 3 && is(h.log[34], Form::SweepPlain, 1, true, false, -1, -1, false) && h.all(34, 37, Form::SweepPlain) &&
             h.ch.coop_pick == Form::Auto;
        h.times_in = true;
        h.a_ms = 10.0;
        h.b_ms = 16.0;
        h.call(1, false);
        h.call(1, false);
        ok = ok && h.asked == 4 && h.all(37, 39, Form::SweepCoop) && !h.log[38].step && h.ch.coop_pick == Form::SweepCoop;
        check("a_pass_per_call_small_scene", ok, "not 17 SweepCoop, 17 SweepPlain, SweepPlain until the times arrive, then the verdict");
    }
    // 3. a subset launch after the warm step and 5 timed passes of arm 0: the step starts again
    {
        Host h = small_scene();
        for (int k = 0; k < 6; ++k) h.call(1, false);
        bool ok = h.ch.state == 1 && h.ch.acc == 5;
        h.ch.subset_launch_queued(Form::SweepCoop);
        ok = ok && h.ch.state == 1 && h.ch.acc == 0 && h.ch.last == Form::SweepCoop;
        for (int k = 0; k < 33; ++k) h.call(1, false);
        ok = ok && h.log.size() == 39 && h.all(0, 22, Form::SweepCoop) && h.all(22, 39, Form::SweepPlain) && h.log[6].before == 0 && h.log[21].after == 1 &&
             h.log[20].after == -1 && h.ch.samples[0] == 16 && h.ch.samples[1] == 16 && h.ch.state == 4;
        check("subset_launch_restarts_the_timed_step", ok, "not 22 SweepCoop then 17 SweepPlain with the opening event recorded again");
    }
    // 4. the coop dead band: 4 % towards the plain instance
    {
        Host lo = small_scene_measured(), hi = small_scene_measured();
        lo.times_in = hi.times_in = true;
        lo.b_ms = hi.b_ms = 16.0;
        lo.a_ms = 0.95 * 16.0;
        hi.a_ms = 0.97 * 16.0;
        lo.call(1, false);
        hi.call(1, false);
        check("coop_dead_band", lo.ch.coop_pick == Form::SweepCoop && lo.log.back().form == Form::SweepCoop && hi.ch.coop_pick == Form::SweepPlain &&
              hi.log.back().form == Form::SweepPlain && lo.ch.probe_ms[0] == 0.0 && lo.ch.bvh_pick == Form::Auto, "0.95 x is not SweepCoop or 0.97 x not SweepPlain");
    }
    // 5. the coop knob: a threshold set by hand decides alone
    {
        Host h = small_scene();
        h.ch.coop_threshold_set_by_hand();
        h.f.coop_min = 5;
        h.frame(40);
        h.frame(40);
        for (int k = 0; k < 40; ++k) h.call(1, false);
        bool ok = h.log.size() == 42 && h.all(0, 42, Form::Sweep) && h.asked == 0 && h.ch.which == Choice::None && h.ch.state == 0 && h.ch.coop_probe == 0 &&
                  h.ch.last == Form::SweepCoop;
        for (const Launch &l : h.log) ok = ok && !l.step && l.priced && l.before == -1 && l.after == -1;
        check("coop_knob_opens_nothing", ok, "a threshold set by hand measured something");
    }
    // 6. hierarchy usable, 200 tree spheres, estimate off
    {
        Host h = tree_scene();
        h.a_ms = 2.0;
        h.b_ms = 6.0;                  // (they arrive when waited for)
        h.call(20, true);
        bool ok = h.log.size() == 5 && h.asked == 0 && h.asked_blocking == 1 &&
                  is(h.log[0], Form::Walk, 1, false, true, -1, -1, true) && is(h.log[1], Form::Walk, 2, false, true, 0, 1, true) &&
                  is(h.log[2], Form::Sweep, 1, false, true, -1, -1, true) && is(h.log[3], Form::Sweep, 2, false, true, 2, 3, true) &&
                  is(h.log[4], Form::Walk, 14, true, false, -1, -1, false);
        ok = ok && h.ch.bvh_pick == Form::Walk && !h.ch.pick_estimated && h.ch.probe_ms[0] == 1.0 && h.ch.probe_ms[1] == 3.0 && h.ch.probe_tree == 200;
        check("blocking_call_splits_1_2_1_2", ok, "not walk 1, walk 2, sweep 1, sweep 2 in natural order and 14 passes of the verdict");

        Host q = tree_scene();
        const int passes[5] = { 1, 1, 2, 3, 13 };
        for (int p : passes) q.call(p, false);
        ok = q.log.size() == 5 && q.asked == 1 &&
             is(q.log[0], Form::Walk, 1, false, true, -1, -1, true) && is(q.log[1], Form::Walk, 1, false, true, 0, 1, true) &&
             is(q.log[2], Form::Sweep, 2, false, true, -1, -1, true) && is(q.log[3], Form::Sweep, 3, false, true, 2, 3, true) &&
             is(q.log[4], Form::Walk, 13, false, false, -1, -1, false);                 // four steps queued, no times: Walk, unpriced
        ok = ok && q.ch.samples[0] == 1 && q.ch.samples[1] == 3 && q.ch.bvh_pick == Form::Auto && q.ch.which == Choice::WalkVsSweep;
        q.call(20, true);               // (a blocking call that finds the steps queued does not wait either)
        ok = ok && q.log.size() == 6 && q.asked_blocking == 0 && is(q.log[5], Form::Walk, 20, false, false, -1, -1, false);
        check("one_step_per_non_blocking_launch", ok, "not a step per launch, then Walk unpriced while the times are out");
    }
    // 7. the walk dead band: 5 % towards the hierarchy
    {
        Host lo = tree_scene_measured(200, 1.04, 1.0), hi = tree_scene_measured(200, 1.06, 1.0);
        check("walk_dead_band", lo.ch.bvh_pick == Form::Walk && lo.log.back().form == Form::Walk && lo.log.back().priced && hi.ch.bvh_pick == Form::Sweep &&
              hi.log.back().form == Form::Sweep && hi.ch.probe_ms[0] == 1.06 && hi.ch.probe_ms[1] == 1.0 && rt::verdict_number(hi.ch.bvh_pick) == 2,
              "1.04 x is not Walk or 1.06 x not Sweep");
    }
    // 8. the estimate: (18.7 P + 8.9 always) / (n + 17.9), n = 200, always = 0
    {
        Host walk = tree_scene(200, true), sweep = tree_scene(200, true), band = tree_scene(200, true), none = tree_scene(200, true);
        walk.ch.tree_uploaded(true, 2.0, 8.0);          // 0.17
        sweep.ch.tree_uploaded(true, 20.0, 60.0);       // 1.72
        band.ch.tree_uploaded(true, 11.0, 30.0);        // 0.94
        none.ch.tree_uploaded(false, 0.0, 0.0);
        for (Host *h : { &walk, &sweep, &band, &none }) h->call(20, false);
        bool ok = walk.log.size() == 1 && is(walk.log[0], Form::Walk, 20, true, false, -1, -1, false) && walk.ch.pick_estimated && walk.ch.bvh_pick == Form::Walk &&
                  walk.ch.probe_ms[0] == 0.0 && walk.ch.probe_ms[1] == 0.0 && walk.ch.est_ratio > 0.17 && walk.ch.est_ratio < 0.18 && walk.ch.state == 0;
        ok = ok && sweep.log.size() == 1 && is(sweep.log[0], Form::Sweep, 20, true, false, -1, -1, false) && sweep.ch.pick_estimated && sweep.ch.probe_ms[1] == 0.0 &&
             sweep.ch.est_ratio > 1.71 && sweep.ch.est_ratio < 1.72;
        ok = ok && is(band.log[0], Form::Walk, 20, false, true, -1, -1, true) && band.ch.bvh_pick == Form::Auto && !band.ch.pick_estimated && band.ch.state == 1 &&
             band.ch.est_ratio > 0.94 && band.ch.est_ratio < 0.95;
        ok = ok && is(none.log[0], Form::Walk, 20, false, true, -1, -1, true) && none.ch.bvh_pick == Form::Auto && none.ch.state == 1 && none.ch.est_ratio == 0.0;
        check("estimate_decides_outside_its_band", ok, "a clear ratio did not decide in one launch, or one inside the band (or none) did not measure");
    }
    // 9. cases that ask nothing
    {
        Host big = tree_scene(1500, true), wide = tree_scene(200, true), twelve = small_scene(12);
        big.ch.tree_uploaded(true, 2.0, 8.0);
        wide.ch.tree_uploaded(true, 2.0, 8.0);
        wide.f.tables_fit = false;
        for (Host *h : { &big, &wide, &twelve }) { h->frame(40); h->frame(40); h->call(1, false); }
        bool ok = true;
        for (Host *h : { &big, &wide, &twelve }) {
            ok = ok && h->log.size() == 3 && h->asked == 0 && h->asked_blocking == 0 && h->ch.which == Choice::None && h->ch.state == 0 &&
                 rt::verdict_number(h->ch.bvh_pick) == 0 && h->ch.coop_pick == Form::Auto;
            for (const Launch &l : h->log) ok = ok && l.form == (h == &twelve ? Form::Sweep : Form::Walk) && l.priced && !l.natural && !l.step && l.before == -1;
        }
        check("nothing_asked_where_the_answer_is_known", ok, "1500 tree spheres, tables beyond LDS or 12 spheres without a hierarchy asked something");
    }
    // 10. after a verdict measured on a tree of 100 spheres: device-resident updates
    {
        Host keep = tree_scene_measured(100, 1.0, 2.0, true), moved = tree_scene_measured(100, 1.0, 2.0, true), many = tree_scene_measured(100, 1.0, 2.0, true),
             lost = tree_scene_measured(100, 1.0, 2.0, true);
        bool ok = keep.ch.bvh_pick == Form::Walk && keep.ch.probe_tree == 100 && keep.ch.est_valid;
        keep.ch.tables_rebuilt(true, 127, 0);           // 4 * 27 = 108 is not more than 100 + 8
        ok = ok && keep.ch.bvh_pick == Form::Walk && keep.ch.state == 4 && keep.ch.est_valid && keep.ch.probe_updates == 1 && keep.ch.probe_tree == 100;
        moved.ch.tables_rebuilt(true, 128, 0);          // 4 * 28 = 112 is
        ok = ok && moved.ch.bvh_pick == Form::Auto && moved.ch.state == 0 && moved.ch.which == Choice::None && !moved.ch.est_valid;
        for (int k = 0; k < 255; ++k) many.ch.tables_rebuilt(true, 100, 0);
        ok = ok && many.ch.bvh_pick == Form::Walk && many.ch.probe_updates == 255;
        many.ch.tables_rebuilt(true, 100, 0);
        ok = ok && many.ch.bvh_pick == Form::Auto && many.ch.probe_updates == 0 && !many.ch.est_valid;
        lost.ch.tables_rebuilt(false, 0, 0);
        ok = ok && lost.ch.bvh_pick == Form::Auto && lost.ch.state == 0 && lost.ch.est_valid;      // (the estimate is voided only with a tree in hand)
        Host during = small_scene(), after = small_scene_measured();
        for (int k = 0; k < 20; ++k) during.call(1, false);
        during.ch.tables_rebuilt(false, 0, 0);
        ok = ok && during.ch.which == Choice::CoopVsPlain && during.ch.state == 3 && during.ch.acc == 2 && during.ch.scene_launches == 20;
        after.times_in = true;
        after.a_ms = 10.0;
        after.b_ms = 16.0;
        after.call(1, false);
        after.ch.tables_rebuilt(true, 300, 0);
        ok = ok && after.ch.coop_pick == Form::SweepCoop && after.ch.state == 4 && after.ch.scene_launches == 35;
        check("updates_keep_the_verdict_until_the_tree_moved", ok, "127 / 128 of 100, the 256th update, a lost tree or the coop measurement");
    }
    // 11. a new scene or a knob set by hand: what goes and what stays
    {
        Choice first;
        bool ok = true;
        for (int how = 0; how < 4; ++how) {
            Host h = tree_scene_measured(100, 1.0, 2.0, true);
            h.ch.follow(&first);
            h.ch.est_ratio = 0.9;
            h.ch.frame_ended();
            h.ch.coop_pick = Form::SweepPlain;          // (by hand: a context has one verdict or the other)
            h.ch.acc = 3;
            if (how == 0) h.ch.new_scene();
            else if (how == 1) h.ch.knob_set();
            else if (how == 2) h.ch.estimate_switched(false);
            else h.ch.coop_threshold_set_by_hand();
            ok = ok && h.ch.bvh_pick == Form::Auto && h.ch.coop_pick == Form::Auto && !h.ch.pick_estimated && h.ch.probe_ms[0] == 0.0 && h.ch.probe_ms[1] == 0.0 &&
                 h.ch.scene_frames == 0 && h.ch.scene_launches == 0 && h.ch.state == 0 && h.ch.acc == 0 && h.ch.which == Choice::None && h.ch.probe_updates == 0;
            ok = ok && h.ch.last == Form::Walk && h.ch.leader == &first && h.ch.use_estimate == 0 && h.ch.coop_probe == (how == 3 ? 0 : 1) && h.ch.est_ratio == 0.9 &&
                 h.ch.est_valid;
        }
        check("new_scene_and_knobs_clear_the_verdicts_only", ok, "something stayed that goes, or went that stays");
    }
    // 12. a follower renders what its leader's last launch was and opens nothing
    {
        Choice first;
        bool ok = true;
        const Form lasts[4] = { Form::Auto, Form::Walk, Form::SweepCoop, Form::SweepPlain };
        for (Form last : lasts) {
            first.launch_queued(last);
            Host tree = tree_scene(), small = small_scene();
            tree.ch.follow(&first);
            small.ch.follow(&first);
            tree.call(20, true);
            tree.call(1, false);
            small.frame(40);
            small.frame(40);
            small.call(1, false);
            const Form want_tree = last == Form::SweepCoop || last == Form::SweepPlain ? Form::Sweep : Form::Walk;
            const Form want_small = last == Form::SweepCoop ? Form::SweepCoop : Form::SweepPlain;
            ok = ok && tree.log.size() == 2 && tree.all(0, 2, want_tree) && small.log.size() == 3 && small.all(0, 3, want_small);
            for (Host *h : { &tree, &small }) {
                ok = ok && h->asked == 0 && h->asked_blocking == 0 && h->ch.state == 0 && h->ch.which == Choice::None;
                for (const Launch &l : h->log) ok = ok && l.priced && !l.step && !l.natural && l.before == -1 && l.after == -1;
            }
        }
        check("a_follower_follows", ok, "a shard with a leader did not render its leader's last form, or opened a step");
    }
    // 13. frame_ended counts only when something of the scene was launched
    {
        Choice ch;
        ch.frame_ended();
        ch.frame_ended();
        bool ok = ch.scene_frames == 0;
        ch.launch_queued(Form::SweepPlain);
        ch.frame_ended();
        ch.frame_ended();
        ok = ok && ch.scene_frames == 2 && ch.scene_launches == 1;
        ch.new_scene();
        ch.frame_ended();
        ok = ok && ch.scene_frames == 0;
        ch.subset_launch_queued(Form::Walk);
        ch.frame_ended();
        check("frame_ended_counts_launched_frames", ok && ch.scene_frames == 1 && ch.last == Form::Walk, "a reset without a launch counted, or one after a launch did not");
    }
    // the diagnostics short-cut and a call with nothing to render measure nothing
    {
        Host forced = tree_scene(), nothing = tree_scene();
        forced.f.diagnostics = true;
        nothing.f.nothing_to_render = true;
        forced.call(20, true);
        nothing.call(0, true);
        check("diagnostics_and_empty_calls_measure_nothing", is(forced.log[0], Form::Auto, 20, false, false, -1, -1, false) && forced.ch.state == 0 &&
              is(nothing.log[0], Form::Sweep, 0, true, false, -1, -1, false) && nothing.ch.state == 0 && forced.log.size() == 1 && nothing.log.size() == 1,
              "a forced walk or an empty call opened a step");
    }
    if (g_failed == 0) printf("choice: clean\n");
    return g_failed;
}
