"""Cross-filtering only the groups still rendering, without a device (include/rt_api.h rt_denoise_pair_tiles_async,
rt_render_adaptive_filtered_tiles): the symbols and bindings, the refusals that come before any device call, and the piece of the frame
record the feature adds (csrc/rt_frame_state.h: `filtered_behind`, the pair id a context's cross-filtered plane was current under when a
subset launch moved on), driven by a small C++ program over the header as tests/test_frame_state_cpu.py drives the rest of the record."""
import ctypes as C
import os
import subprocess

from raytracing_simple_amd import _build, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG = -1
SYMBOLS = ("rt_denoise_pair_tiles_async", "rt_render_adaptive_filtered_tiles")


def test_the_symbols_and_bindings_exist():
    assert sorted(api.SYMBOLS) == _build.declared_symbols("rt_api.h")
    lib = api.load_library()
    for name in SYMBOLS:
        assert name in api.SYMBOLS
        assert callable(getattr(lib, name))
    for name in ("denoise_pair_tiles", "render_adaptive_filtered_tiles"):
        assert callable(getattr(api.RtContext, name))


def test_every_refusal_that_needs_no_device():
    lib = api.load_library()
    other = C.c_void_p(8)                                    # never dereferenced: a null context is refused first
    err, n = api.FrameError(), C.c_int()
    for pair in ((None, other), (other, None), (None, None)):
        for rc in (lib.rt_denoise_pair_tiles_async(*pair, None, None),
                   lib.rt_render_adaptive_filtered_tiles(*pair, 28.0, 4, 4, 32, None, C.byref(err), C.byref(n)),
                   lib.rt_render_adaptive_filtered_tiles(*pair, 28.0, 4, 4, 32, C.byref(api.DenoiseParams(5, 1, 1.0, 0.45)), C.byref(err), None)):
            assert rc == RT_ERR_ARG and b"null" in lib.rt_last_error()
    # the parameters rt_denoise_async refuses, through the new loop: they are checked ahead of the contexts, so no context is needed
    nan, inf = float("nan"), float("inf")
    for field, value in (("search_radius", -1), ("search_radius", 9), ("patch_radius", -1), ("patch_radius", 3), ("alpha", -0.25), ("alpha", nan),
                         ("alpha", inf), ("k", 0.0), ("k", -1.0), ("k", nan), ("k", inf)):
        p = api.DenoiseParams(5, 1, 1.0, 0.45)
        setattr(p, field, value)
        assert lib.rt_render_adaptive_filtered_tiles(other, other, 28.0, 4, 4, 32, C.byref(p), C.byref(err), C.byref(n)) == RT_ERR_ARG
        assert field.encode() in lib.rt_last_error()
    assert n.value == 0 and err.as_dict()["pixels"] == 0     # nothing was written


PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "rt_frame_state.h"

using rt::FrameState;
static int bad = 0;
static void check(const char *what, bool ok) { if (!ok) { printf("%s\n", what); bad = 1; } }

// the cross-filtered planes of a pair, as rt_denoise_pair_tiles_async sorts them: 'c' current (nothing to refresh), 'b' one selection behind
// (refreshable), 's' stale for the call
static char state(const FrameState &a, const FrameState &b) { return a.filtered_with(b) ? 'c' : (a.filtered_behind_with(b) ? 'b' : 's'); }

struct Pair {
    FrameState a, b;
    unsigned long long calls = 0;
    void render(int n) { a.launched(n, true); b.launched(n, true); }
    void pair() { calls += 1; a.pair_filtered(calls); b.pair_filtered(calls); }
    void select(unsigned groups, unsigned tiles) { for (FrameState *f : { &a, &b }) { f->selection_started(); f->selection_landed(groups, tiles); } }
    // rt_render_tiles_async as launch_tiles reports it: nothing at all for an empty selection
    void subset(int n, unsigned of_groups) { for (FrameState *f : { &a, &b }) if (n > 0 && f->counts[0] != 0) f->launched_subset(n, true, f->counts[0] == of_groups); }
    void refresh() { calls += 1; a.pair_tiles_refreshed(calls); b.pair_tiles_refreshed(calls); }
    char is() const { return state(a, b); }
    // pair -> select -> subset launch: one selection behind
    static Pair behind() { Pair p; p.render(4); p.pair(); p.select(3, 10); p.subset(4, 6); return p; }
};

int main() {
    {   // pair -> select -> subset launch -> behind -> refresh -> current, and round again
        Pair p;
        check("fresh contexts hold no plane", p.is() == 's');
        p.render(4);
        check("rendered, never filtered", p.is() == 's' && p.a.filtered_behind == 0);
        p.pair();
        check("after the pair call: current", p.is() == 'c' && p.a.filtered_pair == 1 && p.a.filtered_behind == 0);
        p.select(3, 10);
        check("a selection moves no colour plane: still current", p.is() == 'c');
        p.subset(4, 6);
        check("a subset launch: behind, under the id the planes were current under", p.is() == 'b' && p.a.filtered_pair == 0 && p.a.filtered_behind == 1 && p.b.filtered_behind == 1);
        check("... and the frame is what a subset launch leaves", p.a.current_sample == 8 && p.a.ragged && p.a.have_selection && p.a.launches == 2);
        p.refresh();
        check("refreshed: current under a new id, the record of being behind dropped", p.is() == 'c' && p.a.filtered_pair == 2 && p.b.filtered_pair == 2 && p.a.filtered_behind == 0);
        p.select(2, 7);
        p.subset(4, 6);
        check("the next selection, rendered: behind the refresh call", p.is() == 'b' && p.a.filtered_behind == 2);
        p.refresh();
        check("... and current again", p.is() == 'c' && p.a.filtered_pair == 3);
    }
    {   // two subset launches of one selection stay behind, under the same id
        Pair p = Pair::behind();
        p.subset(2, 6);
        check("two subset launches of one selection", p.is() == 'b' && p.a.filtered_behind == 1 && p.a.current_sample == 10);
        p.subset(1, 6);
        check("three", p.is() == 'b' && p.a.filtered_behind == 1);
    }
    {   // every group selected: the frame stays whole, the planes are behind all the same
        Pair p; p.render(4); p.pair(); p.select(6, 18); p.subset(4, 6);
        check("every group selected", p.is() == 'b' && !p.a.ragged);
    }
    {   // an empty selection launches nothing: the planes stay current
        Pair p; p.render(4); p.pair(); p.select(0, 0); p.subset(4, 6);
        check("an empty selection leaves the planes current", p.is() == 'c' && p.a.current_sample == 4 && p.a.filtered_pair == 1);
        p.subset(0, 6);
        check("no pass to render either", p.is() == 'c');
    }
    // what comes in between and ends it: each on ONE context of a pair that was refreshable, and then on both
    struct { const char *what; void (*f)(FrameState &); } between[] = {
        { "a new selection", [](FrameState &f) { f.selection_started(); f.selection_landed(3, 10); } },
        { "a new selection that has not landed", [](FrameState &f) { f.selection_started(); } },
        { "a whole-frame launch", [](FrameState &f) { f.launched(1, true); } },
        { "rt_reset", [](FrameState &f) { f.reset_blocking(); } },
        { "rt_reset_async", [](FrameState &f) { f.reset_in_place(); } },
        { "rt_seed_stream_async", [](FrameState &f) { f.reset_in_place(); f.custom_seeds_written(); } },
        { "a merge into the context", [](FrameState &f) { f.merged(16); } },
        { "a per-tile merge into the context", [](FrameState &f) { f.merged_by_tile(16); } },
        { "rt_denoise_async into the context", [](FrameState &f) { f.colours_replaced(); } },
        { "a written state", [](FrameState &f) { f.state_written(8, true); } },
        { "a written state without seeds", [](FrameState &f) { f.state_written(8, false); } },
    };
    for (const auto &x : between) {
        Pair p = Pair::behind();
        x.f(p.a);
        if (p.is() != 's' || p.a.filtered_behind != 0 || p.b.filtered_behind != 1) { printf("%s on one context: still refreshable\n", x.what); bad = 1; }
        x.f(p.b);
        if (p.is() != 's' || p.b.filtered_behind != 0) { printf("%s on both contexts: still refreshable\n", x.what); bad = 1; }
        // ... and selecting and rendering again does not bring it back: only a whole-frame pair call does
        Pair q = Pair::behind();
        x.f(q.a);
        x.f(q.b);
        q.select(3, 10);
        if (q.a.current_sample > 0) q.subset(1, 6);
        if (q.is() != 's') { printf("%s, then a selection and a subset launch: refreshable again\n", x.what); bad = 1; }
        q.pair();
        if (q.is() != 'c') { printf("%s, then the pair call: not current\n", x.what); bad = 1; }
    }
    {   // the two contexts behind different pair calls
        Pair p = Pair::behind(), q = Pair::behind();
        q.calls = 7; q.render(0); q.pair(); q.select(3, 10); q.subset(4, 6);
        check("behind different calls", state(p.a, q.b) == 's' && p.a.filtered_behind == 1 && q.b.filtered_behind == 8);
    }
    {   // only one context subset-launched
        Pair p; p.render(4); p.pair(); p.select(3, 10);
        p.a.launched_subset(4, true, false);
        check("one context behind, the other current", p.is() == 's' && p.a.filtered_behind == 1 && p.b.filtered_pair == 1);
    }
    {   // the list of selected groups: once per selection
        FrameState f;
        check("no list before a selection", f.group_list_is_stale());
        f.selection_started(); f.selection_landed(3, 10);
        check("no list yet", f.group_list_is_stale());
        f.group_list_built();
        check("built", !f.group_list_is_stale());
        f.launched_subset(4, true, false);
        check("a launch of the same selection keeps it", !f.group_list_is_stale());
        f.selection_started(); f.selection_landed(3, 10);
        check("a new selection makes it stale", f.group_list_is_stale());
    }
    return bad;
}
'''


def test_the_frame_record_knows_when_the_planes_are_one_selection_behind(tmp_path):
    """pair -> select -> subset launch -> "behind" -> refresh -> current; two subset launches of one selection stay "behind"; a new selection, a
    whole launch, a reset, a seed stream, a merge or a filter into the context, or a written state in between -- on one context or on both -- is
    no longer refreshable, and stays so until a whole-frame pair call; an empty selection leaves the planes current."""
    src = tmp_path / "live_checks.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "live_checks"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
