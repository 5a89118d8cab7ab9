"""The shadow of tests/_frame_shadow.py checked without a device, so that a mistake in the shadow or in a script of
tests/test_gpu_frame_sequences.py is found here and not on a GPU.
1. Against the real header: every script runs with a cast that, instead of calling the device, writes down the events each API call is
   supposed to report to csrc/rt_frame_state.h's FrameState -- the "reported by" column of DESIGN.md section 5.10, in the order the call sites
   report them -- and a small C++ program over the header (g++, as tests/test_frame_state_cpu.py) applies them.  After every call the record and
   the shadow must agree on the pass number, ragged, have_selection, the counts, the launch count and whether the call was refused (what
   rt_render_async refuses is the record's `ragged`; what rt_render_tiles_async refuses, its `have_selection`).  The seed and pixel flags are
   held to what they MEAN (Buffers): the seed buffer the record points the next launch at holds the context's seeds, and pixels_current is
   never set over a packed frame that is stale.  The program restates the call sites' few conditions by hand (launch_tiles' copy of the
   default stream, the merge's choice of kernel); the device tests are what holds the call sites themselves.
2. Against the straight oracle: a ragged sequence through the shadow gives, per tile, the straight render at that tile's count; a whole merge
   through the shadow is merge_restated of straight planes."""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import test_tiles_cpu as T
from _frame_shadow import ACCEPTED, H, W, Actor, Shadow, assert_straight, marked_map, per_pixel
from test_gpu_frame_sequences import SCRIPTS, ragged
from test_gpu_state import bits, merge_restated, oracle, pack
from test_gpu_tiles import S1, S3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One line per API call: `<context> <call> <arguments>`; one line out: the record's fields and the code the call site would return.
# What a call reports, and on what condition, is read off the call sites: rt_api.hip (rt_reset, rt_reset_async, rt_render_async,
# refresh_pixels), rt_state.hip (rt_seed_stream_async, write_one, rt_merge_async), rt_tiles.hip (rt_select_tiles, merge_by_tile),
# rt_launch.hip (launch_form, launch_tiles), rt_denoise.hip.
PROGRAM = r'''
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "rt_frame_state.h"

struct Ctx { rt::FrameState f; bool store = true; };

int main() {
    std::map<std::string, Ctx> cast;
    const unsigned groups = 6, tiles = 18;                  // 41 x 23
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string who, call;
        in >> who >> call;
        Ctx &c = cast[who];
        rt::FrameState &f = c.f;
        int rc = 0, n = 0;
        if (call == "render_async" || call == "render_pass") {
            in >> n;
            if (f.ragged) rc = -5;
            else if (n < 0) rc = -1;
            else if (n > 0) { f.launched(n, c.store); if (call == "render_pass") f.timed(1.0); }
        } else if (call == "reset") f.reset_blocking();
        else if (call == "reset_async") f.reset_in_place();
        else if (call == "seed_stream") { in >> n; f.reset_in_place(); if (n != 0) f.custom_seeds_written(); }
        else if (call == "write_state") { int with_seeds; in >> n >> with_seeds; f.state_written(n, with_seeds != 0); }
        else if (call == "set_pixel_write") { in >> n; c.store = n != 0; }
        else if (call == "select") { unsigned g, t; in >> g >> t; f.selection_started(); f.selection_landed(g, t); }
        else if (call == "render_tiles_async") {
            in >> n;
            if (n < 0) rc = -1;
            else if (!f.have_selection) rc = -5;
            else if (n > 0 && f.counts[0] != 0) {
                if (f.list_is_stale(false, tiles)) f.list_built(false, tiles, (f.counts[1] + 5) / 6 * 6);
                const bool all = f.counts[0] == groups;
                if (f.seeds_default && !all) f.default_seeds_copied();
                f.launched_subset(n, c.store, all);
            }
        } else if (call == "merge") {
            long long total = f.current_sample > 0 ? f.current_sample : 0;
            bool ragged = f.ragged;
            std::string src;
            while (in >> src) { const rt::FrameState &s = cast[src].f; if (s.current_sample > 0) total += s.current_sample; ragged = ragged || s.ragged; }
            if (total == 0) rc = -5;
            else if (ragged) f.merged_by_tile((int)total);
            else f.merged((int)total);
        } else if (call == "denoise") f.colours_replaced();
        else if (call == "pack") { if (!f.pixels_current && f.current_sample > 0) f.pixels_packed(); }
        else { printf("unknown call %s\n", call.c_str()); return 2; }
        printf("%d %d %d %u %u %llu %d %d %d %d\n", f.current_sample, (int)f.ragged, (int)f.have_selection, f.counts[0], f.counts[1], (unsigned long long)f.launches, rc,
               (int)f.seeds_default, (int)f.seeds_custom, (int)f.pixels_current);
    }
    return 0;
}
'''


class OnRecord(Actor):
    """The cast that writes the record's input: `log` collects (line, what the shadow expects the record to answer, what the call did to the
    shadow's buffers -- for Buffers below)."""

    def __init__(self, key, log, diag=False):                # (diag: which library the device's cast binds; there is none here)
        super().__init__(key)
        self.log = log

    def _note(self, line, code, call, **did):
        sh = self.sh
        self.log.append((line, sh.facts() + (code,), dict(did, key=self.key, call=call, colors=sh.colors.copy(), seeds=sh.seeds.copy(), cur=sh.cur,
                                                          rendered=sh.rendered(), store=sh.pixel_write)))

    def _perform(self, call, args, got, left_out, read_pixels):
        did, before = {}, self._before
        if call == "select":
            text = "%d %d" % self.sh.counts                  # (what the device's kernel reports: tests/test_gpu_tile_kernels.py holds it to the restatement)
        elif call in ("write_state", "load_state"):
            with_seeds = isinstance(args[0], Actor) or args[1] is not None
            call, text, did = "write_state", "%d %d" % (self.sh.cur, with_seeds), {"seeds_written": with_seeds}
        elif call == "merge":
            text = " ".join(s.key for s in args[0])
        elif call == "denoise":
            text = ""
        else:
            text = " ".join(str(int(a)) for a in args)
        if call in ("render_async", "render_pass", "render_tiles_async") and self.sh.launches > before[5]:       # a launch was queued
            every = call != "render_tiles_async" or self.sh.counts[0] == self.sh.ty * self.sh.gx
            did = {"launched": np.ones((H, W), bool) if every else per_pixel(T.tiles_of(self.sh.mask, W, H)), "every": every}
        self._note("%s %s %s" % (self.key, call, text), 0 if got == ACCEPTED else got, call, **did)
        if read_pixels:                                       # check() reads the packed frame on the device: refresh_pixels
            self._packs()

    def _step(self, call, *a, **kw):
        self._before = self.sh.facts()
        super()._step(call, *a, **kw)

    def _packs(self):
        self._note("%s pack" % self.key, 0, "pack")

    def compare(self, other):
        self._packs()
        other._packs()

    def read_pixels_async(self):
        self._packs()

    def counters(self, want):                                 # (the device's counters against the oracle's: nothing the record holds)
        pass

    def tile_list(self, mask):                                # (the diagnostics library's list read back: likewise)
        pass


class Buffers:
    """What a context's two device buffers HOLD, followed through a script from what each call does to them -- the seed buffer a launch writes
    (the pristine default stream lies beside it) and the packed pixels -- so that the record's flags can be held to their meaning and not to a
    restatement of themselves: after every call, the buffer `seeds_default` points the next launch at holds the seeds the shadow says the
    context has, and where `pixels_current` is set the pixel buffer holds the pack of the shadow's plane on every tile that holds a pass.
    (pixels_current may be false over a frame that happens to be current: that costs a pack, not a wrong frame.)"""

    def __init__(self):
        self.default = O.seeds(W, H)
        self.d_seeds, self.d_pixels = self.default.copy(), np.zeros((H, W), np.uint32)       # as rt_create's restore kernel leaves them
        self.flags = (0, 0, 1)                               # seeds_default, seeds_custom, pixels_current of a fresh record

    def apply(self, did, flags_after):
        sd_before, _, px_before = self.flags
        call, packed = did["call"], pack(did["colors"], W, H).reshape(H, W)
        if call == "reset":
            self.d_seeds, self.d_pixels = self.default.copy(), np.zeros((H, W), np.uint32)
        elif call == "seed_stream" and not np.array_equal(did["seeds"], self.default):
            self.d_seeds = did["seeds"].copy()
        elif call == "write_state" and did["seeds_written"]:
            self.d_seeds = did["seeds"].copy()
        elif "launched" in did:
            m = did["launched"]
            if sd_before and not did["every"]:               # default_seeds_copied: the copy rt_reset makes, made now
                self.d_seeds = self.default.copy()
            self.d_seeds.reshape(H, W, 2)[m] = did["seeds"].reshape(H, W, 2)[m]
            if did["store"]:
                self.d_pixels[m] = packed[m]
        elif call == "pack" and not px_before and did["cur"] > 0:
            self.d_pixels = packed.copy()
        self.flags = flags_after
        sd, _, px = flags_after
        assert np.array_equal(self.default if sd else self.d_seeds, did["seeds"]), "the next launch would read other seeds than the context has"
        if px and did["cur"] > 0:
            m = did["rendered"]
            assert np.array_equal(self.d_pixels[m], packed[m]), "pixels_current is set over a stale frame"


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frame_shadow")
    src, exe = tmp / "record.cpp", tmp / "record"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "raytracing_simple_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


@pytest.mark.parametrize("script", SCRIPTS, ids=[s.__name__[7:] for s in SCRIPTS])
def test_the_record_and_the_shadow_agree_after_every_call_of_a_script(script, record):
    log = []
    script(lambda key, **kw: OnRecord(key, log, **kw))
    assert len(log) >= 4
    got = record([line for line, _, _ in log])
    assert len(got) == len(log)
    buffers = {}
    for step, ((line, want, did), answer) in enumerate(zip(log, got)):
        said = tuple(int(v) for v in answer.split())
        where = "step %d, `%s`: the record says %s (pass, ragged, selection, groups, tiles, launches, code; seeds_default, seeds_custom, pixels_current)" % (step, line, answer)
        assert said[:7] == want, where
        try:
            buffers.setdefault(did["key"], Buffers()).apply(did, said[7:])
        except AssertionError as e:
            raise AssertionError("%s -- %s" % (where, e))


def test_the_scripts_together_make_every_call_and_meet_refusals():
    """Together the scripts report every event of the table a plain context can meet (not the diagnostics reset, not the multi-device front)."""
    log = []
    for script in SCRIPTS:
        script(lambda key, **kw: OnRecord(key, log, **kw))
    calls = {line.split()[1] for line, _, _ in log}
    assert calls == {"render_async", "render_pass", "reset", "reset_async", "seed_stream", "write_state", "set_pixel_write", "select",
                     "render_tiles_async", "merge", "denoise", "pack"}
    assert {want[-1] for _, want, _ in log} == {0, -5}           # accepted calls, and RT_ERR_STATE refusals


# ---- the shadow against the straight oracle ------------------------------------------------------------------------------------
def test_a_ragged_sequence_through_the_shadow_is_the_straight_render_per_tile():
    class Alone(Actor):
        def _perform(self, *a):
            pass
    x = Alone("x")
    ragged(x)
    sh = x.sh
    assert sh.cur == 7 and sh.launches == 4 and sh.samples == int((np.repeat(np.repeat(sh.passes, 8, 0), 8, 1)[:H, :W]).sum())
    assert sh.pure.all()
    assert_straight(sh, sh.colors, sh.seeds, sh.pixels())
    # ... and without the `pure` bookkeeping: tile by tile, the bits of oracle(p)
    for p in (2, 3, 6, 7):
        want = oracle("demo", W, H, p)
        m = np.repeat(np.repeat(sh.passes == p, 8, 0), 8, 1)[:H, :W]
        assert m.any()
        assert np.array_equal(bits(sh.colors).reshape(H, W, 3)[::-1][m], bits(want["colors"]).reshape(H, W, 3)[::-1][m])
        assert np.array_equal(sh.seeds.reshape(H, W, 2)[m], want["seeds"].reshape(H, W, 2)[m])
        assert np.array_equal(sh.pixels().reshape(H, W)[m], want["pixels"].reshape(H, W)[m])
    # a subset on another stream after an in-place reset: the tiles left out hold the stream's first seeds, a cleared plane (an old frame stood
    # there) and 0 passes -- a 0-pass render
    old = sh.colors.copy()
    assert sh.seed_stream(5) == ACCEPTED and sh.select(marked_map(S3, None), 0) == ACCEPTED and sh.render_tiles_async(2) == ACCEPTED
    assert sh.left_out() == 880 and sh.samples == 2 * 63
    assert_straight(sh, sh.colors, sh.seeds, sh.pixels())
    out = ~np.repeat(np.repeat(sh.passes > 0, 8, 0), 8, 1)[:H, :W]
    assert out.sum() == 880 and bits(old).reshape(H, W, 3)[::-1][out].any() and not bits(sh.colors).reshape(H, W, 3)[::-1][out].any()
    assert bits(sh.colors).reshape(H, W, 3)[::-1][~out].any()


def test_a_whole_merge_through_the_shadow_is_merge_restated_of_straight_planes():
    shadows = [Shadow() for _ in range(3)]
    for k, (sh, n) in enumerate(zip(shadows, (3, 5, 2))):
        assert sh.seed_stream(k + 1) == ACCEPTED and sh.render_async(n) == ACCEPTED
    dst = shadows[0]
    seeds = dst.seeds.copy()
    assert dst.select(marked_map(S1, None), 0) == ACCEPTED
    assert dst.merge(shadows[1:]) == ACCEPTED
    want = merge_restated([oracle("demo", W, H, n, k + 1)["colors"] for k, n in enumerate((3, 5, 2))], (3, 5, 2))
    assert dst.cur == 10 and not dst.ragged and not dst.have_selection and np.array_equal(bits(dst.colors), bits(want))
    assert np.array_equal(dst.seeds, seeds) and np.all(dst.passes == 10)
    # refusals leave the shadow as it was
    before = dst.facts(), dst.colors.copy()
    assert dst.render_tiles_async(1) == -5 and dst.render_async(-1) == -1 and dst.write_state(None, None, 3) == -1
    assert Shadow().merge([Shadow()]) == -5
    assert dst.facts() == before[0] and np.array_equal(bits(dst.colors), bits(before[1]))
