"""Fast mode is an unbiased renderer where the 50 dB gate cannot speak: the mirror box and 256 random spheres at 64x48, the glass and
mirror scene of tests/test_gpu_parity.py at 41x23 -- the scenes where "fast against parity on the SAME random stream" is a strict xfail,
because a last-bit difference sends a path down another branch and two correct renderers then differ at the noise level.

The gate.  Parity mode renders seed streams 1, 2, 3, 4 and fast mode stream 5, PASSES passes each, the product library choosing the
instances.  D = the six rt_compare PSNRs among the parity frames, F = the four of the fast frame against each of them; asserted is
    min(F) >= min(D) - (max(D) - min(D)):
a fast frame is no further from an independent parity frame than independent parity frames are from each other.  The threshold is the
reference's own spread in the same run, not a figure of the code under test.

Its power, measured on the reference renderer itself (parity frames in the fast frame's place; the glass scene's also on the oracle in
tests/test_fast_reference_cpu.py).  At 4096 passes on an MI355X (profiles/HISTORY.md, r20):
    scene              D, dB            threshold   fast F, dB       glass diffuse   light x 1.02   light x 1.10
    mirror_box64       35.90 .. 36.25   35.55       35.89 .. 36.15   19.95 FAILS     35.47 FAILS    30.41 FAILS
    random256          44.62 .. 44.85   44.40       44.73 .. 44.93   33.01 FAILS     43.44 FAILS    36.06 FAILS
    glass_and_mirror   46.22 .. 47.76   44.67       48.05 .. 48.52   26.69 FAILS     47.30 passes   41.03 FAILS
So the gate sees a wrong material branch everywhere and a light 2 % too bright on the two 64x48 scenes.  On the glass-and-mirror scene
(943 pixels, caustics: the four parity frames spread by 1.5 dB) it does NOT see 2 % at a pass count a test can afford: on the oracle that
scene's gate first fails for 1.05 at 16384 passes and still passes 1.02 there.  There the precondition is 10 % (EMISSION below), and
the 2 % figure is printed.  The whole module takes about nine seconds at 4096 passes, a scene's five frames one to two; 16384 would
not change what the glass scene resolves, so PASSES stays 4096.  Run with -s for the figures."""
import time

import numpy as np
import pytest

import _fast_reference as R
from raytracing_simple_amd import api, host

pytestmark = pytest.mark.gpu
PASSES = 4096
SCENES = R.bias_scenes()
EMISSION = {"mirror_box64": 1.02, "random256": 1.02, "glass_and_mirror": 1.10}      # the scale of the light the gate must fail (docstring)


def _frame(spheres, cam, w, h, mode, stream):
    """-> an open context holding the frame (the caller closes it)"""
    ctx = api.RtContext(w, h)
    try:
        ctx.set_scene(spheres)
        ctx.set_camera(cam)
        ctx.set_mode(mode)
        ctx.seed_stream(stream)
        ctx.render_pass(PASSES)
    except Exception:
        ctx.close()
        raise
    return ctx


@pytest.fixture(scope="module", params=range(len(SCENES)), ids=[s[0] for s in SCENES])
def parity_frames(request):
    name, maker, w, h = SCENES[request.param]
    sph, orig, target = maker()
    cam = host.compute_camera(orig, target, w, h)
    t0 = time.time()
    ctxs = [_frame(sph, cam, w, h, api.RT_MODE_PARITY, s) for s in R.PARITY_STREAMS]
    among = [api.error_psnr(ctxs[i].compare(ctxs[j])) for i in range(4) for j in range(i + 1, 4)]
    print("%s %dx%d, %d passes: parity frames by %s in %.2f s; among them %s dB" % (
        name, w, h, PASSES, ctxs[0].last_kernel, time.time() - t0, ["%.2f" % v for v in among]))
    yield {"name": name, "spheres": sph, "cam": cam, "w": w, "h": h, "ctxs": ctxs, "among": among}
    for c in ctxs:
        c.close()


def _gate(pf, spheres, mode, label):
    with _frame(spheres, pf["cam"], pf["w"], pf["h"], mode, R.FAST_STREAM) as ctx:
        kernel = ctx.last_kernel
        against = [api.error_psnr(ctx.compare(c)) for c in pf["ctxs"]]
    ok, thr = R.bias_gate(pf["among"], against)
    print("%s, %s by %s: D %.2f .. %.2f dB, threshold %.2f, F %s -> %s" % (
        pf["name"], label, kernel, min(pf["among"]), max(pf["among"]), thr, ["%.2f" % v for v in against], "passes" if ok else "FAILS"))
    return ok, kernel


def test_fast_frame_is_as_close_to_parity_frames_as_they_are_to_each_other(parity_frames):
    ok, kernel = _gate(parity_frames, parity_frames["spheres"], api.RT_MODE_FAST, "fast mode")
    assert "_fast" in kernel, kernel
    assert ok


@pytest.mark.parametrize("bias", ["glass-turned-diffuse", "brighter-light"])
def test_gate_fails_a_biased_parity_frame(parity_frames, bias):
    """the preconditions of the gate's power, parity only: a biased parity frame in the fast frame's place must FAIL the assertion"""
    sph, scale = parity_frames["spheres"], EMISSION[parity_frames["name"]]
    biased = R.glass_turned_diffuse(sph) if bias == "glass-turned-diffuse" else R.brighter_light(sph, scale)
    ok, _ = _gate(parity_frames, biased, api.RT_MODE_PARITY, bias if bias == "glass-turned-diffuse" else "emission x %.2f" % scale)
    assert not ok
    if bias == "brighter-light" and scale != 1.02:          # what the gate does NOT resolve here: printed for the reader, not asserted
        _gate(parity_frames, R.brighter_light(sph, 1.02), api.RT_MODE_PARITY, "emission x 1.02 (below the gate's resolution on this scene)")


def test_gate_passes_an_honest_parity_frame(parity_frames):
    """a parity frame on the fast frame's stream: the gate does not fail what is unbiased"""
    ok, _ = _gate(parity_frames, parity_frames["spheres"], api.RT_MODE_PARITY, "parity mode, an independent stream")
    assert ok
