"""The refusals of the calls that read or consume a context's derived planes (csrc/rt_internal.h: plane_view, read_plane, filter_input,
ragged_refuse), word for word: the five rt_read_* calls on a context that holds no such plane and with no buffer, and rt_reproject_async and
rt_atrous_async without an input and on a ragged frame.  The expected texts are the ones the calls carried while each stated its own, copied from
those sources; every refusal is followed by one successful read of a plane that is current, against the bits it held before.  The logic is the
host's and does not depend on the frame's size: 8x8 contexts of the Demo scene (one tile), 40x8 (two groups) where a group has to be left out."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library first touches the device, as in tests/test_gpu_denoise.py)

from raytracing_simple_amd import api, host
from test_gpu_feature_planes import context
from test_gpu_state import RT_ERR_ARG, RT_ERR_STATE
from test_gpu_tiles import select

pytestmark = pytest.mark.gpu

NO_PLANE = {
    "read_features": "rt_read_features: the context holds no current feature plane (rt_features_async forms one; rt_set_scene, rt_update_spheres_async and "
                     "rt_set_camera end it)",
    "read_filtered": "rt_read_filtered: the context holds no current cross-filtered plane (rt_denoise_pair_async makes one; whatever moves the colour plane ends it)",
    "read_temporal": "rt_read_temporal: the context holds no current temporal plane (rt_reproject_async forms one; whatever moves the colour plane or ends the "
                     "feature plane ends it)",
    "read_moments": "rt_read_moments: the context holds no current moments plane (rt_reproject_async into it forms one while rt_set_temporal_moments is on; "
                    "whatever ends the temporal plane, or a reprojection into the context with the setting off, ends it)",
    "read_atrous": "rt_read_atrous: the context holds no current filtered plane (rt_atrous_async forms one; whatever ends the temporal plane, a new "
                   "rt_reproject_async into the context or a feature plane formed again ends it)",
}
NO_BUFFER = {
    "rt_read_features": (1, "rt_read_features: out_host is null"),
    "rt_read_filtered": (1, "rt_read_filtered: out_host is null"),
    "rt_read_temporal": (2, "rt_read_temporal: both buffers are null"),
    "rt_read_moments": (1, "rt_read_moments: m_host is null"),
    "rt_read_atrous": (2, "rt_read_atrous: both buffers are null"),
}
RAGGED = "%s is ragged (its tiles hold different pass counts)"
NO_INPUT = "%s holds neither a current temporal plane nor a pass"


def demo(w, h):
    return context(host.demo_scene(), host.compute_camera(host.DEMO_ORIG, host.DEMO_TARGET, w, h), w, h)


def refused(code, text, call, *args):
    with pytest.raises(api.RtError) as e:
        call(*args)
    assert e.value.code == code
    assert str(e.value) == "rt status %d: %s" % (code, text)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_the_five_readers_refuse_a_plane_that_is_not_there_and_no_buffer():
    with demo(8, 8) as C, demo(8, 8) as N, demo(8, 8) as M:
        # C: passes and a feature plane, none of the other four
        C.render_async(2)
        C.features_async()
        feat = C.read_features()
        assert feat.any()
        for name in ("read_filtered", "read_temporal", "read_moments", "read_atrous"):
            refused(RT_ERR_STATE, NO_PLANE[name], getattr(C, name))
            assert same_bits(C.read_features(), feat)
        lib = C._lib
        for name, (buffers, text) in NO_BUFFER.items():
            assert getattr(lib, name)(C._h, *([None] * buffers)) == RT_ERR_ARG
            assert lib.rt_last_error().decode() == text
            assert same_bits(C.read_features(), feat)
        # N: a cross-filtered plane and no feature plane
        N.render_async(1)
        M.render_async(1)
        N.denoise_pair(M)
        filtered = N.read_filtered()
        refused(RT_ERR_STATE, NO_PLANE["read_features"], N.read_features)
        assert same_bits(N.read_filtered(), filtered)


def test_a_filter_without_an_input_is_refused():
    with demo(8, 8) as C, demo(8, 8) as E:
        C.render_async(2)
        C.features_async()
        E.features_async()                                   # a feature plane, no pass, no temporal plane
        feat_c, feat_e = C.read_features(), E.read_features()
        refused(RT_ERR_STATE, "rt_atrous_async: " + NO_INPUT % "the context", E.atrous_async)
        assert same_bits(E.read_features(), feat_e)
        refused(RT_ERR_STATE, "rt_reproject_async: " + NO_INPUT % "the source", C.reproject_async, E)
        assert same_bits(C.read_features(), feat_c) and same_bits(E.read_features(), feat_e)
        E.reproject_async(C)                                 # the other way round is a pure warp: E holds a temporal plane now, and is an input
        T = E.read_temporal(packed=False)
        C.reproject_async(E)
        E.atrous_async()
        assert same_bits(E.read_temporal(packed=False), T)


def test_a_ragged_frame_is_refused():
    with demo(40, 8) as R, demo(40, 8) as Q:
        for c in (R, Q):
            c.render_async(2, c.stream)
            c.features_async()
        assert select(R, np.array([[1, 0]], bool)) == (1, 4)     # the left group of two
        R.render_tiles_async(1, R.stream)
        feat = R.read_features()
        refused(RT_ERR_STATE, "rt_atrous_async: " + RAGGED % "the context", R.atrous_async)
        assert same_bits(R.read_features(), feat)
        refused(RT_ERR_STATE, "rt_reproject_async: " + RAGGED % "the destination", R.reproject_async, Q)
        assert same_bits(R.read_features(), feat)
        refused(RT_ERR_STATE, "rt_reproject_async: " + RAGGED % "the source", Q.reproject_async, R)
        refused(RT_ERR_STATE, NO_PLANE["read_temporal"], Q.read_temporal)     # (the refused call formed nothing)
        assert same_bits(R.read_features(), feat)
