"""The first-hit frames of tests/test_gpu_fast_first_hit.py, proved without a GPU (tests/_first_hit.py): the ORACLE's one-pass frame of
every scene of that module, decoded and checked by the same function under K.exact(), must pass, with the share of pixels the exclusion
rule leaves out inside the 2 % cap -- the reference, the decoding and the choice of scenes hold on their own --, and the same frame with
1 % of its decided pixels' indices replaced by a neighbour's must fail: the check sees a wrong winner.  Run with -s for the figures."""
import numpy as np
import pytest

import _first_hit as FH
import _oracle as O

F = np.float32


@pytest.fixture(scope="module", params=list(FH.SCENES))
def oracle_frame(request):
    name = request.param
    sph, cam = FH.scene(name)
    return name, O.render(sph, cam, FH.W, FH.H, 1, threads=16)["colors"], FH.reference(name, False)


def test_oracle_frame_decodes_to_binary64_s_first_hits(oracle_frame):
    name, colors, ref = oracle_frame
    out = FH.check_frame("oracle / " + name, colors, ref)
    assert out["excluded"] <= 0.02 * out["pixels"]


def test_a_frame_with_one_percent_of_its_winners_replaced_fails(oracle_frame):
    name, colors, ref = oracle_frame
    bad, n = FH.tampered(colors, ref)
    assert n >= 1
    with pytest.raises(AssertionError, match="another sphere wins"):
        FH.check_frame("tampered / " + name, bad, ref, verbose=False)


def test_the_encoding_round_trips_and_refuses_what_is_no_code():
    """every index of a 16 384-record table through one rounded product per channel at |n.d| from 1 down to the smallest normal number; zero,
    subnormal and non-finite channels and a quotient half a code off are refused"""
    i = np.arange(16384)
    for nd in (F(1.0), F(0.3), F(2.0 ** -20), F(1.7e-38)):
        c = np.stack([np.full(len(i), nd, F), nd * (F(1) + (i & 127).astype(F) / F(128)), nd * (F(1) + (i >> 7).astype(F) / F(128))], 1).astype(F)
        frame = np.zeros((FH.H * FH.W, 3), F)
        for a in range(0, len(i), len(frame)):
            part = c[a:a + len(frame)]
            frame[:len(part)] = part
            got = FH.decode(frame.reshape(FH.H, FH.W, 3)[::-1].reshape(-1))
            assert got["valid"][:len(part)].all() and np.array_equal(got["id"][:len(part)], i[a:a + len(part)]), nd
    frame = np.zeros((FH.H * FH.W, 3), F)
    frame[0] = (0.5, 0.0, 0.5)
    frame[1] = (2.0 ** -130, 2.0 ** -130, 2.0 ** -130)
    frame[2] = (np.nan, 1.0, 1.0)
    frame[3] = (0.5, 0.5 * (1 + 0.5 / 128), 0.5)
    frame[4] = (0.5, 1.0, 0.5)                           # (a code of 128: beyond the range)
    frame[5] = (0.5, 0.5, 0.5)
    got = FH.decode(frame.reshape(FH.H, FH.W, 3)[::-1].reshape(-1))
    assert got["hit"][:6].all() and not got["hit"][6:].any()
    assert got["valid"][:6].tolist() == [False, False, False, False, False, True] and got["id"][5] == 0
    assert FH.DECODE_MARGIN < 1e-4                        # against a whole unit between neighbouring codes
