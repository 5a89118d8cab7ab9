"""The scalar blocks and the shading steps of fast mode on the device, through tests/fast_probe.hip (the library's own inline functions,
built by this module with rt_kernel_fast.hip's flags and, as the control, with parity's): see tests/_fast_reference.py for the references,
the envelopes, the limit of the probe and what it cannot reach.

The control arm comes first: it must equal the oracle / the binary32 restatements bit for bit, or the probe is wired wrong and the fast
arm's results mean nothing -- the fast tests of a block then fail with that message.

Three bounds are MEASURED, not derived -- the ulp accuracy of v_rcp_f32 / v_rsq_f32 / v_sqrt_f32, the absolute error of v_sin_f32 /
v_cos_f32 with |sin^2 + cos^2 - 1|, and to_int's delta: profiles/r20_fast_blocks.jsonl holds the observed maximum of each and the input
that gave it (tools/measure_fast_blocks.py), and the tests assert twice that: room for another stepping of the same instruction, not
for another algorithm.  Run with -s for observed / bound."""
import ctypes as C

import numpy as np
import pytest

import _fast_reference as R
import _oracle as O

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
CONTROL = {}            # block -> None (bit-equal) or what differed


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    out = tmp_path_factory.mktemp("fast_probe")
    return {arm: R.Probe(R.build_probe(out, fast=(arm == "fast"))) for arm in ("fast", "control")}


@pytest.fixture(scope="module")
def measured():
    k = R.K.measured()
    if k is None or "to_int_delta" not in R.records() or "sincos_pythagoras" not in R.records():
        pytest.skip("not measured yet: profiles/r20_fast_blocks.jsonl has no record (tools/measure_fast_blocks.py writes it)")
    return k


@pytest.fixture(scope="module")
def inputs():
    return R.block_inputs()


EDGES = np.array([0.0, 2.0 ** -96, 2.0 ** -149, 2.0 ** -130, 2.0 ** -127, 3.4028234663852886e38, np.inf, np.nan], F)


def _control(probes, inputs, block):
    """None when the control arm reproduces the binary32 reference of `block` bit for bit (cached), else a description"""
    if block in CONTROL:
        return CONTROL[block]
    p = probes["control"]
    assert not p.fast
    bad = None
    with np.errstate(all="ignore"):
        def differs(name, got, want):
            same = R.bits_equal(got, want)
            return None if same.all() else "%s: %d of %d differ, first at input index %d" % (name, int((~same).sum()), same.size, int(np.argmin(same.reshape(-1))))
        if block == "sincos":
            u = (np.arange(0, 1 << 23, 64) / F(1 << 23)).astype(F)
            sn, cs = p.eval("sincos", u)
            ws, wc = R.sincos32(u)
            bad = differs("sine", sn, ws) or differs("cosine", cs, wc)
        elif block == "to_int":
            near, grid, edges = R.to_int_inputs()
            v = np.concatenate([near[::7], grid[::16], edges])
            lib = O.oracle()
            want = np.array([lib.orc_to_int(C.c_float(float(x))) for x in v], np.int32)
            bad = differs("to_int", p.eval("to_int", v)[0], want.view(F))
            g = v[(v >= 0) & (v <= 1)]
            bad = bad or differs("gamma", p.eval("gamma", g)[0], np.array([lib.om_gammaf(float(x)) for x in g], F))
        elif block == "roots":
            x = inputs
            bad = differs("rt_rcp", p.eval("rcp", np.concatenate([x["rcp"], EDGES]))[0], F(1) / np.concatenate([x["rcp"], EDGES]))
            bad = bad or differs("rt_div", p.eval("div", x["div_a"], x["div_b"])[0], x["div_a"] / x["div_b"])
            bad = bad or differs("rt_sqrt", p.eval("sqrt", np.concatenate([x["sqrt"], EDGES]))[0], np.sqrt(np.concatenate([x["sqrt"], EDGES])))
            for op in ("sqrt_unit", "sqrt_det"):            # (no range check in these two: their contract is 0 or >= 2^-96)
                bad = bad or differs(op, p.eval(op, x[op])[0], np.sqrt(x[op]))
            dd = np.concatenate([x["sq_len"], EDGES])
            root, inv = p.eval("sqrt_and_rcp", dd)
            bad = bad or differs("sqrt_and_rcp root", root, np.sqrt(dd)) or differs("sqrt_and_rcp reciprocal", inv, F(1) / np.sqrt(dd))
            a = _unit_inputs()
            bad = bad or differs("unit", p.eval("unit", a)[0], R.unit32(a))
        else:
            raise KeyError(block)
    CONTROL[block] = bad
    return bad


def _need_control(probes, inputs, block):
    bad = _control(probes, inputs, block)
    if bad:
        pytest.fail("the control arm of the probe does not reproduce parity arithmetic (%s): the probe is wired wrong, the fast arm's results mean nothing" % bad)


def _unit_inputs():
    rng = np.random.default_rng(11)
    return (R.log_uniform(rng, np.log2(1e-6), np.log2(1e4), 3 * 65536).reshape(-1, 3) * rng.choice([-1, 1], (65536, 3))).astype(F)


@pytest.mark.parametrize("block", ["sincos", "to_int", "roots"])
def test_control_arm_is_parity_arithmetic_bit_for_bit(probes, inputs, block):
    assert _control(probes, inputs, block) is None


def test_fast_sine_and_cosine_of_every_draw(probes, inputs, measured):
    """all 2^23 arguments u = k / 2^23 against sin(2 pi u), cos(2 pi u) in binary64"""
    _need_control(probes, inputs, "sincos")
    rec = R.records()
    u = (np.arange(1 << 23) / F(1 << 23)).astype(F)
    sn, cs = probes["fast"].eval("sincos", u)
    ang = 2.0 * np.pi * u.astype(D)
    e_sin, e_cos = np.abs(sn.astype(D) - np.sin(ang)).max(), np.abs(cs.astype(D) - np.cos(ang)).max()
    pyth = np.abs(sn.astype(D) ** 2 + cs.astype(D) ** 2 - 1.0).max()
    b_sin, b_cos, b_pyth = (2 * rec[k]["observed_max"] for k in ("v_sin_f32", "v_cos_f32", "sincos_pythagoras"))     # profiles/r20_fast_blocks.jsonl
    print("sin %.3g / %.3g   cos %.3g / %.3g   |sin^2 + cos^2 - 1| %.3g / %.3g" % (e_sin, b_sin, e_cos, b_cos, pyth, b_pyth))
    assert e_sin <= b_sin and e_cos <= b_cos and pyth <= b_pyth
    q = (np.arange(4) * (1 << 21)).astype(np.int64)                        # u = 0, 1/4, 1/2, 3/4: exact values
    assert sn[q].tolist() == [0.0, 1.0, 0.0, -1.0] and cs[q].tolist() == [1.0, 0.0, -1.0, 0.0]


def test_fast_to_int(probes, inputs, measured):
    _need_control(probes, inputs, "to_int")
    delta = 2 * R.records()["to_int_delta"]["observed_max"]                # profiles/r20_fast_blocks.jsonl
    near, grid, edges = R.to_int_inputs()
    lib = O.oracle()
    for name, v in (("near the 255 boundaries", near), ("every 1024th pattern of [0, 1]", grid), ("edges", edges)):
        got = probes["fast"].eval("to_int", v)[0].view(np.int32).astype(np.int64)
        want, dist = R.to_int64(v)
        assert (np.abs(got - want) <= 1).all(), name
        clear = dist > delta
        differ = got != want
        print("to_int, %s: %d of %d differ from binary64, the furthest %.3g from its boundary; delta %.3g" % (
            name, int(differ.sum()), len(v), float(dist[differ].max()) if differ.any() else 0.0, delta))
        assert np.array_equal(got[clear], want[clear]), name
        sub = np.nonzero(clear)[0][::7 if len(v) > 1000 else 1]            # the parity result on the same set (a seventh of it: one call each)
        parity = np.array([lib.orc_to_int(C.c_float(float(x))) for x in v[sub]], np.int64)
        assert np.array_equal(got[sub], parity), name
    # +-0, subnormals (v_log_f32 of a subnormal), the smallest normal -> 0; 1, 1 + ulp, 7.5, +inf -> 255; negatives, -inf, NaN -> 0
    got = probes["fast"].eval("to_int", edges)[0].view(np.int32)
    assert got.tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 255, 0, 0, 0, 255, 0, 0]


def test_fast_reciprocals_and_square_roots(probes, inputs, measured):
    """ulp error against binary64 over 2^20 log-uniform values per range; rt_div = a * v_rcp(b): the reciprocal's K ulps are at most
    2 K ulps of the quotient (an ulp is between 2^-24 and 2^-23 of its value) and the product rounds once more: 2 K + 0.5"""
    _need_control(probes, inputs, "roots")
    k, x, p = measured, inputs, probes["fast"]
    with np.errstate(all="ignore"):
        root, inv = p.eval("sqrt_and_rcp", x["sq_len"])
        seen = [("rt_rcp", R.ulp_error(p.eval("rcp", x["rcp"])[0], 1.0 / x["rcp"].astype(D)).max(), k.rcp),
                ("rt_div", R.ulp_error(p.eval("div", x["div_a"], x["div_b"])[0], x["div_a"].astype(D) / x["div_b"].astype(D)).max(), 2 * k.rcp + 0.5),
                ("sqrt_and_rcp root", R.ulp_error(root, np.sqrt(x["sq_len"].astype(D))).max(), k.sqrt),
                ("sqrt_and_rcp reciprocal", R.ulp_error(inv, 1.0 / np.sqrt(x["sq_len"].astype(D))).max(), k.rsq)]
        for op in ("sqrt", "sqrt_unit", "sqrt_det"):
            seen.append(("rt_" + op, R.ulp_error(p.eval(op, x[op])[0], np.sqrt(x[op].astype(D))).max(), k.sqrt))
    for name, got, bound in seen:
        print("%-24s %.3f ulp, bound %.3f" % (name, got, bound))
        assert got <= bound, name


def test_fast_blocks_at_the_edges(probes, inputs, measured):
    """0, 2^-96, subnormals, FLT_MAX, inf, NaN.  Never a NaN where parity returns a number.  The hardware forms may flush a subnormal
    operand or result to zero, so a subnormal gives 0 or the value: sqrt in [0, sqrt(x) (1 + 2^-20)], a reciprocal of 2^126 at least."""
    _need_control(probes, inputs, "roots")
    k, p = measured, probes["fast"]
    with np.errstate(all="ignore"):
        for op in ("sqrt", "sqrt_unit", "sqrt_det"):
            got = p.eval(op, EDGES)[0]
            assert not np.isnan(got[:7]).any() and np.isnan(got[7]), op
            assert got[0] == 0 and got[6] == np.inf, op
            assert R.ulp_error(got[[1, 5]], np.sqrt(EDGES[[1, 5]].astype(D))).max() <= k.sqrt, op
            assert ((got[2:5] >= 0) & (got[2:5].astype(D) <= np.sqrt(EDGES[2:5].astype(D)) * (1 + 2.0 ** -20))).all(), op
        got = p.eval("rcp", EDGES)[0]
        assert not np.isnan(got[:7]).any() and np.isnan(got[7])
        assert got[0] == np.inf and got[6] == 0 and (got[2:5] >= F(2.0 ** 126)).all()
        assert R.ulp_error(got[1:2], 1.0 / EDGES[1:2].astype(D)).max() <= k.rcp
        assert 0 <= got[5] <= F(2.0 ** -127)                                  # 1 / FLT_MAX is a subnormal: itself or zero
        root, inv = p.eval("sqrt_and_rcp", EDGES)
        assert not np.isnan(root[:7]).any() and not np.isnan(inv[:7]).any() and np.isnan(root[7]) and np.isnan(inv[7])
        assert inv[0] == np.inf and inv[6] == 0 and (inv[2:5] >= F(2.0 ** 63)).all()
        assert R.ulp_error(inv[[1, 5]], 1.0 / np.sqrt(EDGES[[1, 5]].astype(D))).max() <= k.rsq


def test_fast_unit_vectors(probes, inputs, measured):
    """components spanning 1e-6 .. 1e4; the bound is the running error of a.a, v_rsq_f32 and the three products
    (about (2.5 + 2 K_rsq) 2^-24 of the length)"""
    _need_control(probes, inputs, "roots")
    a = _unit_inputs()
    got = probes["fast"].eval("unit", a)[0]
    want = R.e_unit(R.e_vec(a), measured)
    ratio = max(float((np.abs(got[:, c].astype(D) - want[c].v) / want[c].e).max()) for c in range(3))
    length_bound = np.sqrt(sum((np.abs(want[c].v) + want[c].e) ** 2 for c in range(3))) - 1.0
    off = np.abs(np.linalg.norm(got.astype(D), axis=1) - 1.0)
    print("unit(): observed / bound %.3f; largest | |unit(a)| - 1 | %.3g, allowed %.3g" % (ratio, off.max(), length_bound.max()))
    assert ratio <= 1.0 and (off <= length_bound).all()


@pytest.mark.parametrize("what", [0, 1, 2, 3, 4], ids=["camera", "bounce", "hit-record", "glass", "light"])
def test_fast_shading_steps(probes, inputs, measured, what):
    """every output within the running-error bound of the operations that form it (tests/_fast_reference.py shade64 writes each line
    out), decisions equal to binary64's away from their ties; directions of unit length within unit()'s bound"""
    _need_control(probes, inputs, "roots")
    _need_control(probes, inputs, "sincos")
    rec, cam, extra = R.shade_inputs(what, np.random.default_rng(40 + what))
    got = probes["fast"].shade(what, rec, cam)
    R.check_shade(what, got, rec, extra, measured)
    unit_bound = (2.5 + 2 * measured.rsq) * R.U * 1.01
    if what == 0:
        assert (np.abs(np.linalg.norm(got[:, 6:9].astype(D), axis=1) - 1.0) <= unit_bound).all()
    if what == 1:
        assert (np.abs(np.linalg.norm(got[:, 0:3].astype(D), axis=1) - 1.0) <= unit_bound).all()
        assert ((got[:, 6:9].astype(D) * rec[:, 0:3].astype(D)).sum(1) >= 0).all()          # cosine_direction . normal >= 0
    if what == 4:
        lit = got[:, 0] != 0
        assert (np.abs(np.linalg.norm(got[lit, 1:4].astype(D), axis=1) - 1.0) <= unit_bound).all()
