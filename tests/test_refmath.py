"""tests/refmath.py -- the expected side of tests/test_device_arith.py -- pinned to what the suite
already trusts: the host hooks over the ABI-form code (tests/hooks.py ed_add, sw_add,
ristretto_encode; themselves checked limb for limb against the reference oracle in
tests/test_host_arith.py), and the oracle itself where it is built.  The points are the adversarial
set the GPU tests use: identity, torsion, inverses, doublings, multiples of the base points.  The
case tables of the GPU tests are built and cross-checked here too (model against big integers), so
every expectation the GPU run compares with has been validated without a GPU."""
import numpy as np
import pytest

from tests import device_cases as dc
from tests import hooks
from tests import refmath as rm


def ed_set():
    pts = [rm.ED_IDENTITY] + rm.ed_torsion()[1:] + rm.ed_multiples(6) + rm.ed_multiples(3, 2**200 + 7, 5)
    pts += [rm.ed_neg(p) for p in pts[8:11]]
    return pts


def test_edwards_constants_and_torsion():
    assert rm.ed_on_curve(rm.ED_BASE) and rm.ED_BASE[0] == \
        15112221349535400772501151409588531511454012693041857206046113283949847762202
    assert rm.ed_mul(rm.ED_L, rm.ED_BASE) == rm.ED_IDENTITY
    t = rm.ed_torsion()
    assert len(set(t)) == 8 and all(rm.ed_on_curve(q) for q in t)
    assert t[4] == (0, rm.P - 1) and t[2][1] == 0 and t[6][1] == 0   # order 2: (0, -1); order 4: (+-i, 0)
    assert rm.ed_mul(8, t[1]) == rm.ED_IDENTITY and rm.ed_mul(4, t[1]) != rm.ED_IDENTITY


def test_edwards_addition_matches_host_hooks():
    pts = ed_set()
    for i, a in enumerate(pts):
        for j, b in enumerate(pts):
            za, zb = 1 + 3 * i, 2**254 + j
            got = hooks.ed_add(np.array(rm.ed_point51(rm.ed_extended(a, za)), np.uint64),
                               np.array(rm.ed_point51(rm.ed_extended(b, zb)), np.uint64))
            assert rm.ed_same(rm.ed_from51(got), rm.ed_add(a, b)), (i, j)


def test_ristretto_encoding_matches_host_hooks(request):
    pts = ed_set()
    tors = rm.ed_torsion()
    for i, a in enumerate(pts):
        ext = rm.ed_extended(a, 5 + i)
        want = bytes(hooks.ristretto_encode(np.array(rm.ed_point51(ext), np.uint64)))
        assert rm.ristretto_encode(ext) == want, i
        # the four representatives of a ristretto point (shifts by the 4-torsion) encode equal
        for k in (2, 4, 6):
            assert rm.ristretto_encode(rm.ed_extended(rm.ed_add(a, tors[k]), 9)) == want
    assert rm.ristretto_encode(rm.ed_extended(rm.ED_IDENTITY)) == bytes(32)
    assert rm.ristretto_encode(rm.ed_extended(rm.ED_BASE)).hex() == \
        "e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"   # RFC 9496 A.1, B


def test_ristretto_encoding_matches_oracle(oracle):
    for i, a in enumerate(ed_set()):
        ext = rm.ed_extended(a, 11 + i)
        assert rm.ristretto_encode(ext) == bytes(
            oracle.ristretto_compress(np.array(rm.ed_point51(ext), np.uint64)))


@pytest.mark.parametrize("name", ["bn254", "grumpkin", "bls12_381"])
def test_weierstrass_addition_matches_host_hooks(name):
    c = rm.CURVES[name]
    assert c.on_curve(c.base)
    pts = [None] + c.multiples(6) + c.multiples(2, 2**100 + 1, 3)
    pts += [c.neg(p) for p in pts[1:4]]
    assert all(c.on_curve(q) for q in pts)
    for i, a in enumerate(pts):
        for j, b in enumerate(pts):
            pa, pb = c.projective(a, 1 + i), c.projective(b, 2**200 + j)
            got = hooks.sw_add(c.cid, np.array(rm.sw_point64(c, pa), np.uint64),
                               np.array(rm.sw_point64(c, pb), np.uint64))
            assert c.same(rm.sw_from64(c, got), c.add(a, b)), (i, j)
            got29 = hooks.sw29_add(c.cid, np.array(rm.sw_point64(c, pa), np.uint64),
                                   np.array(rm.sw_point64(c, pb), np.uint64))
            assert c.same(rm.sw_from64(c, got29), c.add(a, b)), (i, j)


def test_weierstrass_addition_matches_oracle(oracle):
    for name, c in rm.CURVES.items():
        pts = c.multiples(4)
        for a in pts:
            for b in pts:
                got = oracle.add_projective(c.cid, np.array(rm.sw_point64(c, c.projective(a, 3)), np.uint64),
                                            np.array(rm.sw_point64(c, c.projective(b, 5)), np.uint64))
                assert c.same(rm.sw_from64(c, got), c.add(a, b))


def test_limb_layouts_roundtrip():
    x = 2**255 - 20
    assert rm.value(rm.fe51(x), 51) == x and rm.value(rm.fe29(x), 29) == x
    assert rm.rows16_values(rm.rows16([x, 1, 0, 2**256 - 1])) == [x, 1, 0, 2**256 - 1]
    for c in rm.CURVES.values():
        v = [c.p - 1, 0, 5 * c.p + 3, c.Rw - 1]
        assert rm.wave_values(c, rm.wave_rows(c, v)) == v
        pr = (3, c.p - 2, 7)
        assert rm.sw_from29(c, rm.sw_point29(c, pr, (0, 2, 5))) == pr
        assert rm.sw_from64(c, rm.sw_point64(c, pr)) == pr


#--------------------------------------------------------------------------------------------------
# the case tables of tests/test_device_arith.py: built here, inside every contract the models
# check, and the models' lane words agree with big integers on them
#--------------------------------------------------------------------------------------------------
def test_ed16w_case_tables_are_inside_the_contract_and_the_model_is_right_on_them():
    t = dc.ed16w_tables()
    for name, (u, v) in t["fmul"].items():
        got = rm.rows16_values(t["fmul_model"][name])
        for r in range(4):
            assert got[r] % rm.P == rm.rows16_values(u)[r] * rm.rows16_values(v)[r] % rm.P, (name, r)
        assert max(t["fmul_model"][name]) < 2**16 + 64, name
    for name, (kind, st, q, want) in t["point"].items():
        got = rm.rows16_values(t["point_model"][name])
        assert dc.ed_point_matches(got, want), name


@pytest.mark.parametrize("name", ["bn254", "grumpkin", "bls12_381"])
def test_sww_case_tables_are_inside_the_contract_and_the_model_is_right_on_them(name):
    c = rm.CURVES[name]
    t = dc.sww_tables(name)
    rwi = rm.inv(c.Rw, c.p)
    for case, (u, v) in t["fmul"].items():
        got = rm.wave_values(c, t["fmul_model"][case])
        for r in range(4):
            assert got[r] % c.p == rm.wave_values(c, u)[r] * rm.wave_values(c, v)[r] * rwi % c.p, (case, r)
        assert max(t["fmul_model"][case]) < (1 << c.LB) + 2
    for case, (kind, st, q, want) in t["point"].items():
        got = rm.wave_values(c, t["point_model"][case])[:3]
        assert c.same(got, want), case
