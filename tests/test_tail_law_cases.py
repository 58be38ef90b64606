"""The host side of the group-law tests, without a device (tests/tail_law_util.py): images encode and decode as the layouts say, the
representatives sit where they claim, the case tables hold the operand classes they are there for, and the step-by-step expectations
agree with scalar multiplication."""
import ctypes as C
import random

import pytest

import blaze_amd
import tail_law_util as U
from msm_tail_ref import LAWS
from oracle import pyref

KEYS = sorted(LAWS)
KEY_LAWS = [(k, law) for k in KEYS for law in U.laws_of(k)]


def test_layouts_exist_for_the_product_laws_only():
    w = (C.c_uint32 * 32)()
    for curve in pyref.CURVES:
        for rep in (0, 1):
            for law, lid in U.LAW_ID.items():
                rc = blaze_amd.aux().blz_test_law_layout(pyref.CURVES[curve]["id"], rep, lid, w)
                want = (curve, rep) in LAWS and law in U.laws_of((curve, rep))
                assert (rc == 0) == want, (curve, rep, law)
    assert blaze_amd.aux().blz_test_law_layout(7, 0, 0, w) != 0


@pytest.mark.parametrize("key,law", KEY_LAWS)
def test_layout_is_what_the_device_types_say(key, law):
    L = U.layout(key[0], key[1], law)
    rr, row = LAWS[key]
    assert L.lanes == {"lane": 1, "quad": 4, "row": 64}[law]
    assert L.e == L.B * L.NL and L.R > 4 * L.m and L.stride >= L.NL and L.stride % 2 == 0
    assert (L.B < 32) == rr and L.closed == (not rr) and L.tree == (rr and law == "lane")
    for exit in (0, 1, 2):
        assert any(L.bounds[U.EXIT_BOUND[exit]]) == (exit in U.EXITS[law])
    for name, b in L.bounds.items():
        if any(b):
            # a limb bound never lets a coordinate of its value bound overflow the top limb's register
            assert b[4] < 1 << 32 and max(b[:4]) * L.m < L.R
    if law == "row":
        assert L.bounds["in"][4] == 1 << L.B and L.bounds["strict"][4] == (1 << L.B) - 1
        # the strict exits are what the lane and quad laws of the field read
        lane = U.layout(key[0], key[1], "lane").bounds["in"]
        assert all(s <= r for s, r in zip(L.bounds["strict"], lane)) and L.bounds["to_lane"] == L.bounds["strict"]


@pytest.mark.parametrize("key,law", KEY_LAWS)
def test_encode_then_decode_is_the_identity(key, law):
    L = U.layout(key[0], key[1], law)
    rng = random.Random(5)
    S = U.point_set(key[0])
    reps = ("low", "top") + (("weak",) if law == "row" else ())
    weak_limbs = 0
    for name, P in S.items():
        for rep in reps:
            zs = U.weak_zs(key[0], key[1]) if rep == "weak" else (1, rng.randrange(2, L.m))
            for z in zs:
                img = U.encode(L, P, z, rep)
                assert len(img) == L.dwords
                d = U.decode(L, img)
                assert d.point == P and d.consistent, (name, rep)
                assert d.literal_inf == (P is None)
                assert d.max_limb <= L.bounds["in"][4]
                if P is None:
                    continue
                for v, f in zip(d.values, L.bounds["in"][:4]):
                    assert L.within(v, f)
                    # low: below m; top: the input bound minus at most one m
                    assert U.value_factor(L, v) == (f if rep == "top" else 1), (name, rep)
                if rep == "weak":
                    assert d.values == U.decode(L, U.encode(L, P, z, "low")).values
                    weak_limbs += sum(1 for x in img if x == 1 << L.B)
    if law == "row":
        assert weak_limbs >= 2 * len(S)   # the weak images do hold limbs equal to 2^B (zz has three zero limbs under these z)


def test_a_coordinate_is_its_limb_sum_whatever_the_limbs():
    L = U.layout("BLS381", 0, "row")
    P = U.point_set("BLS381")["P0"]
    img = U.encode(L, P, 3, "low")
    v = U.decode(L, img).values
    img[0] += 1 << L.B            # a pending carry in limb 0 of x ...
    img[1] -= 1                   # ... borrowed from limb 1: the same value
    assert U.decode(L, img).values == v and U.decode(L, img).point == P
    img[2 * L.stride] += 1
    assert not U.decode(L, img).consistent


CLASSES = {
    "ADD": {"inf_left", "inf_right", "equal", "opposite", "result_inf"},
    "RUNSUM": {"inf_left", "inf_right", "equal", "opposite", "result_inf", "computed_doubled"},
    "HORNER": {"inf_left", "inf_right", "equal", "opposite", "result_inf", "computed_doubled"},
    "REUSE": {"inf_left", "inf_right", "equal", "opposite", "result_inf", "computed_doubled"},
    "TREE": {"inf_right", "equal", "opposite", "result_inf", "computed_doubled"},
}


@pytest.mark.parametrize("curve", sorted(pyref.CURVES))
@pytest.mark.parametrize("program", sorted(CLASSES))
def test_every_table_meets_its_operand_classes(curve, program):
    args = {"HORNER": [a for a in U.HORNER_ARGS if a], "TREE": [a for a in U.TREE_ARGS if a >= 33]}.get(program, [0])
    for arg in args:
        cases = U.table(curve, program, arg)
        seen = set().union(*(c.events for c in cases))
        want = set(CLASSES[program])
        if curve == "BLS377" and program != "ADD":   # (ADD's operands are fresh loads)
            want.add("computed_T_doubled")
        assert want <= seen, (arg, want - seen)
        assert program == "TREE" or any(c.expect is None for c in cases)   # (a tree meets infinity in a partial sum: result_inf)
    # equal operands with different z: the "each" z mode gives every operand its own
    assert "each" in U.Z_MODES and "one" in U.Z_MODES


def test_the_order_two_point_meets_itself_as_a_loaded_lazy_form():
    """RUNSUM's s += run doubles a bucket's sum when the buckets below it are empty: with the sum T in a representative whose
    y is a non-zero multiple of m (top), the doubling sees what a computed T looks like."""
    L = U.layout("BLS377", 0, "row")
    T = U.point_set("BLS377")["T"]
    assert any(c.pts[0] == T and c.pts[1:] == [None] * 3 and c.expect is None for c in U.table("BLS377", "RUNSUM"))
    d = U.decode(L, U.encode(L, T, 5, "top"))
    assert d.values[1] % L.m == 0 and d.values[1] != 0 and d.point == T


@pytest.mark.parametrize("curve", sorted(pyref.CURVES))
def test_stepwise_expectations_equal_scalar_multiplication(curve):
    add, mul = (lambda p, q: pyref.add(curve, p, q)), (lambda p, k: pyref.mul(curve, p, k))
    for c in U.table(curve, "RUNSUM"):
        want = None
        for w, P in zip((4, 3, 2, 1), c.pts):
            want = add(want, mul(P, w))
        assert c.expect == want
    for arg in U.HORNER_ARGS:
        for c in U.table(curve, "HORNER", arg):
            want = add(add(mul(c.pts[0], 1 << (2 * arg)), mul(c.pts[1], 1 << arg)), c.pts[2])
            assert c.expect == want
    for c in U.table(curve, "REUSE"):
        assert c.expect == add(add(mul(add(c.pts[0], c.pts[1]), 2), c.pts[2]), c.pts[3])
    for arg in U.TREE_ARGS:
        for c in U.table(curve, "TREE", arg):
            want = None
            for P in c.pts:
                want = add(want, P)
            assert len(c.pts) == arg and c.expect == want


def test_images_cross_every_case_with_z_modes_and_representatives():
    L = U.layout("BLS377", 0, "row")
    cases = U.table("BLS377", "DBL")
    flat, expect, labels = U.images(L, cases, 4)
    assert len(expect) == len(cases) * 9 == len(labels) and len(flat) == len(expect) * 4 * L.dwords
    Lq = U.layout("BN254", 1, "quad")
    assert len(U.images(Lq, U.table("BN254", "DBL"), 4)[1]) == len(U.table("BN254", "DBL")) * 6
    # what goes in decodes to the case's points
    i = labels.index("case 3 z=each rep=weak")
    img = flat[i * 4 * L.dwords:i * 4 * L.dwords + L.dwords]
    assert U.decode(L, img).point == cases[3].pts[0]
