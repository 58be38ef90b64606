"""The reduced-radix primitives (field_rr.hip.hpp, rr_bfly / rr_canon / dft8_rr, rr_dot) one by one on raw limb images at the top of
what their types admit, against Python integers (tests/rr_image_util.py): residues, the declared bound of every result, exact
integers for the linear ops, and limb-for-limb agreement with the exact models of the Montgomery and Shoup columns.  One launch per
(field, op, variant) the hook's layout lists."""
import ctypes as C

import pytest

import blaze_amd
import rr_image_util as U
from oracle import pyref

pytestmark = pytest.mark.gpu

PARAMS = [(c, f, v.id) for c, f in U.FIELDS for v in U.layout(c, f).variants]
RAN = set()
WORST = {}   # field -> the largest r / m a Shoup product left on the device


def _variant(curve, field, vid):
    L = U.layout(curve, field)
    return L, next(v for v in L.variants if v.id == vid)


@pytest.mark.parametrize("curve,field,vid", PARAMS, ids=["%s_%s_%s" % (c, "Fr" if f else "Fq", v) for c, f, v in PARAMS])
def test_rr_primitive(gpu, curve, field, vid):
    L, v = _variant(curve, field, vid)
    c = U.cases(curve, field, v.op, v.var)
    outs = U.run(L, v, c)
    RAN.add((curve, field, v.op, v.var))
    assert len(outs) == len(c.ins)
    bad = U.failures(L, v, c, outs)
    if v.name in ("SHOUP", "SHOUP_U"):
        WORST[L.name] = max([WORST.get(L.name, 0.0)] + [L.value(o[0]) / L.m for o in outs])
    print("%s %s: %d cases, %d wrong" % (L.name, v.id, len(outs), len(bad)))
    assert not bad, "%d of %d wrong, first: %s" % (len(bad), len(outs), bad[:4])


def test_every_listed_variant_ran_and_nothing_else(gpu):
    """What ran is what the layouts list, every op of the table among it.  Meaningful only when the whole module runs, in file
    order, in one process: the set is filled by test_rr_primitive above, so a selection (-k, --lf), a reordering or a split over
    workers fails here although nothing is wrong."""
    listed = {(c, f, v.op, v.var) for c, f in U.FIELDS for v in U.layout(c, f).variants}
    assert RAN == listed, "not run: %s; not listed: %s" % (sorted(listed - RAN)[:8], sorted(RAN - listed)[:8])
    assert {U.OP_NAME[op] for _, _, op, _ in RAN} == set(U.OP)
    for name, worst in sorted(WORST.items()):
        print("%s: the largest Shoup result on the device is %.4f m" % (name, worst))
        assert worst < 2


@pytest.mark.parametrize("curve,field", U.FIELDS, ids=["%s_%s" % (c, "Fr" if f else "Fq") for c, f in U.FIELDS])
def test_neg_of_zero_keeps_the_declared_bound(gpu, curve, field):
    """2^J m - 0 IS 2^J m: rr_neg<J> declares a value below (2^J + 1) m and returns exactly 2^J m, rr_cneg<J> - whose result is
    stored and subtracted under the bound 2^J m - leaves a literal zero alone, whatever the sign."""
    L = U.layout(curve, field)
    seen = 0
    for v in L.variants:
        if v.name not in ("NEG", "CNEG"):
            continue
        c = U.cases(curve, field, v.op, v.var)
        sub = U.Cases(L, v)
        for i, ins in enumerate(c.ins):
            if not any(ins[0]):
                sub.add(c.labels[i], ins, c.extra[i])
        assert len(sub.ins) >= (1 if v.name == "NEG" else 3), v.id
        outs = U.run(L, v, sub)
        assert not U.failures(L, v, sub, outs), U.failures(L, v, sub, outs)[:2]
        for out in outs:
            assert L.value(out[0]) == ((L.m << v.param) if v.name == "NEG" else 0), v.id
        seen += len(outs)
    assert seen >= 8


def test_mul_and_mul_ref_agree_limb_for_limb(gpu):
    """the asm columns against the compiler's own schedule of the same product, on the widest operands of the largest field"""
    L, v = _variant("BLS377", 0, "MUL_2")
    c = U.cases("BLS377", 0, v.op, v.var)
    outs = U.run(L, v, c)
    assert all(o[0] == o[1] for o in outs)


def test_hook_refuses_what_the_code_cannot_instantiate(gpu):
    buf = (C.c_uint32 * (64 * 16 * 14))()
    p = C.cast(buf, C.c_void_p)
    f = blaze_amd.aux().blz_test_rr_op
    ids = {c: pyref.CURVES[c]["id"] for c in pyref.CURVES}
    # (device, curve, field, op, variant): the Shoup ops on 14 limbs, a DFT without a w8, J beyond the value range, unknown ops
    refused = [(0, ids["BLS381"], 0, U.OP["SHOUP"], 0), (0, ids["BLS377"], 0, U.OP["SHOUP_U"], 1), (0, ids["BLS377"], 0, U.OP["SHOUP_QUOT"], 0),
               (0, ids["BLS381"], 0, U.OP["DFT8"], 0), (0, ids["BN254"], 0, U.OP["DFT8"], 0), (0, ids["BLS381"], 1, U.OP["SUB"], 6),
               (0, ids["BLS381"], 1, U.OP["SUB_TWICE"], 5), (0, ids["BLS381"], 1, U.OP["NEG"], 0), (0, ids["BLS381"], 1, U.OP["DOT"], 7),
               (0, ids["BLS381"], 1, 19, 0), (0, ids["BLS381"], 1, -1, 0), (0, ids["BLS381"], 2, 0, 0), (0, 3, 0, 0, 0)]
    for args in refused:
        assert f(*args, p, p, 1) != 0, args
    assert f(0, ids["BLS381"], 1, 0, 0, p, p, 0) != 0 and f(0, ids["BLS381"], 1, 0, 0, None, p, 1) != 0
