"""The host side of the reduced-radix primitive tests, without a device (tests/rr_image_util.py): the layouts say what the device
types say, every operand image sits inside its declared bound and the extremes are extreme, the Shoup model meets the truncation
it was written for, and the judge accepts the exact models' own results."""
import ctypes as C
import random

import pytest

import blaze_amd
import rr_image_util as U
from oracle import pyref

FIELD_IDS = ["%s_%s" % (c, "Fr" if f else "Fq") for c, f in U.FIELDS]
NINE = [(c, f) for c, f in U.FIELDS if U.layout(c, f).NL == 9]
PRODUCTS = ("MUL", "SQR", "MUL2", "PAIR", "DOT")
# the ops every field has, and what the 9-limb fields (the constant-operand columns) and the scalar fields (a w8) add
COMMON = {"MUL", "SQR", "MUL2", "PAIR", "DOT", "NORM", "REDUCE2M", "SUB", "SUB_TWICE", "NEG", "CNEG", "BFLY", "CANON", "ZERO", "WORDS"}
SHOUP = {"SHOUP", "SHOUP_U", "SHOUP_QUOT"}


def test_layouts_exist_for_the_six_fields_only():
    w = (C.c_uint32 * U.LAYOUT_WORDS)()
    for curve in pyref.CURVES:
        for field in (0, 1):
            assert blaze_amd.aux().blz_test_rr_layout(pyref.CURVES[curve]["id"], field, w) == 0
    for curve, field in ((3, 0), (0, 2), (-1, 0), (0, -1)):
        assert blaze_amd.aux().blz_test_rr_layout(curve, field, w) != 0


@pytest.mark.parametrize("curve,field", U.FIELDS, ids=FIELD_IDS)
def test_layout_is_what_the_device_types_say(curve, field):
    L = U.layout(curve, field)
    assert (L.B, L.NL) == ((28, 14) if L.m.bit_length() > 256 else (29, 9)) and L.E == L.B * L.NL
    assert L.H == L.E - L.m.bit_length() and (1 << L.H) * L.m < L.R
    # rr_cols_ok: (fsum + 1) NL + 1 <= 2^(64 - 2B), and FS is the last fsum it admits
    assert (L.FS + 1) * L.NL + 1 <= 1 << (64 - 2 * L.B) < (L.FS + 2) * L.NL + 1
    assert 32 * L.N32 >= L.m.bit_length() + 1 and L.T2M == (2 * L.m) >> (L.B * (L.NL - 1))
    assert len(L.by) == len(L.variants), "an (op, variant) listed twice"
    names = {v.name for v in L.variants}
    want = COMMON | (SHOUP if L.NL == 9 else set()) | ({"DFT8"} if L.NL == 9 and field == 1 else set())
    assert names == want
    for v in L.variants:
        for F, V in v.ins + v.outs:
            assert F < 1 << (32 - L.B) and V <= 1 << L.H, v.id
    # the widest variants stand on the limits themselves
    fmax = (1 << (32 - L.B)) - 1
    assert L.by[(U.OP["MUL"], 0)].ins == ((min(L.FS, fmax), 1 << L.H), (1, 1))
    assert L.by[(U.OP["MUL"], 1)].ins == ((1, 1), (min(L.FS, fmax), 1 << L.H))
    fa, fb = (f for f, _ in L.by[(U.OP["MUL"], 2)].ins)
    assert fa * fb <= L.FS < (fa + 1) * fb and abs(fa - fb) <= 1
    assert all(va * vb == 1 << L.H for (_, va), (_, vb) in [L.by[(U.OP["MUL"], k)].ins for k in (0, 1, 2)])
    (fs, vs), = L.by[(U.OP["SQR"], 0)].ins
    assert fs * fs <= L.FS and 2 * fs <= fmax and ((fs + 1) ** 2 > L.FS or 2 * (fs + 1) > fmax) and vs * vs <= 1 << L.H < 4 * vs * vs
    for k in (0, 1):
        (fa, va), (fb, vb), (fc, vc), (fd, vd) = L.by[(U.OP["MUL2"], k)].ins
        assert fa * fb + fc * fd == L.FS and va * vb + vc * vd == 1 << L.H
    assert L.by[(U.OP["NORM"], 0)].ins == ((fmax, 1 << L.H),) and L.by[(U.OP["NORM"], 0)].outs == ((1, 1 << L.H),)
    (fr, vr), = L.by[(U.OP["REDUCE2M"], 0)].ins
    mtop = L.m >> (L.B * (L.NL - 1))
    ok = lambda v: 4 * (v + 1) <= mtop and (v + 1) * (mtop + 1) <= 1 << 30
    assert fr == fmax and ok(vr) and (vr == 1 << L.H or not ok(vr + 1))
    dots = sorted(v.param for v in L.variants if v.name == "DOT" and v.var < 100)
    assert dots == list(range(1, L.FS + 1))
    for v in L.variants:
        if v.name == "DOT" and v.var < 100:   # N normalised pairs fill the column bound at N = FS, the values 2^HEAD as far as N divides it
            assert v.ins == ((1, (1 << L.H) // v.param),) * v.param + ((1, 1),) * v.param
    if L.NL == 9:
        pos = L.by[(U.OP["DOT"], 100)]
        assert pos.param == L.POS_DOT and len(pos.ins) == 2 * L.POS_DOT
        for name in ("SHOUP", "SHOUP_U"):   # both table forms at the same operand types
            assert {v.ins[0] for v in L.variants if v.name == name and v.var < 100} == {(1, 1 << L.H), (L.FS, 1 << L.H)}
            assert {v.var for v in L.variants if v.name == name} == {0, 1, 100, 101}
    for name in ("SUB", "SUB_TWICE", "NEG", "CNEG"):
        js = sorted(v.param for v in L.variants if v.name == name)
        grow = {"SUB": 1, "SUB_TWICE": 2}.get(name)
        more = 1 if name == "NEG" else 0   # 2^J m - 0 is 2^J m: rr_neg declares 2^J + 1; rr_cneg leaves a zero alone and declares 2^J
        legal = [j for j in range(1, L.NKM + 1) if ((1 << L.H) - grow * (1 << j) >= 1 if grow else (1 << j) + more <= 1 << L.H)]
        assert js == legal and js, name
        for v in L.variants:
            if v.name == name:
                assert grow or v.outs[0] == (2, (1 << v.param) + more)
                assert v.ins[-1 if name in ("SUB", "SUB_TWICE", "NEG") else 0] == (1, 1 << (v.param - 1))
                assert v.outs[0][1] <= 1 << L.H and (not grow or v.outs[0] == (fmax, 1 << L.H))
    assert {v.param for v in L.variants if v.name == "BFLY"} >= ({0, 1, 2} if L.NL == 9 else {0, 2})


@pytest.mark.parametrize("curve,field", U.FIELDS, ids=FIELD_IDS)
def test_every_image_is_inside_its_bound_and_the_extremes_are_extreme(curve, field):
    L = U.layout(curve, field)
    for v in L.variants:
        c = U.cases(curve, field, v.op, v.var)
        assert 32 <= len(c.ins) <= 4096 and len(c.labels) == len(c.ins), v.id
        for j, (F, V) in enumerate(v.ins):
            imgs = [case[j] for case in c.ins]
            assert all(len(x) == L.NL and L.within(x, (F, V)) for x in imgs), (v.id, j)
            if F == 0:
                if v.name == "WORDS":   # raw words: the upper edge is 2^(32 N32) - 1, or the last integer below param m that fits
                    top = min(v.param * L.m, 1 << (32 * L.N32)) if v.param else 1 << (32 * L.N32)
                    vals = [U.words_value(x) for x in imgs]
                    assert max(vals) == top - 1 and 0 in vals and all(not any(x[L.N32:]) for x in imgs), v.id
                    assert v.var != 0 or [0xffffffff] * L.N32 + [0] * (L.NL - L.N32) in imgs
                continue
            if v.name == "DFT8" and j >= 8:
                continue   # the three twiddles: fixed canonical values
            assert any(max(x) == (F << L.B) - 1 for x in imgs), "%s operand %d: no limb reaches F 2^B - 1" % (v.id, j)
            assert any(L.value(x) == V * L.m - 1 for x in imgs), "%s operand %d: no value reaches V m - 1" % (v.id, j)
            assert any(L.value(x) == 0 for x in imgs) or v.name == "DFT8"
    # a shifted extreme is no extreme: the check above does fail on a table that stops short
    v = L.by[(U.OP["NORM"], 0)]
    F, V = v.ins[0]
    short = [U.split(L, V * L.m - 2)]
    assert not any(L.value(x) == V * L.m - 1 for x in short) and not any(max(x) == (F << L.B) - 1 for x in short)


@pytest.mark.parametrize("curve,field", U.FIELDS, ids=FIELD_IDS)
def test_all_peaks_meet_in_one_case(curve, field):
    """a column with all its products at their maximum: some case of every product has EVERY operand at its all-ones value"""
    L = U.layout(curve, field)
    for v in L.variants:
        if v.name in PRODUCTS:
            c = U.cases(curve, field, v.op, v.var)
            ones = [U.all_ones_below(L, V * L.m) for _, V in v.ins]
            assert any(all(L.value(x) == o for x, o in zip(case, ones)) for case in c.ins), v.id


def test_resplit_keeps_the_integer_and_reaches_the_cap():
    L = U.layout("BLS381", 1)
    rng = random.Random(3)
    for F in (2, 3, 6, 7):
        v = U.all_ones_below(L, 8 * L.m)
        for mode in U.MODES:
            x = U.resplit(L, U.split(L, v), F, mode, rng)
            assert L.value(x) == v and max(x) < F << L.B and min(x) >= 0
        assert max(U.resplit(L, U.split(L, v), F, "even")) == (F << L.B) - 1
        assert U.resplit(L, U.split(L, v), F, "bottom")[0] == (F << L.B) - 1
    assert U.resplit(L, U.split(L, 5), 7, "max") == U.split(L, 5)


@pytest.mark.parametrize("curve,field", U.FIELDS, ids=FIELD_IDS)
def test_the_judge_accepts_the_exact_models(curve, field):
    """Every product table through the Montgomery model and every linear table through plain integers: no column sum leaves 64
    bits (mont_model asserts it), every result keeps the bound its type declares, and the judge finds nothing wrong - then a
    result one off in one limb, or one m too large, is refused."""
    L = U.layout(curve, field)
    for v in L.variants:
        if v.name not in PRODUCTS + ("SUB", "SUB_TWICE", "NEG", "CNEG", "NORM", "CANON"):
            continue
        if v.name == "DOT" and v.param not in (1, L.POS_DOT, L.FS):
            continue
        c = U.cases(curve, field, v.op, v.var)
        step = 1 if v.name not in PRODUCTS else max(1, len(c.ins) // 150)
        for i in list(range(0, len(c.ins), step))[:400] + list(range(min(40, len(c.ins)))):
            want = U.expect(L, v, c.ins[i], c.extra[i])
            outs = [w[1] if w[0] == "limbs" else U.split(L, w[1]) for w in want]
            if v.name not in PRODUCTS and v.name not in ("NORM", "CANON"):
                outs = [U.resplit(L, o, v.outs[0][0], "rand", random.Random(i)) for o in outs]
            why = U.judge(L, v, c.ins[i], outs, c.extra[i])
            assert why is None, (v.id, c.labels[i], why)
            if i < 3:
                bad = [list(o) for o in outs]
                bad[0][1] ^= 1
                assert U.judge(L, v, c.ins[i], bad, c.extra[i]) is not None
                if v.name in PRODUCTS:
                    bad = [U.split(L, L.value(outs[0]) + 2 * L.m)] + outs[1:]
                    assert "declared bound" in U.judge(L, v, c.ins[i], bad, c.extra[i])


@pytest.mark.parametrize("curve,field", NINE, ids=["%s_%d" % k for k in NINE])
def test_the_shoup_model_meets_the_truncation(curve, field):
    """At least 32 crafted (x, w) per 9-limb field on which the truncated quotient is one below floor(x wq / Rrr) by the model;
    random pairs practically never are.  The result stays the product and below 2m, and - recorded here - the model never takes the
    T2M correction on operands the type admits: r / m stays below 1 + V m / Rrr + 2^-22."""
    L = U.layout(curve, field)
    found, tries = U.truncation_cases(curve, field)
    assert len(found) >= 32, "%d truncation cases in %d tries" % (len(found), tries)
    rng = random.Random(11)
    near = 0
    for _ in range(2000):
        x, w = rng.randrange((1 << L.H) * L.m), rng.randrange(L.m)
        _, qt, qf, _ = U.shoup_model(L, U.split(L, x), w)
        assert qt in (qf, qf - 1)
        near += qt != qf
    assert near <= 2, "random pairs were not expected on the correction path: %d of 2000" % near
    worst, corrected = 0.0, 0
    for op in ("SHOUP", "SHOUP_U"):
        for v in L.variants:
            if v.name != op:
                continue
            c = U.cases(curve, field, v.op, v.var)
            assert sum(1 for lab in c.labels if lab.startswith("trunc")) >= (32 if v.ins[0][1] == 1 << L.H else 0)
            for ins, w in zip(c.ins, c.extra):
                r, qt, qf, raw = U.shoup_model(L, ins[0], w)
                x = L.value(ins[0])
                assert qt in (qf, qf - 1) and qf in ((x * w) // L.m, (x * w) // L.m - 1)
                assert L.value(r) % L.m == x * w % L.m and L.value(r) < 2 * L.m and max(r) <= L.mask
                worst = max(worst, raw / L.m)
                corrected += raw != L.value(r)
                assert raw / L.m < 1 + x / L.R + 2.0 ** -22
    print("%s: largest r / m of the model before the correction %.4f, corrections taken %d" % (L.name, worst, corrected))
    assert corrected == 0 and worst < 1 + (1 << L.H) * L.m / L.R + 2.0 ** -22 < 2


def test_quot_ws_hold_the_edges():
    L = U.layout("BN254", 1)
    ws = U.quot_ws(L, random.Random(1))
    assert {0, 1, 2, L.m - 1, L.m - 2, (L.m + 1) // 2, (L.m - 1) // 2, 1 << 100, (1 << 100) - 1, (1 << 100) + 1} <= set(ws) and max(ws) < L.m
