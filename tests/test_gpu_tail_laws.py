"""The group laws of the MSM tail (ec_law.hip.hpp: lane, quad and row, every field's own) element by element against the oracle,
on raw point images built on the host (tests/tail_law_util.py): operands at the top of the range their type admits, weakly
normalised limbs, equal and opposite operands in computed lazy forms, the point of order two on BLS12-377, and sums handed from
one law to another.  Integer arithmetic: every comparison is exact."""
from functools import lru_cache

import pytest

import tail_law_util as U
from msm_tail_ref import LAWS

pytestmark = pytest.mark.gpu

KEYS = sorted(LAWS)
POINT_PROGRAMS = ("IDENT", "ADD", "DBL", "RUNSUM", "HORNER", "REUSE")
PARAMS = [(k, law, prog, ex) for k in KEYS for law in U.laws_of(k) for prog in POINT_PROGRAMS for ex in U.EXITS[law]]


@lru_cache(maxsize=None)
def _inputs(key, law, program, arg):
    L = U.layout(key[0], key[1], law)
    return U.images(L, U.table(key[0], program, arg), 4)


def _check(L, program, exit, arg, flat, expect, labels, k=4):
    outs = U.run(L, program, exit, k, arg, flat)
    assert len(outs) == len(expect)
    bad = U.failures(L, exit, outs, expect, ["%s arg=%d %s" % (program, arg, s) for s in labels])
    print("%s/%d %s %s exit %d arg %d: %d cases, %d wrong" % (L.curve, L.rep, L.law, program, exit, arg, len(outs), len(bad)))
    return outs, bad


@pytest.mark.parametrize("key,law,program,exit", PARAMS, ids=lambda v: "%s_%d" % v if isinstance(v, tuple) else str(v))
def test_law_program(gpu, key, law, program, exit):
    """(a) the decoded result is the oracle's point, a result at infinity has literally zero zz; (b) the image keeps the bounds the
    layout promises for the exit."""
    L = U.layout(key[0], key[1], law)
    bad = []
    for arg in (U.HORNER_ARGS if program == "HORNER" else (0,)):
        flat, expect, labels = _inputs(key, law, program, arg)
        bad += _check(L, program, exit, arg, flat, expect, labels)[1]
    assert not bad, "%d wrong, first: %s" % (len(bad), bad[:8])


@pytest.mark.parametrize("key", [k for k in KEYS if LAWS[k][0]], ids=lambda k: "%s_%d" % k)
def test_shuffle_tree(gpu, key):
    """ptrr_shuffle_round as k_combine_buckets_wave runs it, over 1 .. 64 lanes"""
    L = U.layout(key[0], key[1], "lane")
    bad = []
    for arg in U.TREE_ARGS:
        flat, expect, labels = U.images(L, U.table(key[0], "TREE", arg), arg)
        bad += _check(L, "TREE", 0, arg, flat, expect, labels, k=arg)[1]
    assert not bad, "%d wrong, first: %s" % (len(bad), bad[:8])


def _pairs(L, outs, expect, curve):
    """results of one law as the operands of another: case i is (out_i, out_i+1, inf, inf); every fourth takes out_i twice"""
    from oracle import pyref

    inf = [0] * L.dwords
    flat, ident, summed = [], [], []
    n = len(outs)
    for i in range(n):
        j = i if i % 4 == 3 else (i + 1) % n
        flat += outs[i] + outs[j] + inf + inf
        ident.append(expect[i])
        summed.append(pyref.add(curve, expect[i], expect[j]))
    return flat, ident, summed, ["operands %d, %d" % (i, i if i % 4 == 3 else (i + 1) % n) for i in range(n)]


@pytest.mark.parametrize("key", [k for k in KEYS if LAWS[k][1]], ids=lambda k: "%s_%d" % k)
def test_row_sums_are_read_by_the_other_laws(gpu, key):
    """(c) store_strict leaves the accumulator form the quad and lane laws read; store leaves the weak form the row law reads"""
    curve = key[0]
    row = U.layout(curve, key[1], "row")
    flat, expect, labels = _inputs(key, "row", "REUSE", 0)
    strict, bad = _check(row, "REUSE", 2, 0, flat, expect, labels)
    weak, bad2 = _check(row, "REUSE", 0, 0, flat, expect, labels)
    assert not bad + bad2, (bad + bad2)[:8]
    for law in ("quad", "lane"):
        L = U.layout(curve, key[1], law)
        assert L.dwords == row.dwords and L.bounds["in"][4] >= row.bounds["strict"][4]
        f2, ident, summed, lab = _pairs(L, strict, expect, curve)
        for program, want in (("IDENT", ident), ("ADD", summed)):
            bad = _check(L, program, 0, 0, f2, want, lab)[1]
            assert not bad, "%s reading store_strict: %s" % (law, bad[:8])
    f2, ident, summed, lab = _pairs(row, weak, expect, curve)
    for program, want, exit in (("IDENT", ident, 0), ("ADD", summed, 0), ("ADD", summed, 2), ("ADD", summed, 1)):
        bad = _check(row, program, exit, 0, f2, want, lab)[1]
        assert not bad, "row reading its own store: %s" % bad[:8]


def test_hook_refuses_what_it_cannot_index(gpu):
    import ctypes as C

    import blaze_amd

    L = U.layout("BLS381", 0, "lane")
    buf = (C.c_uint32 * (64 * L.dwords))()
    p = C.cast(buf, C.c_void_p)
    f = blaze_amd.aux().blz_test_law_op
    # (device, curve, repr, law, program, exit, k, arg, in, out, n)
    for args in [(0, 1, 0, 0, 1, 0, 3, 0), (0, 1, 0, 0, 4, 0, 4, 65), (0, 1, 0, 0, 6, 0, 65, 2), (0, 1, 0, 0, 6, 0, 4, 5), (0, 1, 0, 0, 6, 0, 4, 0),
                 (0, 1, 0, 1, 6, 0, 4, 2), (0, 1, 0, 0, 1, 1, 4, 0), (0, 1, 0, 1, 1, 2, 4, 0), (0, 1, 0, 0, 7, 0, 4, 0), (0, 2, 0, 2, 1, 0, 4, 0),
                 (0, 0, 1, 0, 1, 0, 4, 0)]:
        assert f(*args, p, p, 1) != 0, args
