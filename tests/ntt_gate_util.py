"""What the tests of blz_ntt_sumcheck_gate share beyond tests/ntt_mle_util.py: the Python-integer reference of a caller-defined
gate, the gate catalogue and the house input recipe (ntt_spmv_util._inputs: the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked
random 256-bit words behind)."""
import ctypes as C

import blaze_amd
from blaze_amd._lib import BlzSumGate, BlzVecArg
from ntt_spmv_util import _inputs


def gate_value(v, terms, common, r):
    """G at one point: v[j] the value of table j"""
    s = 0
    for sign, factors in terms:
        pr = 1
        for f in factors:
            pr = pr * v[f] % r
        s += sign * pr
    return (s if common is None else v[common] * s) % r


def sum_gate_ref(tables, terms, common, r, length, points):
    """out[t] = sum over the pairs (T[p], T[p + length / 2]) of G at lo + t (hi - lo); tables are read periodically"""
    half = length // 2
    out = []
    for t in range(points):
        s = 0
        for p in range(half):
            s += gate_value([a[p % len(a)] + t * (a[(p + half) % len(a)] - a[p % len(a)]) for a in tables], terms, common, r)
        out.append(s % r)
    return out


def gate_inputs(r, ntables, length, seed):
    """`ntables` tables of `length` words, the edge words rotated so that they meet one another and not only themselves"""
    vals = [_inputs(r, length, seed + 10 * j) for j in range(ntables)]
    return [v[j % length:] + v[:j % length] for j, v in enumerate(vals)]


# name -> (ntables, terms [(sign, [table indices])], common).  Each exists for the failure it can expose:
#   G1  one term, one factor, no common: no product at all, closed with k = 1 (BLZ_GATE_PRODUCT at k = 1)
#   G2  R1CS as a sum gate: mixed term lengths (a deficit), a negated term, a common factor; equals BLZ_GATE_R1CS byte for byte
#   G3  vanilla PLONK over [eq, qL, qR, qM, qO, qC, a, b, c]: term lengths 2, 2, 3, 2, 1 under a common factor, degree 4
#   G4  full size: 12 tables, 8 terms, one of 4 factors, no common, a table repeated within a term (a a a a) and across terms,
#       tables 10 and 11 named by no term - and still folded
#   G5  common also a factor, T0 (T0 T1 - T2);  G5Z  signs that cancel: + a b - a b, every output word 0
PLONK_TERMS = [(1, [1, 6]), (1, [2, 7]), (1, [3, 6, 7]), (-1, [4, 8]), (1, [5])]
CATALOGUE = {
    "G1": (1, [(1, [0])], None),
    "G2": (4, [(1, [1, 2]), (-1, [3])], 0),
    "G3": (9, PLONK_TERMS, 0),
    "G4": (12, [(1, [0, 0, 0, 0]), (-1, [1, 2]), (1, [3]), (1, [4, 5, 6]), (-1, [7, 7, 8]), (1, [9, 0]), (-1, [2]), (1, [1, 2, 3])], None),
    "G5": (3, [(1, [0, 1]), (-1, [2])], 0),
    "G5Z": (2, [(1, [0, 1]), (-1, [0, 1])], None),
}


def make_gate(ntables, terms, common, reserved=0):
    g = BlzSumGate(ntables, len(terms), -1 if common is None else common, reserved)
    for m, (sign, factors) in enumerate(terms[:8]):
        g.term[m].nfactors, g.term[m].negate = len(factors), int(sign < 0)
        for j, f in enumerate(factors[:4]):
            g.term[m].factor[j] = f
    return g


def raw_gate(cl, gate, tables, r, points, length, d_out):
    """The C entry point itself: gate a BlzSumGate (or None), tables ints (buffers) / DeviceBuffers / BlzVecArgs (or None),
    r a DeviceBuffer / BlzVecArg / None, d_out an address"""
    if tables is None:
        arr = None
    else:
        arr = (BlzVecArg * max(len(tables), 1))(*[x if isinstance(x, BlzVecArg) else cl._vec_arg(x) for x in tables])
    vr = r if isinstance(r, BlzVecArg) or r is None else cl._vec_arg(r)
    return blaze_amd.lib().blz_ntt_sumcheck_gate(cl._h, None if gate is None else C.byref(gate), arr, None if vr is None else C.byref(vr),
                                                 points, length, d_out)
