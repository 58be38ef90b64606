"""What the tests of blz_ntt_zerocheck_gate share beyond tests/ntt_gate_util.py and tests/ntt_mle_util.py: the Python-integer
reference of a gate's round polynomial under a weight table, the weight's own step, the linear factor the caller multiplies back
in, and the C entry point itself."""
import ctypes as C

import blaze_amd
from blaze_amd._lib import BlzVecArg
from ntt_gate_util import PLONK_TERMS, gate_value

# the PLONK gate without its eq table: [qL, qR, qM, qO, qC, a, b, c], every index of PLONK_TERMS one lower, no common factor
PLONK8_TERMS = [(sign, [f - 1 for f in factors]) for sign, factors in PLONK_TERMS]
R1CS3_TERMS = [(1, [0, 1]), (-1, [2])]   # Az Bz - Cz over [Az, Bz, Cz]


def weighted_sum_gate_ref(tables, weight, terms, common, r, length, points):
    """sum_gate_ref with a weight: out[t] = sum over the pairs (T[p], T[p + length / 2]) of weight[p] x G at lo + t (hi - lo);
    tables and weight are read periodically"""
    half = length // 2
    out = []
    for t in range(points):
        s = 0
        for p in range(half):
            s += weight[p % len(weight)] * gate_value([a[p % len(a)] + t * (a[(p + half) % len(a)] - a[p % len(a)]) for a in tables], terms, common, r)
        out.append(s % r)
    return out


def weight_step_ref(weight, r, length):
    """The weight words a step with r at live length `length` writes: W[q] + W[q + length / 4], q < length / 4, canonical"""
    quarter = length // 4
    return [(weight[q] + weight[q + quarter]) % r for q in range(quarter)]


def eq1(a, x, r):
    """eq(a, x) = a x + (1 - a)(1 - x)"""
    return (a * x + (1 - a) * (1 - x)) % r


def raw_zerocheck(cl, gate, tables, weight, r, points, length, d_out):
    """The C entry point itself: gate a BlzSumGate (or None), tables ints (buffers) / DeviceBuffers / BlzVecArgs (or None),
    weight and r a DeviceBuffer / BlzVecArg / None, d_out an address"""
    if tables is None:
        arr = None
    else:
        arr = (BlzVecArg * max(len(tables), 1))(*[x if isinstance(x, BlzVecArg) else cl._vec_arg(x) for x in tables])
    vw = weight if isinstance(weight, BlzVecArg) or weight is None else cl._vec_arg(weight)
    vr = r if isinstance(r, BlzVecArg) or r is None else cl._vec_arg(r)
    return blaze_amd.lib().blz_ntt_zerocheck_gate(cl._h, None if gate is None else C.byref(gate), arr, None if vw is None else C.byref(vw),
                                                  None if vr is None else C.byref(vr), points, length, d_out)
