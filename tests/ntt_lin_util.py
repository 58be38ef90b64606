"""What the tests of blz_ntt_gate_eval_lin share beyond tests/ntt_gate_util.py: the Python-integer reference of a gate whose
factors may be linear forms (lin_value at one position, lin_ref over a length with periodic tables and rotations), the
catalogue of form gates, and the description builder for the C entry point."""
import ctypes as C

import blaze_amd
from blaze_amd._lib import BlzLinGate, BlzVecArg

FORM = 0x80
NO_COEF = 0xFF
M64 = (1 << 64) - 1


def form_value(v, form, r):
    """sum of (+/-) [v[coef] x] v[table] over the summands (sign, coef, table); coef None is 1"""
    return sum(sign * (v[t] if c is None else v[c] * v[t]) for sign, c, t in form) % r


def lin_value(v, forms, terms, common, r):
    """The gate at one point: v[j] the value of table j; a factor (and common) is a table index or FORM + k"""
    def val(f):
        return form_value(v, forms[f - FORM], r) if f >= FORM else v[f]
    s = 0
    for sign, factors in terms:
        pr = 1
        for f in factors:
            pr = pr * val(f) % r
        s += sign * pr
    return (s if common is None else val(common) * s) % r


def lin_ref(vals, forms, terms, common, r, length, rot=None):
    """dst[p], p < length: table i read at (p + rot[i]) mod 2^64 mod its count"""
    rot = rot or [0] * len(vals)
    return [lin_value([v[((p + k) & M64) % len(v)] for v, k in zip(vals, rot)], forms, terms, common, r) for p in range(length)]


def _perm():
    """Z(wX) prod_j (w_j + beta sigma_j + gamma) - Z prod_j (w_j + beta k_j X + gamma) over
    [Z (rot 1), Z, a, b, c, sigma1, sigma2, sigma3, X, beta, beta k1, beta k2, gamma]"""
    forms = [[(1, None, 2 + j), (1, 9, 5 + j), (1, None, 12)] for j in range(3)]
    forms += [[(1, None, 2 + j), (1, (9, 10, 11)[j], 8), (1, None, 12)] for j in range(3)]
    return forms, [(1, [0, FORM, FORM + 1, FORM + 2]), (-1, [1, FORM + 3, FORM + 4, FORM + 5])]


PERM_FORMS, PERM_TERMS = _perm()
PERM_ROT = [1] + [0] * 12


def perm_counts(n):
    return [n] * 9 + [1] * 4


# name -> (ntables, forms, terms, common, counts(n), rot or None, {index: the index whose words it shares}).  Each exists for
# the failure it can expose:
#   PERM    the three-wire permutation term: 13 tables, six forms with a one-word coefficient each (LDS), two four-factor terms
#           that begin with a word and go on with forms, a negated term, Z under two indices with rotations 1 and 0
#   NUM     prod_3 (w + beta id + gamma): a term that BEGINS with a form (the constant R^3 meets a form's value)
#   LOGUP   beta + gamma f1 + gamma^2 f2 + gamma^3 f3: a lone four-summand form, the only factor of the only term (no product
#           outside the form), its first summand a one-word table without coefficient
#   ZL1     (Z - one) L1: a negated summand without coefficient
#   COMMON  a form as common whose FIRST summand is negated and whose coefficient has n words; common also a factor
#   TWICE   one form twice in a term and once more in another
#   LONG    coefficients of n and of 4 words: a slot of their own, two products
#   SQUARE  a coefficient that is the table it multiplies, n words and one word
#   T16     16 tables, four forms of four summands under a table as common, a one-factor term, and a form no term names
def _n(count_list):
    return lambda n: [n if c == "n" else min(c, n) for c in count_list]


CATALOGUE = {
    "PERM": (13, PERM_FORMS, PERM_TERMS, None, perm_counts, PERM_ROT, {1: 0}),
    "NUM": (8, [[(1, None, j), (1, 6, 3 + j), (1, None, 7)] for j in range(3)], [(1, [FORM, FORM + 1, FORM + 2])], None,
            _n(["n"] * 6 + [1, 1]), None, {}),
    "LOGUP": (7, [[(1, None, 0), (1, 1, 4), (1, 2, 5), (1, 3, 6)]], [(1, [FORM])], None, _n([1, 1, 1, 1, "n", "n", "n"]), None, {}),
    "ZL1": (3, [[(1, None, 0), (-1, None, 1)]], [(1, [FORM, 2])], None, _n(["n", 1, "n"]), None, {}),
    "COMMON": (4, [[(-1, None, 0), (1, 1, 2)]], [(1, [1, 2]), (-1, [3]), (1, [FORM])], FORM, _n(["n"] * 4), None, {}),
    "TWICE": (3, [[(1, None, 0), (1, 2, 1)]], [(1, [FORM, FORM]), (-1, [FORM, 0])], None, _n(["n", "n", 1]), None, {}),
    "LONG": (5, [[(1, 1, 0), (-1, 2, 3)], [(-1, 4, 4), (1, 4, 0)]], [(1, [FORM, 0]), (1, [FORM + 1])], None, _n(["n", "n", 4, "n", 4]), None, {}),
    "SQUARE": (2, [[(1, 0, 0), (1, None, 1)], [(1, 1, 1)]], [(1, [FORM]), (1, [FORM + 1, 0])], None, _n(["n", 1]), None, {}),
    "T16": (16, [[(1, None, 4 * k), (-1, 15 - k, 4 * k + 1), (1, k, 4 * k + 2), (-1, None, 4 * k + 3)] for k in range(4)] + [[(1, 13, 12)]],
            [(1, [FORM, FORM + 1, FORM + 2, FORM + 3]), (-1, [15])], 14, _n(["n"] * 12 + [1, 1, 4, 1]), None, {}),
}


def make_lin_gate(ntables, forms, terms, common):
    g = BlzLinGate(ntables, len(terms), -1 if common is None else common, len(forms))
    for m, (sign, factors) in enumerate(terms[:8]):
        g.term[m].nfactors, g.term[m].negate = len(factors), int(sign < 0)
        for j, f in enumerate(factors[:4]):
            g.term[m].factor[j] = f
    for k, form in enumerate(forms[:8]):
        g.form[k].nsummands = len(form)
        for s, (sign, coef, table) in enumerate(form[:4]):
            x = g.form[k].summand[s]
            x.coef, x.table, x.negate = NO_COEF if coef is None else coef, table, int(sign < 0)
    return g


def raw_lin(cl, gate, dst, tables, rot, length):
    """The C entry point itself: gate a BlzLinGate (or None), dst / tables ints (buffers) / DeviceBuffers / BlzVecArgs (or None),
    rot a list of ints or None"""
    def arg(x):
        return x if isinstance(x, BlzVecArg) else cl._vec_arg(x)
    arr = None if tables is None else (BlzVecArg * max(len(tables), 1))(*[arg(x) for x in tables])
    vd = None if dst is None else arg(dst)
    rots = None if rot is None else (C.c_uint64 * max(len(rot), 1))(*[k & M64 for k in rot])
    return blaze_amd.lib().blz_ntt_gate_eval_lin(cl._h, None if gate is None else C.byref(gate), None if vd is None else C.byref(vd), arr, rots, length)
