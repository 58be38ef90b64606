"""Host side of the group-law tests (tests/test_tail_law_cases.py, tests/test_gpu_tail_laws.py): point images in a law's own memory
layout built and read back with Python integers, the case tables, and their expected points from oracle/pyref.py.

An image is x | y | zz | zzz with X = x z^2 R + kx m, Y = y z^3 R + ky m, ZZ = z^2 R + .., ZZZ = z^3 R + .. (mod m, R the law's Montgomery
radix), each split into B-bit limbs; infinity is the all-zero image.  What a law admits (how many m a coordinate may carry, how
large a limb may be) comes from blz_test_law_layout, which reads it off the device types."""
import ctypes as C
import random
from functools import lru_cache

import blaze_amd
from msm_tail_ref import LAWS
from oracle import pyref

LAW_ID = {"lane": 0, "quad": 1, "row": 2}
PROGRAM = {"IDENT": 0, "ADD": 1, "DBL": 2, "RUNSUM": 3, "HORNER": 4, "REUSE": 5, "TREE": 6}
EXITS = {"lane": (0,), "quad": (0, 1), "row": (0, 1, 2)}
EXIT_BOUND = {0: "store", 1: "to_lane", 2: "strict"}
TREE_ARGS = (1, 2, 3, 33, 63, 64)
HORNER_ARGS = (0, 1, 5)


def laws_of(key):
    return ("lane", "quad") + (("row",) if LAWS[key][1] else ())


class Layout:
    def __init__(self, curve, rep, law):
        w = (C.c_uint32 * 32)()
        blaze_amd._lib.check(blaze_amd.aux().blz_test_law_layout(pyref.CURVES[curve]["id"], rep, LAW_ID[law], w))
        self.curve, self.rep, self.law = curve, rep, law
        self.B, self.NL, self.stride, self.e, self.lanes, closed = w[0:6]
        self.closed = bool(closed)
        self.bounds = {"in": tuple(w[6:11]), "store": tuple(w[11:16]), "strict": tuple(w[16:21]), "to_lane": tuple(w[21:26])}
        self.tree = bool(w[26])
        self.m = pyref.CURVES[curve]["q"]
        self.R = 1 << self.e
        self.dwords = 4 * self.stride

    def within(self, value, v):
        """value inside the range a bound of v m promises"""
        return value <= v * self.m if self.closed else value < v * self.m


@lru_cache(maxsize=None)
def layout(curve, rep, law):
    return Layout(curve, rep, law)


# ---------------------------------------------------------------------------------------------- images
def split(L, value, weak=False):
    """value -> stride dwords: NL limbs of B bits, the top limb keeps the rest.  weak: every zero limb under a non-zero one becomes
    2^B by borrowing 1 from the limb above (from the top down, so a run of zero limbs becomes 2^B, 2^B - 1, .., 2^B - 1)."""
    mask = (1 << L.B) - 1
    limbs = [(value >> (L.B * i)) & mask for i in range(L.NL - 1)] + [value >> (L.B * (L.NL - 1))]
    if weak:
        for i in range(L.NL - 2, -1, -1):
            if limbs[i] == 0 and limbs[i + 1] > 0:
                limbs[i] = 1 << L.B
                limbs[i + 1] -= 1
    assert max(limbs) <= L.bounds["in"][4], "the value does not fit the law's limbs"
    return limbs + [0] * (L.stride - L.NL)


def encode(L, P, z=1, rep="low"):
    """The image of P (None: infinity) scaled by z.  rep: low (each coordinate below m), top (the largest multiple of m the law
    admits on input added), weak (low, weakly normalised limbs: row law only)."""
    if P is None:
        return [0] * L.dwords
    m = L.m
    zz = z * z % m
    zzz = zz * z % m
    vals = [P[0] * zz * L.R % m, P[1] * zzz * L.R % m, zz * L.R % m, zzz * L.R % m]
    out = []
    for v, f in zip(vals, L.bounds["in"][:4]):
        out += split(L, v + (f - 1) * m if rep == "top" else v, weak=rep == "weak")
    return out


class Decoded:
    pass


def decode(L, img):
    """Any image: a coordinate is sum limb 2^(B i) whatever the limbs are.  .point (None: zz = 0 mod m), .literal_inf (every limb of
    zz zero), .consistent (ZZ^3 = ZZZ^2 as field elements), .values (the four integers), .max_limb."""
    d = Decoded()
    S, m = L.stride, L.m
    d.values = [sum(img[c * S + i] << (L.B * i) for i in range(L.NL)) for c in range(4)]
    d.max_limb = max(max(img[c * S:c * S + L.NL]) for c in range(4))
    d.literal_inf = not any(img[2 * S:2 * S + L.NL])
    X, Y, ZZ, ZZZ = d.values
    if ZZ % m == 0:
        d.point, d.consistent = None, True
    else:
        d.consistent = ZZZ % m != 0 and (ZZ * ZZ * ZZ - ZZZ * ZZZ * L.R) % m == 0
        d.point = (X * pow(ZZ, -1, m) % m, Y * pow(ZZZ, -1, m) % m) if d.consistent else ("inconsistent",)
    return d


def value_factor(L, value):
    """the smallest f with value < f m"""
    return value // L.m + 1


def _sqrt(a, p):
    """Tonelli-Shanks; None when a is no square"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    mm, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (mm - i - 1), p)
        mm, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


@lru_cache(maxsize=None)
def weak_zs(curve, rep, count=4):
    """z values whose ZZ = z^2 R mod m has zero limbs (0, 5 and 6), so that the weak form of the image holds limbs equal to 2^B:
    random Montgomery forms practically never have a zero limb."""
    L = layout(curve, rep, "row")
    rng = random.Random(377)
    mask, out = (1 << L.B) - 1, []
    keep = ~(mask | (mask << 5 * L.B) | (mask << 6 * L.B))
    rinv = pow(L.R, -1, L.m)
    while len(out) < count:
        zzr = rng.randrange(L.m) & keep
        z = _sqrt(zzr * rinv, L.m)
        if z:
            out.append(z)
    return tuple(out)


# ---------------------------------------------------------------------------------------------- points and case tables
@lru_cache(maxsize=None)
def point_set(curve):
    """names -> points: six random multiples of G, their negatives, infinity; BLS12-377 also T = (q - 1, 0) of order two, A, T - A"""
    rng = random.Random(20377)
    c = pyref.CURVES[curve]
    G = pyref.generator(curve)
    pts = {}
    for i in range(6):
        pts["P%d" % i] = pyref.mul(curve, G, rng.randrange(1, c["r"]))
        pts["-P%d" % i] = pyref.neg(curve, pts["P%d" % i])
    pts["inf"] = None
    if curve == "BLS377":
        T = (c["q"] - 1, 0)
        assert pyref.is_on_curve(curve, T) and pyref.add(curve, T, T) is None
        A = pyref.mul(curve, G, rng.randrange(1, c["r"]))
        pts["T"], pts["A"], pts["T-A"] = T, A, pyref.add(curve, T, pyref.neg(curve, A))
    return pts


def simulate(curve, program, pts, arg=0):
    """The program on affine points, step by step as the hook kernel runs it: (result, events).  events: the operand classes its
    additions and doublings met - inf_left, inf_right, equal, opposite, result_inf, computed_doubled (equal operands of which one
    came out of a formula rather than out of memory), computed_T_doubled (the same, the operand being the point of order two)."""
    ev = set()
    T = (pyref.CURVES[curve]["q"] - 1, 0) if curve == "BLS377" else ("none",)

    def add(a, b):   # a, b: (point, computed)
        (p, pc), (q, qc) = a, b
        if q is None:
            ev.add("inf_right")
            return a
        if p is None:
            ev.add("inf_left")
            return b
        r = pyref.add(curve, p, q)
        if p == q:
            ev.add("equal")
            if pc or qc:
                ev.add("computed_doubled")
                if p == T:
                    ev.add("computed_T_doubled")
        elif p[0] == q[0]:
            ev.add("opposite")
        if r is None:
            ev.add("result_inf")
        return (r, True)

    def dbl(a):
        if a[0] is None:
            return a
        r = pyref.add(curve, a[0], a[0])
        if a[1]:
            ev.add("computed_doubled")
            if a[0] == T:
                ev.add("computed_T_doubled")
        if r is None:
            ev.add("result_inf")
        return (r, True)

    ld = [(p, False) for p in pts]
    inf = (None, False)
    if program == "IDENT":
        acc = ld[0]
    elif program == "ADD":
        acc = add(ld[0], ld[1])
    elif program == "DBL":
        acc = dbl(ld[0])
    elif program == "RUNSUM":
        run = acc = inf
        for j in range(4):
            run = add(run, ld[j])
            acc = add(acc, run)
    elif program == "HORNER":
        acc = ld[0]
        for j in (1, 2):
            for _ in range(arg):
                acc = dbl(acc)
            acc = add(acc, ld[j])
    elif program == "REUSE":
        acc = add(ld[0], ld[1])
        acc = add(acc, acc)
        acc = add(add(acc, ld[2]), ld[3])
    elif program == "TREE":
        lanes = ld[:arg] + [inf] * (64 - arg)
        r = 1
        while r < arg:
            for i in range(0, 64, 2 * r):
                if i + r < arg:
                    lanes[i] = add(lanes[i], lanes[i + r])
            r *= 2
        acc = lanes[0]
    else:
        raise ValueError(program)
    return acc[0], ev


class Case:
    """one base case: the points by value, the program's argument, the expected point and the operand classes it meets"""

    def __init__(self, curve, program, pts, arg=0):
        self.pts, self.arg = list(pts), arg
        self.expect, self.events = simulate(curve, program, self.pts, arg)


@lru_cache(maxsize=None)
def table(curve, program, arg=0):
    """the base cases of a program (for HORNER and TREE: of one arg)"""
    S = point_set(curve)
    names = list(S)
    rnd = [S["P%d" % i] for i in range(6)]
    neg, add, mul = (lambda p: pyref.neg(curve, p)), (lambda p, q: pyref.add(curve, p, q)), (lambda p, k: pyref.mul(curve, p, k))
    rng = random.Random(99 + PROGRAM[program])
    pick = lambda: S[rng.choice(names)]
    cases = []
    if program in ("IDENT", "DBL"):
        cases = [[S[a], None, None, None] for a in names]
    elif program == "ADD":
        cases = [[S[a], S[b], None, None] for a in names for b in names]
    elif program == "RUNSUM":
        for a in names:
            cases.append([S[a], None, None, None])
        for i in range(6):
            cases.append([rnd[i], neg(rnd[i]), rnd[(i + 1) % 6], None])
            cases.append([rnd[i], rnd[(i + 1) % 6], rnd[i], None])   # s = 2P + Q meets run = 2P + Q: a computed sum doubled
        if curve == "BLS377":
            cases.append([S["A"], add(S["T"], neg(mul(S["A"], 2))), S["A"], None])   # ... the sum being T
            cases.append([S["A"], S["T-A"], None, None])
            cases.append([None, S["T"], None, None])
        for _ in range(12):
            cases.append([pick() for _ in range(4)])
    elif program == "HORNER":
        for i in range(6):
            cases.append([rnd[i], rnd[(i + 2) % 6], rnd[(i + 3) % 6], None])
        p0, p1 = rnd[0], rnd[1]
        cases.append([p0, p1, neg(mul(add(mul(p0, 1 << arg), p1), 1 << arg)), None])   # the walk ends at infinity
        cases.append([p0, neg(mul(p0, 1 << arg)), rnd[2], None])                        # ... passes through it
        cases.append([p0, mul(p0, 1 << arg), rnd[2], None])                             # adds the accumulator to its equal
        cases.append([None, p0, p1, None])
        cases.append([p0, None, None, None])
        if curve == "BLS377":
            cases.append([S["T"], p0, p1, None])
            cases.append([S["A"], add(S["T"], neg(mul(S["A"], 1 << arg))), p1, None])   # the walk computes T, then doubles it
        for _ in range(6):
            cases.append([pick(), pick(), pick(), None])
    elif program == "REUSE":
        for i in range(6):
            a, b = rnd[i], rnd[(i + 1) % 6]
            cases.append([a, b, rnd[(i + 2) % 6], rnd[(i + 3) % 6]])
            cases.append([a, b, neg(mul(add(a, b), 2)), rnd[(i + 3) % 6]])   # the sum meets its negative
            cases.append([a, b, mul(add(a, b), 2), rnd[(i + 3) % 6]])        # ... its equal
            cases.append([a, a, rnd[(i + 2) % 6], None])
            cases.append([a, neg(a), b, b])
            cases.append([None, a, None, neg(mul(a, 2))])
        if curve == "BLS377":
            for a in rnd[:3] + [S["A"]]:
                cases.append([a, add(S["T"], neg(a)), rnd[4], rnd[5]])       # a computed T added to itself
                cases.append([a, add(S["T"], neg(a)), None, None])
        for _ in range(8):
            cases.append([pick() for _ in range(4)])
    elif program == "TREE":
        base = [rnd[0]]
        for _ in range(63):
            base.append(add(base[-1], rnd[1]))          # 64 distinct points
        eq = list(base)
        for i in range(0, 64, 4):
            eq[i + 1] = eq[i]                           # equal neighbours (round 1) ...
        eq[2], eq[3] = eq[0], eq[0]                     # ... and equal sums (round 2)
        op = list(base)
        for i in range(0, 64, 8):
            op[i + 1] = neg(op[i])                      # a -P neighbour
        op[4] = None                                    # ... and an infinity among the operands
        mix = [pick() for _ in range(64)]
        cases = [v[:arg] for v in (base, eq, op, mix)]
        if curve == "BLS377" and arg >= 3:
            cases.append(([S["A"], S["T-A"], S["T"], None] + base[4:])[:arg])   # round 1 computes T, round 2 adds T to it
    return [Case(curve, program, c, arg) for c in cases]


Z_MODES = ("one", "shared", "each")


def variants(L):
    """(z mode, representative) a table is crossed with on this law"""
    reps = ("low", "top") + (("weak",) if L.law == "row" else ())
    return [(zm, r) for zm in Z_MODES for r in reps]


def images(L, cases, k):
    """The table crossed with the z modes and representatives: (flat dword list of n k images, expected points, labels)."""
    rng = random.Random(4242)
    wz = weak_zs(L.curve, L.rep) if L.law == "row" else ()
    flat, expect, labels = [], [], []
    for ci, c in enumerate(cases):
        for zm, rep in variants(L):
            shared = rng.randrange(2, L.m)
            for j in range(k):
                P = c.pts[j] if j < len(c.pts) else None
                if rep == "weak":
                    z = wz[0] if zm == "one" else wz[1] if zm == "shared" else wz[j % len(wz)]
                else:
                    z = 1 if zm == "one" else shared if zm == "shared" else rng.randrange(2, L.m)
                flat += encode(L, P, z, rep)
            expect.append(c.expect)
            labels.append("case %d z=%s rep=%s" % (ci, zm, rep))
    return flat, expect, labels


# ---------------------------------------------------------------------------------------------- the device
def run(L, program, exit, k, arg, flat):
    """the hook on n = len(flat) / (k image dwords) cases: a list of result images"""
    n = len(flat) // (k * L.dwords)
    assert n * k * L.dwords == len(flat)
    src = (C.c_uint32 * len(flat))(*flat)
    dst = (C.c_uint32 * (n * L.dwords))()
    rc = blaze_amd.aux().blz_test_law_op(0, pyref.CURVES[L.curve]["id"], L.rep, LAW_ID[L.law], PROGRAM[program], exit, k, arg,
                                         C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), n)
    blaze_amd._lib.check(rc)
    out = list(dst)
    return [out[i * L.dwords:(i + 1) * L.dwords] for i in range(n)]


def failures(L, exit, outs, expect, labels):
    """What is wrong with the result images of an exit: (a) the point, bit-exact, a result at infinity with literally zero zz;
    (b) the bounds the layout promises for the exit."""
    b = L.bounds[EXIT_BOUND[exit]]
    bad = []
    for img, want, label in zip(outs, expect, labels):
        d = decode(L, img)
        why = []
        if d.point != want:
            why.append("point")
        elif want is None and not d.literal_inf:
            why.append("infinity with non-zero zz limbs")
        if d.max_limb > b[4]:
            why.append("limb %#x" % d.max_limb)
        for name, v, f in zip("x y zz zzz".split(), d.values, b[:4]):
            if not L.within(v, f):
                why.append("%s needs %d m" % (name, value_factor(L, v)))
        if why:
            bad.append(label + ": " + ", ".join(why))
    return bad
