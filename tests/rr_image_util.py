"""Host side of the reduced-radix primitive tests (tests/test_rr_image_cases.py, tests/test_gpu_rr_primitives.py): limb images built
and read back with Python integers, the case tables of every op, the expected results, and an exact model of the Shoup product's
truncated quotient.

An image is NL dwords, limb i at dword i; its integer is sum limb_i 2^(B i) whatever the limbs' size.  What an operand admits - every
limb < F 2^B, integer < V m - comes from blz_test_rr_layout, which reads it off the device types; nothing here copies a bound."""
import ctypes as C
import random
from functools import lru_cache

import blaze_amd
from oracle import pyref

OP = {"MUL": 0, "SQR": 1, "MUL2": 2, "PAIR": 3, "DOT": 4, "SHOUP": 5, "SHOUP_U": 6, "SHOUP_QUOT": 7, "NORM": 8, "REDUCE2M": 9, "SUB": 10,
      "SUB_TWICE": 11, "NEG": 12, "CNEG": 13, "BFLY": 14, "CANON": 15, "ZERO": 16, "WORDS": 17, "DFT8": 18}
OP_NAME = {v: k for k, v in OP.items()}
FIELDS = tuple((c, f) for c in sorted(pyref.CURVES) for f in (0, 1))
LAYOUT_WORDS = 8192
WAVE = 64
BR8 = (0, 4, 2, 6, 1, 5, 3, 7)   # dft8_rr's input order


class Variant:
    def __init__(self, op, var, param, ins, outs):
        self.op, self.var, self.param, self.ins, self.outs = op, var, param, ins, outs
        self.name = OP_NAME.get(op, "op%d" % op)

    @property
    def id(self):
        return "%s_%d" % (self.name, self.var)


class Layout:
    def __init__(self, curve, field):
        w = (C.c_uint32 * LAYOUT_WORDS)()
        blaze_amd._lib.check(blaze_amd.aux().blz_test_rr_layout(pyref.CURVES[curve]["id"], field, w))
        self.curve, self.field = curve, field
        self.B, self.NL, self.H, self.NKM, self.FS, self.E, self.N32, self.POS_DOT, self.T2M, count, used = w[0:11]
        self.mask = (1 << self.B) - 1
        self.R = 1 << self.E
        self.m = sum(w[16 + i] << (self.B * i) for i in range(self.NL))
        self.Rinv = pow(self.R, -1, self.m)
        self.variants = []
        pos = 16 + self.NL
        for _ in range(count):
            op, var, kin, kout, param = w[pos:pos + 5]
            b = [(w[pos + 5 + 2 * i], w[pos + 6 + 2 * i]) for i in range(kin + kout)]
            self.variants.append(Variant(op, var, param, tuple(b[:kin]), tuple(b[kin:])))
            pos += 5 + 2 * (kin + kout)
        assert pos == used <= LAYOUT_WORDS
        self.by = {(v.op, v.var): v for v in self.variants}

    @property
    def name(self):
        return "%s_%s" % (self.curve, "Fr" if self.field else "Fq")

    def value(self, img):
        return sum(x << (self.B * i) for i, x in enumerate(img))

    def within(self, img, bound):
        """is the image inside what a type (F, V) declares?  (1, 0): normalised limbs, any integer; (0, .): no limb image"""
        F, V = bound
        if F == 0:
            return all(0 <= x < 1 << 32 for x in img)
        return all(0 <= x < F << self.B for x in img) and (V == 0 or self.value(img) < V * self.m)


@lru_cache(maxsize=None)
def layout(curve, field):
    L = Layout(curve, field)
    assert L.m == pyref.CURVES[curve]["r" if field else "q"], "the device's modulus is not the oracle's"
    return L


# ---------------------------------------------------------------------------------------------- images
def split(L, value):
    """normalised: NL - 1 limbs of B bits, the top limb keeps the rest"""
    return [(value >> (L.B * i)) & L.mask for i in range(L.NL - 1)] + [value >> (L.B * (L.NL - 1))]


def resplit(L, limbs, F, mode, rng=None):
    """The same integer with limbs up to F 2^B - 1: c 2^B moves from limb i + 1 into limb i.  bottom: as much as fits, from the top
    limb down (the low limbs end up heaviest); max: as much as fits, from the bottom up; even / odd: every second limb takes all it can
    from the one above; rand: random amounts in a random order."""
    x = list(limbs)
    cap = (F << L.B) - 1
    order = {"bottom": range(L.NL - 2, -1, -1), "max": range(L.NL - 1), "even": range(0, L.NL - 1, 2), "odd": range(1, L.NL - 1, 2)}.get(mode)
    if mode == "rand":
        order = list(range(L.NL - 1))
        rng.shuffle(order)
    for i in order:
        c = min(x[i + 1], (cap - x[i]) >> L.B)
        if mode == "rand":
            c = rng.randrange(c + 1)
        x[i] += c << L.B
        x[i + 1] -= c
    return x


def all_ones_below(L, bound):
    """the largest integer below `bound` whose lower NL - 1 limbs are all 2^B - 1"""
    low = (1 << (L.B * (L.NL - 1))) - 1
    top = (bound - 1) >> (L.B * (L.NL - 1))
    v = (top << (L.B * (L.NL - 1))) | low
    if v >= bound:
        v -= 1 << (L.B * (L.NL - 1))
    return v if v >= 0 else None


def values(L, V, rng, nrand=12):
    """(label, integer) below V m: the edges of every multiple of m (sampled above 64), the top of the range, all-ones limbs, random"""
    m = L.m
    ones = all_ones_below(L, V * m)
    out = [("Vm-1", V * m - 1)] + ([("ones", ones)] if ones is not None else []) + [("0", 0), ("1", 1), ("m-1", m - 1)]
    ks = list(range(1, V)) if V <= 64 else sorted(set([1, 2, 3, V // 2, V - 2, V - 1] + [rng.randrange(1, V) for _ in range(24)]))
    for k in ks:
        out += [("%dm-1" % k, k * m - 1), ("%dm" % k, k * m), ("%dm+1" % k, k * m + 1)]
    out += [("rand%d" % i, rng.randrange(V * m)) for i in range(nrand)]
    seen, uniq = set(), []
    for lab, v in out:
        if v not in seen and 0 <= v < V * m:
            seen.add(v)
            uniq.append((lab, v))
    return uniq


MODES = ("bottom", "max", "even", "odd", "rand")


def operand_images(L, bound, rng, nrand=12):
    """(label, limbs) for an operand of type (F, V): every value of values() normalised and, for F > 1, re-split in every mode.
    The first entries are the PEAKS: the range's top and the all-ones value in their heaviest splits."""
    F, V = bound
    out, peaks = [], []
    for lab, v in values(L, V, rng, nrand):
        n = split(L, v)
        imgs = [(lab + "/norm", n)]
        if F > 1:
            imgs += [("%s/%s" % (lab, mode), resplit(L, n, F, mode, rng)) for mode in MODES]
        (peaks if lab in ("Vm-1", "ones") else out).extend(imgs)
    return peaks, peaks + out


def words_images(L, rng, bound=None, n=40):
    """raw 32-bit word images: integers up to 2^(32 N32) - 1 (or below `bound`), N32 words in an image of NL dwords"""
    top = min(bound, 1 << (32 * L.N32)) if bound else 1 << (32 * L.N32)
    vals = [("0", 0), ("1", 1), ("m-1", L.m - 1), ("m", L.m), ("m+1", L.m + 1), ("top-1", top - 1), ("top-2", top - 2), ("2m", min(2 * L.m, top - 1)),
            ("half", top >> 1)] + [("rand%d" % i, rng.randrange(top)) for i in range(n)]
    out = []
    for lab, v in vals:
        if 0 <= v < top:
            out.append((lab, [(v >> (32 * i)) & 0xffffffff for i in range(L.N32)] + [0] * (L.NL - L.N32)))
    return out


def words_value(img):
    return sum(x << (32 * i) for i, x in enumerate(img))


# ---------------------------------------------------------------------------------------------- the Montgomery product, exactly
def mont_model(L, pairs):
    """(sum a_i b_i) / Rrr by product scanning as the device does it (rr_mul_ref's columns): the result limbs, which the quotient
    digits determine uniquely.  Asserts that no column sum leaves 64 bits - the budget rr_cols_ok proves - on these very limbs."""
    NL, B, mask = L.NL, L.B, L.mask
    ml = split(L, L.m)
    n0 = (-pow(L.m, -1, 1 << B)) % (1 << B)
    acc, q, t = 0, [0] * NL, [0] * NL
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - NL + 1), min(k, NL - 1)
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        if k < NL:
            acc += sum(q[i] * ml[k - i] for i in range(k))
            q[k] = ((acc & 0xffffffff) * n0) & mask
            acc += q[k] * ml[0]
        else:
            acc += sum(q[i] * ml[k - i] for i in range(k - NL + 1, NL))
            t[k - NL] = acc & mask
        assert acc < 1 << 64, "a column sum leaves 64 bits"
        acc >>= B
    assert acc < 1 << 32
    t[NL - 1] = acc
    return t


# ---------------------------------------------------------------------------------------------- the Shoup product, exactly
def shoup_entry(L, w):
    return w, (w * L.R) // L.m


def shoup_model(L, x, w):
    """rr_mul_shoup on the limbs x (any the type admits) and the entry of the canonical w, as the device computes it: the high half
    of x wq summed from column NL - 2 up, then x w + q (Rrr - m) modulo Rrr in NL columns, then the T2M correction.
    Returns (result limbs, q_trunc, floor(x wq / Rrr), the result before the correction as an integer)."""
    NL, B, mask = L.NL, L.B, L.mask
    wl, wql, mbar = split(L, w), split(L, (w * L.R) // L.m), split(L, L.R - L.m)
    acc, q = 0, [0] * NL
    for K in range(NL - 2, 2 * NL - 1):
        acc += sum(x[i] * wql[K - i] for i in range(max(0, K - NL + 1), min(K, NL - 1) + 1))
        assert acc < 1 << 64
        if K >= NL:
            q[K - NL] = acc & mask
        acc >>= B
    q[NL - 1] = acc & 0xffffffff
    acc, r = 0, [0] * NL
    for K in range(NL):
        acc += sum(x[i] * wl[K - i] + q[i] * mbar[K - i] for i in range(K + 1))
        assert acc < 1 << 64
        r[K] = acc & mask
        acc >>= B
    raw = L.value(r)
    if r[NL - 1] >= L.T2M:
        r = split(L, raw - L.m) if raw >= L.m else r
    return r, L.value(q), (L.value(x) * ((w * L.R) // L.m)) >> L.E, raw


def quot_ws(L, rng, nrand=24):
    """the twiddles of the SHOUP_QUOT table: the edges of [0, m), the powers of two and their neighbours, random"""
    m = L.m
    ws = [0, 1, 2, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2]
    j = 1
    while (1 << j) - 1 < m:
        ws += [w for w in ((1 << j) - 1, 1 << j, (1 << j) + 1) if w < m]
        j += 1
    ws += [rng.randrange(m) for _ in range(nrand)]
    return sorted(set(ws))


@lru_cache(maxsize=None)
def truncation_cases(curve, field, want=48, seed=2929):
    """(x, w) on which the truncated quotient is one below floor(x wq / Rrr) BY THE MODEL: w with an odd wq, x = s wq^-1 mod Rrr for a
    small s, so that frac(x wq / Rrr) = s / Rrr lies under what the columns left out are worth.  x is a normalised value below
    2^HEAD m, the widest the Shoup product's operand type admits.  Also returns the number of tries."""
    L = layout(curve, field)
    rng = random.Random(seed)
    out, tries = [], 0
    smax = 1 << (L.B * (L.NL - 1) - 3)
    while len(out) < want and tries < 20000:
        tries += 1
        w = rng.randrange(1, L.m)
        wq = (w * L.R) // L.m
        if wq % 2 == 0:
            continue
        x = rng.randrange(1, smax) * pow(wq, -1, L.R) % L.R
        if x >= (1 << L.H) * L.m:
            continue
        _, qt, qf, _ = shoup_model(L, split(L, x), w)
        if qt == qf - 1:
            out.append((x, w))
    return out, tries


# ---------------------------------------------------------------------------------------------- case tables
class Cases:
    """the cases of one (field, op, variant): .ins[i] the k_in operand images of case i, .labels[i], .extra[i] what the expectation
    needs beyond the images"""

    def __init__(self, L, v):
        self.L, self.v, self.ins, self.labels, self.extra = L, v, [], [], []

    def add(self, label, imgs, extra=None):
        assert len(imgs) == len(self.v.ins)
        self.ins.append([list(x) for x in imgs])
        self.labels.append(label)
        self.extra.append(extra)

    def flat(self):
        return [x for case in self.ins for img in case for x in img]


def _combine(c, pools, rng, cap=1400):
    """operand pools [(peaks, all)] -> cases: every combination of the peaks (aligned where there are too many), then every image of
    every operand at least once against cycling partners"""
    k = len(pools)
    peaks = [p[0] for p in pools]
    if k <= 2:
        def rec(j, cur):
            if j == k:
                c.add(" | ".join(x[0] for x in cur), [x[1] for x in cur])
                return
            for x in peaks[j]:
                rec(j + 1, cur + [x])
        rec(0, [])
    else:
        for i in range(max(len(p) for p in peaks)):
            for shift in (0, 1, 2):
                cur = [peaks[j][(i + shift * j) % len(peaks[j])] for j in range(k)]
                c.add(" | ".join(x[0] for x in cur), [x[1] for x in cur])
    n = min(cap, max(len(p[1]) for p in pools))
    for i in range(n):   # (step 1: a pool no longer than n is walked whole; the offsets keep equal pools from pairing an image with itself)
        cur = [pools[j][1][(i + 17 * j) % len(pools[j][1])] for j in range(k)]
        c.add(" | ".join(x[0] for x in cur), [x[1] for x in cur])
    for i in range(64):
        cur = [rng.choice(pools[j][1]) for j in range(k)]
        c.add(" | ".join(x[0] for x in cur), [x[1] for x in cur])


def _pools(L, bounds, rng, nrand=12):
    cache, out = {}, []
    for b in bounds:
        if b not in cache:
            cache[b] = operand_images(L, b, rng, nrand)
        out.append(cache[b])
    return out


@lru_cache(maxsize=None)
def cases(curve, field, op, var):
    L = layout(curve, field)
    v = L.by[(op, var)]
    rng = random.Random(1000 * op + var + 7)
    c = Cases(L, v)
    name = v.name
    if name in ("MUL", "SQR", "MUL2", "PAIR", "NORM", "REDUCE2M", "SUB", "SUB_TWICE", "NEG", "BFLY", "CANON"):
        _combine(c, _pools(L, v.ins, rng), rng)
        if name in ("SUB", "SUB_TWICE", "NEG"):
            # b = 0 and the b with the largest top limb a value below 2^(J-1) m can have, against every peak of a
            bb = v.ins[-1]
            tops = [("0/norm", split(L, 0)), ("Vm-1/norm", split(L, bb[1] * L.m - 1))]
            for lab, b in tops:
                if name == "NEG":
                    c.add(lab, [b])
                else:
                    for la, a in operand_images(L, v.ins[0], rng)[0]:
                        c.add(la + " | " + lab, [a, b])
    elif name == "CNEG":
        for lab, b in operand_images(L, v.ins[0], rng)[1]:
            for s in (0, 1, 0x80000000):
                c.add("%s | sign=%#x" % (lab, s), [b, [s] + [0] * (L.NL - 1)])
    elif name == "DOT":
        n = v.param
        pa, pb = operand_images(L, v.ins[0], rng, 6), operand_images(L, v.ins[n], rng, 6)
        for i in range(len(pa[0])):          # every product of the column at its peak
            for j in range(len(pb[0])):
                c.add("all %s x %s" % (pa[0][i][0], pb[0][j][0]), [pa[0][i][1]] * n + [pb[0][j][1]] * n)
        for i in range(300):
            a = [pa[1][(i + 5 * t) % len(pa[1])] for t in range(n)]
            b = [pb[1][(7 * i + 3 * t) % len(pb[1])] for t in range(n)]
            c.add("%s x %s" % (",".join(x[0] for x in a), ",".join(x[0] for x in b)), [x[1] for x in a] + [x[1] for x in b])
    elif name in ("SHOUP", "SHOUP_U"):
        peaks, pool = operand_images(L, v.ins[0], rng)
        ws = quot_ws(L, rng, 16)
        rows = []   # (label, x limbs, w)
        for i, (lab, x) in enumerate(pool):
            rows.append((lab, x, ws[(5 * i) % len(ws)]))
        for lab, x in peaks:                 # the top of the range against many twiddles: f + x eps / Rrr as large as it gets
            for w in [L.m - 1, L.m - 2, (L.m + 1) // 2] + [rng.randrange(L.m) for _ in range(12)]:
                rows.append((lab, x, w))
        for d in range(1, 17):
            rows.append(("Vm-1-%d" % d, split(L, v.ins[0][1] * L.m - 1 - d), rng.randrange(L.m)))
        if v.ins[0][1] == 1 << L.H:          # the crafted truncation cases are values below 2^HEAD m
            for x, w in truncation_cases(curve, field)[0]:
                rows.append(("trunc", split(L, x), w))
                if v.ins[0][0] > 1:
                    rows.append(("trunc/rand", resplit(L, split(L, x), v.ins[0][0], "rand", rng), w))
        if name == "SHOUP":
            for lab, x, w in rows:
                c.add("%s | w=%#x" % (lab, w), [x, split(L, w)], w)
        else:
            # a wave multiplies by the twiddle of its FIRST case: the other lanes carry one the device must not use
            while len(rows) % WAVE:
                rows.append(rows[len(rows) % 37])
            for w in (L.m - 1, 0, all_ones_below(L, L.m)):     # whole waves on the edges of the twiddle's own range
                rows += [(pool[(3 * i) % len(pool)][0], pool[(3 * i) % len(pool)][1], w) for i in range(WAVE)]
            for i, (lab, x, w) in enumerate(rows):
                first = rows[i - i % WAVE][2]
                decoy = first if (i // WAVE) % 2 == 0 else (w if w != first else (w + 1) % L.m)
                c.add("%s | wave w=%#x" % (lab, first), [x, split(L, decoy if i % WAVE else first)], first)
    elif name == "SHOUP_QUOT":
        for w in quot_ws(L, rng):
            if v.param == 0:
                c.add("w=%#x" % w, [split(L, w)], w)
            else:
                for k in (0, 1):
                    x = w * L.R % L.m + k * L.m
                    c.add("w=%#x + %dm" % (w, k), [split(L, x)], w)
        for lab, x in operand_images(L, v.ins[0], rng)[1]:     # the edges of the operand's own range
            c.add(lab, [x], L.value(x) * (L.Rinv if v.param else 1) % L.m)
    elif name == "ZERO":
        pa, pb = operand_images(L, v.ins[0], rng), operand_images(L, v.ins[1], rng)
        for i, (lab, a) in enumerate(pa[1]):
            c.add(lab + " | " + pb[1][(3 * i) % len(pb[1])][0], [a, pb[1][(3 * i) % len(pb[1])][1]])
        # equal residues, every pair of multiples of m the two types admit (sampled)
        Fa, Va = v.ins[0]
        Fb, Vb = v.ins[1]
        for t in range(200):
            r = rng.choice([0, 1, L.m - 1, rng.randrange(L.m)])
            ka, kb = rng.randrange(Va), rng.randrange(Vb)
            if t < 8:
                ka, kb = (Va - 1, 0) if t % 2 else (0, Vb - 1)
            a = resplit(L, split(L, r + ka * L.m), Fa, rng.choice(MODES), rng)
            b = resplit(L, split(L, r + kb * L.m), Fb, rng.choice(MODES), rng)
            c.add("equal residues %dm, %dm" % (ka, kb), [a, b])
    elif name == "WORDS":
        if var == 1:
            for lab, a in operand_images(L, v.ins[0], rng, 40)[1]:
                c.add(lab, [a])
        else:
            for lab, w in words_images(L, rng, v.param * L.m if v.param else None):
                c.add(lab, [w])
    elif name == "DFT8":
        assert field == 1
        w8 = pyref.omega(curve, 3)
        ws = [split(L, pow(w8, k, L.m)) for k in (1, 2, 3)]
        peaks, pool = operand_images(L, v.ins[0], rng, 24)
        top = dict(peaks)["Vm-1/norm"]
        c.add("all Vm-1", [top] * 8 + ws, w8)
        for j in range(8):
            c.add("Vm-1 at %d, 0 elsewhere" % j, [top if i == j else split(L, 0) for i in range(8)] + ws, w8)
            c.add("0 at %d, Vm-1 elsewhere" % j, [split(L, 0) if i == j else top for i in range(8)] + ws, w8)
        for i in range(240):
            xs = [pool[(i + 9 * j) % len(pool)] if i % 2 else rng.choice(pool) for j in range(8)]
            c.add(",".join(x[0] for x in xs), [x[1] for x in xs] + ws, w8)
    else:
        raise KeyError("no case table for op %s" % name)
    return c


# ---------------------------------------------------------------------------------------------- running and judging
def run(L, v, c):
    """one launch: the k_out result images of every case"""
    n, flat = len(c.ins), c.flat()
    kin, kout = len(v.ins), len(v.outs)
    assert len(flat) == n * kin * L.NL
    src = (C.c_uint32 * len(flat))(*flat)
    dst = (C.c_uint32 * (n * kout * L.NL))()
    blaze_amd._lib.check(blaze_amd.aux().blz_test_rr_op(0, pyref.CURVES[L.curve]["id"], L.field, v.op, v.var, C.cast(src, C.c_void_p),
                                                         C.cast(dst, C.c_void_p), n))
    d = list(dst)
    return [[d[(i * kout + j) * L.NL:(i * kout + j + 1) * L.NL] for j in range(kout)] for i in range(n)]


def expect(L, v, ins, extra):
    """What the results of one case must be: a list, one entry per result image -
    ("eq", integer) the exact integer, ("res", residue) the residue mod m, ("flags", {index: value}), ("words", integer),
    ("words_res", residue) words holding that residue below 2m, ("maybe", bool) dword 2 must be 1 when the bool is set."""
    m, val, name = L.m, L.value, v.name
    a = [val(x) for x in ins]
    def prod(*pairs):   # the Montgomery product of sum a_i b_i: the model's limbs and the residue they must have
        return ("limbs", mont_model(L, [(ins[i], ins[j]) for i, j in pairs]), sum(a[i] * a[j] for i, j in pairs) * L.Rinv % m)

    if name == "MUL":
        p = prod((0, 1))
        return [p, p]
    if name == "SQR":
        return [prod((0, 0))]
    if name == "MUL2":
        return [prod((0, 1), (2, 3))]
    if name == "PAIR":
        return [prod((0, 1)), prod((2, 3))] if v.param == 0 else [prod((0, 0)), prod((1, 1))]
    if name == "DOT":
        n = v.param
        return [prod(*[(i, n + i) for i in range(n)])]
    if name in ("SHOUP", "SHOUP_U"):
        w = extra
        return [("limbs", shoup_model(L, ins[0], w)[0], a[0] * w % m), ("eq", w), ("eq", (w * L.R) // m)]
    if name == "SHOUP_QUOT":
        return [("eq", extra), ("eq", (extra * L.R) // m)]
    if name == "NORM":
        return [("eq", a[0])]
    if name == "REDUCE2M":
        return [("res", a[0] % m)]
    J = v.param
    if name == "SUB":
        return [("eq", a[0] - a[1] + (m << J))]
    if name == "SUB_TWICE":
        return [("eq", a[0] - 2 * a[1] + (m << (J + 1)))]
    if name == "NEG":
        return [("eq", (m << J) - a[0])]
    if name == "CNEG":
        return [("eq", (m << J) - a[0] if ins[1][0] and a[0] else a[0])]   # (a literal zero stays zero)
    if name == "BFLY":
        k = v.outs[1][1] - v.ins[0][1]     # the multiple of m the difference carries: V_d - V_u
        return [("eq", a[0] + a[1]), ("eq", a[0] - a[1] + k * m)]
    if name == "CANON":
        return [("eq", a[0] % m)]
    if name == "ZERO":
        return [("flags", {0: int(a[0] % m == 0), 1: int(not any(ins[0])), 3: int(a[1] % m == 0)}, (a[0] - a[1]) % m == 0)]
    if name == "WORDS":
        R32 = 1 << (32 * L.N32)
        if v.var == 0:
            w = words_value(ins[0])
            return [("eq", w), ("res", w * L.R % m)]
        if v.var == 1:
            return [("words", a[0]), ("words_res", a[0] * R32 * L.Rinv % m)]
        return [("res", words_value(ins[0]) * L.R * pow(R32, -1, m) % m)]
    if name == "DFT8":
        x = [0] * 8
        for j in range(8):
            x[BR8[j]] = a[j]
        return [("res", sum(x[n] * pow(extra, n * k, m) for n in range(8)) % m) for k in range(8)]
    raise KeyError(name)


def judge(L, v, ins, outs, extra):
    """None, or what is wrong with the results of one case"""
    want = expect(L, v, ins, extra)
    assert len(want) == len(outs) == len(v.outs)
    for j, (w, out, bound) in enumerate(zip(want, outs, v.outs)):
        kind = w[0]
        if bound[0] and not L.within(out, bound):
            return "result %d leaves its declared bound (F, V) = %s: limbs %s, value / m = %.4f" % (
                j, bound, [hex(x) for x in out], L.value(out) / L.m)
        if kind == "eq" and L.value(out) != w[1]:
            return "result %d is %#x, not the integer %#x" % (j, L.value(out), w[1])
        if kind == "res" and L.value(out) % L.m != w[1]:
            return "result %d has residue %#x, not %#x" % (j, L.value(out) % L.m, w[1])
        if kind == "limbs":
            if L.value(out) % L.m != w[2]:
                return "result %d has residue %#x, not %#x" % (j, L.value(out) % L.m, w[2])
            if list(out) != list(w[1]):
                return "result %d differs from the exact model of the device's columns: %s, model %s" % (j, [hex(x) for x in out], [hex(x) for x in w[1]])
        if kind == "flags":
            for i, f in w[1].items():
                if out[i] != f:
                    return "flag %d is %d, not %d" % (i, out[i], f)
            if w[2] and out[2] != 1:
                return "rr_maybe_equal is false on equal residues"
            if out[2] not in (0, 1) or any(out[4:]):
                return "stray flag words %s" % out
        if kind == "words" and (words_value(out[:L.N32]) != w[1] or any(out[L.N32:])):
            return "result %d holds the words of %#x, not of %#x" % (j, words_value(out[:L.N32]), w[1])
        if kind == "words_res":
            x = words_value(out[:L.N32])
            if x % L.m != w[1] or x >= 2 * L.m or any(out[L.N32:]):
                return "result %d holds %#x: residue %#x wanted, below 2m" % (j, x, w[1])
    return None


def failures(L, v, c, outs):
    bad = []
    for i, (ins, out) in enumerate(zip(c.ins, outs)):
        why = judge(L, v, ins, out, c.extra[i])
        if why:
            bad.append("%s %s case %d [%s]: %s; operands %s" % (L.name, v.id, i, c.labels[i], why, [[hex(x) for x in img] for img in ins]))
    return bad
