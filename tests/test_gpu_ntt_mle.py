"""Multilinear tables on resident buffers (blz_ntt_vec_mle_fold / _round / _eq) on the device: bind a variable, take a round
polynomial, build eq(tau, .) - and what they are for, a whole Spartan-style sumcheck over the vectors vec_spmv produces.  Every
expected value is Python integer arithmetic and every comparison is byte for byte: any 256-bit input word counts as its
residue, every output word is canonical, and no byte outside the words an op owns changes.  The input recipe is the house one
(tests/ntt_vec_util.py): the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random 256-bit words behind."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_mle_util import challenges, fill as _fill, fold_ref, interpolate, pairs   # `fill` is a local name in the tests below
from ntt_spmv_util import _inputs, _u32, sparse_rows, spmv_ref
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
SUM, DOT = NTTClient.FOLD_SUM, NTTClient.FOLD_DOT
LOGNS = [1, 6, 9, 11]   # one pair; less than a block; one block; several blocks (the round: through the workspace)


def round_ref(tables, r, length, points, low):
    prs = [pairs(a, length, low) for a in tables]
    out = []
    for t in range(points):
        s = 0
        for p in range(length // 2):
            term = 1
            for pr in prs:
                lo, hi = pr[p]
                term = term * (lo + t * (hi - lo)) % r
            s += term
        out.append(s % r)
    return out


def eq_ref(tau, r):
    tab = [1]
    for t in tau:
        tab = [v * (1 - t) % r for v in tab] + [v * t % r for v in tab]
    return tab


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", LOGNS)
def test_fold_against_python_integers(gpu, field, logn):
    """len = 2, a middle power and n, both pairings; buffer -> other buffer, device words -> buffer, buffer -> device words, in
    place on a buffer and on device words, a periodic source of 1 and of 4 words; r walks through 0, 1, r - 1, r + 1 and a
    random word >= r.  The destination is random bytes before every call and only its first len / 2 words may change; a source
    that is not the destination keeps its bytes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(r, n, 900 * logn + len(field))
    ab = _pack(a)
    cl = _client(field, logn)
    rs = challenges(r, logn)
    drs = [cl.scalar(v) for v in rs]
    src, dstw = _dev(ab), DeviceBuffer(0, 32 * n)
    periodic = [(_dev(ab[:32 * c]), a[:c]) for c in (1, 4) if c <= n]
    turn = 0
    for length in sorted({2, 1 << ((logn + 1) // 2), n}):
        half = length // 2
        for low in (False, True):
            def want_of(vals):
                return _pack(fold_ref(vals, r, rs[turn % 5], length, low))

            def check(got, fill, vals, what):
                assert got[:32 * half] == want_of(vals), (what, length, low, rs[turn % 5])
                assert got[32 * half:] == fill[32 * half:], (what, length, low, "bytes behind the words written")

            for what in ("buffer -> buffer", "words -> buffer", "buffer -> words", "in place, buffer", "in place, words", "periodic 1", "periodic 4"):
                fill = _fill(n, turn + 1)
                dr = drs[turn % 5]
                if what == "buffer -> buffer":
                    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, fill))
                    cl.vec_mle_fold(1, 0, dr, length, low); cl.wait_result()
                    check(bytes(cl.result(1)), fill, a, what)
                    assert bytes(cl.result(0)) == ab
                elif what == "words -> buffer":
                    cl.set_data(NTTInput(0, fill))
                    cl.vec_mle_fold(0, src, dr, length, low); cl.wait_result()
                    check(bytes(cl.result(0)), fill, a, what)
                    assert bytes(src.download()) == ab
                elif what == "buffer -> words":
                    cl.set_data(NTTInput(1, ab)); dstw.upload(fill)
                    cl.vec_mle_fold(dstw, 1, dr, length, low); cl.wait_result()
                    check(bytes(dstw.download()), fill, a, what)
                    assert bytes(cl.result(1)) == ab
                elif what == "in place, buffer":
                    cl.set_data(NTTInput(1, ab))
                    cl.vec_mle_fold(1, 1, dr, length, low); cl.wait_result()
                    check(bytes(cl.result(1)), ab, a, what)
                elif what == "in place, words":
                    dstw.upload(ab)
                    cl.vec_mle_fold(dstw, dstw, dr, length, low); cl.wait_result()
                    check(bytes(dstw.download()), ab, a, what)
                else:
                    c = int(what[-1])
                    if c > n:
                        continue
                    d, vals = periodic[0 if c == 1 else 1]
                    cl.set_data(NTTInput(0, fill))
                    cl.vec_mle_fold(0, d, dr, length, low); cl.wait_result()
                    check(bytes(cl.result(0)), fill, vals, what)
                turn += 1
    assert turn >= 10
    cl.close()
    for d in drs + [src, dstw] + [p[0] for p in periodic]:
        d.free()


def test_fold_second_turn_of_the_grid_stride_loop(gpu):
    """2^20 output words are two sweeps of the 2048 x 256 launch grid.  BLS12-381, len = n = 2^21: the default pairing from
    buffer 0 into buffer 1, BLZ_MLE_LOW in place (through the scratch).  Every word is checked, and the upper half stays."""
    field, logn = "BLS381", 21
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    raw = random.Random(2100).randbytes(32 * n)
    a = _unpack(raw)
    rr = _words(2101, 1)[0]
    cl = _client(field, logn)
    dr = cl.scalar(rr)
    cl.set_data(NTTInput(0, raw))
    cl.vec_mle_fold(1, 0, dr)
    cl.wait_result()
    half = n // 2
    assert bytes(cl.result(1)) == _pack([(lo + rr * (a[p + half] - lo)) % r for p, lo in enumerate(a[:half])]) + bytes(32 * half)
    cl.vec_mle_fold(0, 0, dr, low=True)
    cl.wait_result()
    assert bytes(cl.result(0)) == _pack([(a[2 * p] + rr * (a[2 * p + 1] - a[2 * p])) % r for p in range(half)]) + raw[32 * half:]
    cl.close()
    dr.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", LOGNS)
def test_round_against_python_integers(gpu, field, logn):
    """k = 1, 2, 3 operands x points = 1 .. 4 x both pairings at len = n (and len = n / 2 for k = 3), operands drawn from the
    two buffers, n device words, periodic words and the same table twice.  d_out has a guard word behind it.  out[0] + out[1] is
    the SUM (k = 1) or DOT (k = 2) of the table computed by the existing reductions."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    t0, t1, t2 = (_inputs(r, n, 1000 * logn + len(field) + i) for i in range(3))
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(t0)))
    cl.set_data(NTTInput(1, _pack(t1)))
    w = _dev(_pack(t2))
    pc = min(4, n)
    per = _dev(_pack(t2[:pc]))
    tab = {"b0": (0, t0), "b1": (1, t1), "w": (w, t2), "p": (per, t2[:pc])}
    combos = {1: [("b0",), ("w",), ("p",)], 2: [("b0", "b1"), ("b0", "b0"), ("w", "p")], 3: [("b0", "b1", "w"), ("w", "w", "b1"), ("b0", "p", "b1")]}
    guard = bytes(range(100, 132))
    turn = 0
    for k in (1, 2, 3):
        for points in (1, 2, 3, 4):
            for low in (False, True):
                names = combos[k][turn % 3]
                turn += 1
                for length in ([n, n // 2] if k == 3 and n >= 4 else [n]):
                    out = _dev(_fill(points, turn) + guard)
                    ops = [tab[x][0] for x in names] + [None] * (3 - k)
                    got = cl.vec_mle_round(*ops, points=points, length=length, low=low, out=out)
                    cl.wait_result()
                    assert got is out
                    data = bytes(out.download())
                    want = round_ref([tab[x][1] for x in names], r, length, points, low)
                    assert data == _pack(want) + guard, (names, points, low, length)
                    out.free()
                if k < 3 and points >= 2:
                    ops = [tab[x][0] for x in names]
                    whole = cl.vec_reduce(SUM if k == 1 else DOT, *ops)
                    cl.wait_result()
                    assert _word(whole) == (want[0] + want[1]) % r, (names, points, low)
                    whole.free()
    # points defaults to k + 1
    out = cl.vec_mle_round(0, 1)
    cl.wait_result()
    assert out.nbytes == 96 and bytes(out.download()) == _pack(round_ref([t0, t1], r, n, 3, False))
    assert bytes(cl.result(0)) == _pack(t0) and bytes(cl.result(1)) == _pack(t1) and bytes(w.download()) == _pack(t2)
    cl.close()
    for d in (w, per, out):
        d.free()


def test_round_second_turn_of_the_grid_stride_loop(gpu):
    """BLS12-381, len = n = 2^21, k = 2, points = 3: every lane owns two pairs and 2048 partials per point meet in the
    workspace."""
    field, logn = "BLS381", 21
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    ra, rb = random.Random(2110).randbytes(32 * n), random.Random(2111).randbytes(32 * n)
    a, b = _unpack(ra), _unpack(rb)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ra))
    cl.set_data(NTTInput(1, rb))
    out = cl.vec_mle_round(0, 1, points=3)
    cl.wait_result()
    half = n // 2
    s = [0, 0, 0]
    for p in range(half):
        la, lb = a[p], b[p]
        da, db = a[p + half] - la, b[p + half] - lb
        s[0] += la * lb
        s[1] += (la + da) * (lb + db)
        s[2] += (la + 2 * da) * (lb + 2 * db)
    assert bytes(out.download()) == _pack([v % r for v in s])
    cl.close()
    out.free()


@pytest.mark.parametrize("field", FIELDS)
def test_eq_against_python_integers(gpu, field):
    """m = 0, 1, 5, 8, 10 (one tile), 11, 13 (two levels) on one handle of 2^13 positions; points of unmasked random words (most
    of them >= r) and points that hold 0, 1, r - 1, r + 1 and 2^256 - 1.  Into a buffer and into device words full of random
    bytes: the bytes beyond 2^m words stay.  Into exactly 2^m device words: their SUM, read periodically over the n positions,
    is n / 2^m - the table adds up to 1."""
    logn = 13
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    dstw = DeviceBuffer(0, 32 * n)
    for m in (0, 1, 5, 8, 10, 11, 13):
        edges = [0, 1, r - 1, r + 1, TOP]
        for kind, tau in (("random", _words(77 * m + len(field), m)), ("edges", [(_words(m, m)[i] if i % 2 else edges[(i // 2) % 5]) for i in range(m)])):
            point = _dev(_pack(tau)) if m else None
            want = _pack(eq_ref(tau, r))
            fill = _fill(n, m + 3)
            cl.set_data(NTTInput(1, fill))
            cl.vec_mle_eq(1, point, m); cl.wait_result()
            assert bytes(cl.result(1)) == want + fill[len(want):], (m, kind, "buffer")
            dstw.upload(fill)
            cl.vec_mle_eq(dstw, point, m); cl.wait_result()
            assert bytes(dstw.download()) == want + fill[len(want):], (m, kind, "device words")
            exact = _dev(_fill(1 << m, m))
            cl.vec_mle_eq(exact, point); cl.wait_result()
            assert bytes(exact.download()) == want
            total = cl.vec_reduce(SUM, exact); cl.wait_result()
            assert _word(total) == (n >> m) % r, (m, kind)
            for d in (exact, total, point):
                if d is not None:
                    d.free()
    cl.close()
    dstw.free()


def test_eq_three_levels(gpu):
    """BLS12-381, m = 21: variables [0, 10) | [10, 20) | [20, 21).  4096 sampled positions against the product formula, SUM = 1,
    and DOT(f, eq(tau)) = f folded 21 times at the same point (top variable first), the last fold into one device word."""
    field, m = "BLS381", 21
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    tau = _words(2120, m)
    cl = _client(field, m)
    point = _dev(_pack(tau))
    cl.vec_mle_eq(0, point); cl.wait_result()
    table = bytes(cl.result(0))
    rng = random.Random(2121)
    for p in [0, 1, 1023, 1024, n - 1] + [rng.randrange(n) for _ in range(4091)]:
        v = 1
        for i, t in enumerate(tau):
            v = v * (t if (p >> i) & 1 else 1 - t) % r
        assert table[32 * p: 32 * p + 32] == v.to_bytes(32, "little"), p
    total = cl.vec_reduce(SUM, 0); cl.wait_result()
    assert _word(total) == 1
    cl.set_data(NTTInput(1, random.Random(2122).randbytes(32 * n)))
    dot = cl.vec_reduce(DOT, 1, 0); cl.wait_result()
    last = _dev(bytes(range(32)))
    for i in reversed(range(m)):
        dr = cl.scalar(tau[i])
        cl.vec_mle_fold(last if i == 0 else 1, 1, dr, 2 << i); cl.wait_result()
        dr.free()
    assert _word(last) == _word(dot) and _word(dot) != 0
    cl.close()
    for d in (point, total, dot, last):
        d.free()


def test_eq_second_turn_of_the_tile_loop(gpu):
    """At most 2048 blocks build an equality table, so m = 22 is the first size at which a block writes a second tile of 1024
    words from the table it built once.  BLS12-381 into n device words: 2048 sampled positions, half of them in the upper half,
    against the product formula, and the SUM of the table is 1."""
    field, m = "BLS381", 22
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    tau = _words(2130, m)
    cl = _client(field, m)
    point, dst = _dev(_pack(tau)), DeviceBuffer(0, 32 * n)
    cl.vec_mle_eq(dst, point); cl.wait_result()
    rng = random.Random(2131)
    for p in [0, n // 2 - 1, n // 2, n - 1] + [rng.randrange(n // 2) for _ in range(1022)] + [rng.randrange(n // 2, n) for _ in range(1022)]:
        v = 1
        for i, t in enumerate(tau):
            v = v * (t if (p >> i) & 1 else 1 - t) % r
        assert bytes(dst.download(32, 32 * p)) == v.to_bytes(32, "little"), p
    total = cl.vec_reduce(SUM, dst); cl.wait_result()
    assert _word(total) == 1
    cl.close()
    for d in (point, dst, total):
        d.free()


def _sumcheck(field, low):
    """A satisfied random R1CS of 2^10 constraints (a witness of 2n words, the upper half chosen so that A z o B z = C z) through
    vec_spmv to A z, B z, C z; eq(tau); then ten rounds of sumcheck for sum_p eq(p) (Az(p) Bz(p) - Cz(p)) = 0: the round polynomial
    as round(eq, Az, Bz; 4) - round(eq, Cz; 4), s(0) + s(1) = claim, a seeded challenge uploaded as a device word, the four
    tables folded in place - Az and Bz in the buffers, Cz and eq in device words -, the next claim s(r) by interpolation."""
    m = 10
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 40 + low)
    z = [rng.randrange(r) for _ in range(n)]
    A, B, Cf = (sparse_rows(rng, r, n, n) for _ in range(3))
    az, bz, cf = (spmv_ref(z, r, n, mat[1], mat[0], mat[2]) for mat in (A, B, Cf))
    z += [(az[p] * bz[p] - cf[p]) % r for p in range(n)]
    rpC, colC, valC = [], [], []
    for p in range(n):   # C = C_free plus the identity on the fresh column
        rpC.append(len(colC))
        colC += Cf[1][Cf[0][p]:Cf[0][p + 1]] + [n + p]
        valC += Cf[2][Cf[0][p]:Cf[0][p + 1]] + [1]
    rpC.append(len(colC))
    cz = [(az[p] * bz[p]) % r for p in range(n)]
    dz = _dev(_pack(z))
    cl = _client(field, m)
    d_cz, d_eq = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    keep = [DeviceBuffer(0, 32 * n) for _ in range(4)]   # the original tables, for the closing check
    arrays = [_dev(b) for b in (_u32(rpC), _u32(colC), _pack(valC), _u32(A[0]), _u32(A[1]), _pack(A[2]), _u32(B[0]), _u32(B[1]), _pack(B[2]))]
    cl.vec_spmv(0, dz, arrays[1], row_ptr=arrays[0], val=arrays[2]); cl.wait_result()
    cl.result_device(0, d_cz)
    cl.vec_spmv(0, dz, arrays[4], row_ptr=arrays[3], val=arrays[5]); cl.wait_result()
    cl.vec_spmv(1, dz, arrays[7], row_ptr=arrays[6], val=arrays[8]); cl.wait_result()
    assert bytes(cl.result(0)) == _pack(az) and bytes(cl.result(1)) == _pack(bz) and bytes(d_cz.download()) == _pack(cz)
    tau = _words(len(field) + 41, m)
    point = _dev(_pack(tau))
    cl.vec_mle_eq(d_eq, point); cl.wait_result()
    cl.result_device(0, keep[0]); cl.result_device(1, keep[1])
    keep[2].upload(bytes(d_cz.download())); keep[3].upload(bytes(d_eq.download()))
    claim, challenges = 0, []
    s1, s2 = DeviceBuffer(0, 128), DeviceBuffer(0, 128)
    for rnd in range(m):
        length = n >> rnd
        cl.vec_mle_round(d_eq, 0, 1, points=4, length=length, low=low, out=s1); cl.wait_result()
        cl.vec_mle_round(d_eq, d_cz, points=4, length=length, low=low, out=s2); cl.wait_result()
        s = [(x - y) % r for x, y in zip(_unpack(s1.download()), _unpack(s2.download()))]
        assert (s[0] + s[1]) % r == claim, (rnd, "s(0) + s(1) = claim")
        c = rng.getrandbits(256)
        challenges.append(c)
        dc = cl.scalar(c)
        for table in (0, 1, d_cz, d_eq):
            cl.vec_mle_fold(table, table, dc, length, low); cl.wait_result()
        dc.free()
        claim = interpolate(s, c, r)
    finals = [_unpack(cl.result(0))[0], _unpack(cl.result(1))[0], _word(d_cz), _word(d_eq)]
    assert claim == finals[3] * (finals[0] * finals[1] - finals[2]) % r
    # each word is the original table at the challenges: DOT(table, eq(challenges)) on the device; the top variable was bound first
    dch = _dev(_pack(challenges if low else challenges[::-1]))
    eqc = DeviceBuffer(0, 32 * n)
    cl.vec_mle_eq(eqc, dch); cl.wait_result()
    for table, final in zip(keep, finals):
        d = cl.vec_reduce(DOT, table, eqc); cl.wait_result()
        assert _word(d) == final
        d.free()
    cl.close()
    for d in arrays + keep + [dz, d_cz, d_eq, point, s1, s2, dch, eqc]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_end_to_end(gpu, field):
    """Both binding orders for BLS12-381, the default (top variable first) for the others."""
    for low in ((False, True) if field == "BLS381" else (False,)):
        _sumcheck(field, low)


def test_protocol_and_refusals(gpu):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 51), _inputs(r, n, 52)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 161))
    out = _dev(mark)          # 5 words
    big = _dev(bytes(64 * n))  # 2n words
    dstw = _dev(bytes(32 * n))
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def ref(v):
        return None if v is None else C.byref(v)

    def fold(flags, d, x, rr, length):
        return L.blz_ntt_vec_mle_fold(cl._h, flags, ref(d), ref(x), ref(rr), length)

    def rnd(flags, x, y, z, points, length, o):
        return L.blz_ntt_vec_mle_round(cl._h, flags, ref(x), ref(y), ref(z), points, length, o)

    def eq(d, p, m):
        return L.blz_ntt_vec_mle_eq(cl._h, ref(d), p, m)

    V = BlzVecArg
    B0, B1, W, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    OUT = V(out.ptr, 0, 0, 4)
    refused = {
        "fold: flag bit 1": (lambda: fold(2, B1, B0, R, n), "unknown multilinear flags"),
        "fold: flag bit 31": (lambda: fold(0x80000001, B1, B0, R, n), "unknown multilinear flags"),
        "fold: null dst": (lambda: fold(0, None, B0, R, n), "takes dst, a and r"),
        "fold: null a": (lambda: fold(0, B1, None, R, n), "takes dst, a and r"),
        "fold: null r": (lambda: fold(0, B1, B0, None, n), "takes dst, a and r"),
        "fold: r names a buffer": (lambda: fold(0, B1, B0, B0, n), "r.d_ptr != NULL, r.count == 1"),
        "fold: r of two words": (lambda: fold(0, B1, B0, V(words.ptr, 0, 0, 2), n), "r.d_ptr != NULL, r.count == 1"),
        "fold: len 0": (lambda: fold(0, B1, B0, R, 0), "len 0: the live length is 2^m with 2 <= len <= 256"),
        "fold: len 1": (lambda: fold(0, B1, B0, R, 1), "len 1: the live length is 2^m"),
        "fold: len 6": (lambda: fold(0, B1, B0, R, 6), "len 6: the live length is 2^m"),
        "fold: len 2n": (lambda: fold(0, B1, B0, R, 2 * n), "len 512: the live length is 2^m with 2 <= len <= 256"),
        "fold: a reserved": (lambda: fold(0, B1, V(None, 0, 7, 0), R, n), "operand a: reserved must be 0"),
        "fold: a buf 2": (lambda: fold(0, B1, V(None, 2, 0, 0), R, n), "operand a: buf must be 0 or 1"),
        "fold: a count 3": (lambda: fold(0, B1, V(words.ptr, 0, 0, 3), R, n), "operand a: count 3 is not a power of two"),
        "fold: a count 2n": (lambda: fold(0, B1, V(big.ptr, 0, 0, 2 * n), R, n), "operand a: count 512 is not a power of two in [1, 256]"),
        "fold: a count of a buffer": (lambda: fold(0, B1, V(None, 0, 0, n // 2), R, n), "operand a: a transform buffer holds"),
        "fold: a in host memory": (lambda: fold(0, B1, V(host_ptr, 0, 0, n), R, n), "operand a: d_ptr is not"),
        "fold: a misaligned": (lambda: fold(0, B1, V(words.ptr + 8, 0, 0, 1), R, n), "operand a: d_ptr is not 16-byte aligned"),
        "fold: a past its allocation": (lambda: fold(0, B1, V(one_word.ptr, 0, 0, 2), R, n), "operand a: 2 elements run past the end"),
        "fold: r in host memory": (lambda: fold(0, B1, B0, V(host_ptr, 0, 0, 1), n), "operand r: d_ptr is not"),
        "fold: dst reserved": (lambda: fold(0, V(None, 1, 1, 0), B0, R, n), "operand dst: reserved must be 0"),
        "fold: dst buf 2": (lambda: fold(0, V(None, 2, 0, 0), B0, R, n), "operand dst: buf must be 0 or 1"),
        "fold: dst count below out_len": (lambda: fold(0, V(out.ptr, 0, 0, 4), B0, R, 16), "operand dst: count 4 is below the 8 words"),
        "fold: dst count 3": (lambda: fold(0, V(out.ptr, 0, 0, 3), B0, R, 4), "operand dst: count 3 is not a power of two"),
        "fold: dst count 0": (lambda: fold(0, V(out.ptr, 0, 0, 0), B0, R, 4), "operand dst: count 0 is not a power of two"),
        "fold: dst count 2n": (lambda: fold(0, V(big.ptr, 0, 0, 2 * n), B0, R, 4), "operand dst: count 512 is not a power of two in [1, 256]"),
        "fold: dst in host memory": (lambda: fold(0, V(host_ptr, 0, 0, n), B0, R, n), "operand dst: d_ptr is not"),
        "fold: dst misaligned": (lambda: fold(0, V(out.ptr + 8, 0, 0, 1), B0, R, 2), "operand dst: d_ptr is not 16-byte aligned"),
        "fold: dst past its allocation": (lambda: fold(0, V(out.ptr, 0, 0, 8), B0, R, 2), "operand dst: 8 elements run past the end"),
        "fold: dst inside the source": (lambda: fold(0, V(words.ptr + 32, 0, 0, 1), W, R, 2), "dst overlaps the words of a"),
        "fold: source inside dst": (lambda: fold(0, V(words.ptr, 0, 0, n), V(words.ptr + 64, 0, 0, 4), R, 8), "dst overlaps the words of a"),
        "fold: in place, periodic": (lambda: fold(0, W, V(words.ptr, 0, 0, 4), R, 8), "periodic source cannot be folded in place"),
        "fold: r in the words written": (lambda: fold(0, W, B0, V(words.ptr + 32, 0, 0, 1), 4), "r lies in the words dst receives"),
        "round: flag bit 1": (lambda: rnd(2, B0, None, None, 2, n, out.ptr), "unknown multilinear flags"),
        "round: null a": (lambda: rnd(0, None, B1, None, 2, n, out.ptr), "a is NULL"),
        "round: c without b": (lambda: rnd(0, B0, None, B1, 2, n, out.ptr), "b is NULL while c is set"),
        "round: points 0": (lambda: rnd(0, B0, None, None, 0, n, out.ptr), "points 0 is not in [1, 4]"),
        "round: points 5": (lambda: rnd(0, B0, None, None, 5, n, out.ptr), "points 5 is not in [1, 4]"),
        "round: len 3": (lambda: rnd(0, B0, None, None, 2, 3, out.ptr), "len 3: the live length is 2^m"),
        "round: len 2n": (lambda: rnd(0, B0, None, None, 2, 2 * n, out.ptr), "len 512: the live length is 2^m"),
        "round: null d_out": (lambda: rnd(0, B0, B1, None, 3, n, None), "null d_out"),
        "round: d_out in host memory": (lambda: rnd(0, B0, B1, None, 3, n, host_ptr), "operand d_out: d_ptr is not"),
        "round: d_out misaligned": (lambda: rnd(0, B0, B1, None, 3, n, out.ptr + 8), "operand d_out: d_ptr is not 16-byte aligned"),
        "round: d_out past its allocation": (lambda: rnd(0, B0, B1, None, 4, n, out.ptr + 64), "operand d_out: 4 elements run past the end"),
        "round: d_out on b's words": (lambda: rnd(0, B0, W, None, 3, n, words.ptr + 32 * (n - 1) - 64), "d_out overlaps the words of a d_ptr operand"),
        "round: d_out's last word on c": (lambda: rnd(0, B0, B1, V(words.ptr + 64, 0, 0, 1), 3, n, words.ptr), "d_out overlaps the words of a d_ptr operand"),
        "round: b reserved": (lambda: rnd(0, B0, V(None, 1, 3, 0), None, 3, n, out.ptr), "operand b: reserved must be 0"),
        "round: c count 3": (lambda: rnd(0, B0, B1, V(words.ptr, 0, 0, 3), 3, n, out.ptr), "operand c: count 3 is not a power of two"),
        "eq: null dst": (lambda: eq(None, one_word.ptr, 1), "takes dst"),
        "eq: m above log n": (lambda: eq(B0, words.ptr, logn + 1), "m 9 is above the handle's log_size 8"),
        "eq: null d_point": (lambda: eq(B0, None, 1), "null d_point"),
        "eq: d_point in host memory": (lambda: eq(B0, host_ptr, 2), "d_point is not"),
        "eq: d_point misaligned": (lambda: eq(B0, words.ptr + 8, 2), "d_point is not 16-byte aligned"),
        "eq: d_point past its allocation": (lambda: eq(B0, one_word.ptr, 2), "2 elements run past the end of the allocation d_point"),
        "eq: d_point in the words written": (lambda: eq(W, words.ptr + 64, 2), "d_point lies in the words dst receives"),
        "eq: dst count below 2^m": (lambda: eq(OUT, words.ptr, 3), "operand dst: count 4 is below the 8 words"),
        "eq: dst count 3": (lambda: eq(V(out.ptr, 0, 0, 3), words.ptr, 1), "operand dst: count 3 is not a power of two"),
        "eq: dst buf 2": (lambda: eq(V(None, 2, 0, 0), words.ptr, 1), "operand dst: buf must be 0 or 1"),
    }
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and _word(one_word) == 7 and bytes(out.download()) == mark
    # a fold in flight, buffer 0 -> buffer 1: the source can be read, the destination cannot, nothing else starts
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.vec_mle_round(0), lambda: cl.vec_mle_eq(1, one_word))
    cl.vec_mle_fold(1, 0, one_word)
    assert bytes(cl.result(0)) == ab
    for attempt in busy + (lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab))):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    assert bytes(cl.result(1)) == _pack(fold_ref(a, r, 7, n, False)) + bb[16 * n:] and bytes(cl.result(0)) == ab
    cl.set_data(NTTInput(1, bb))
    # a round in flight over buffer 0 and device words, and an equality table into device words: no buffer is written - both can
    # be read, buffer 1 (not named) can be written, buffer 0 (read) cannot
    for start in (lambda: cl.vec_mle_round(0, words), lambda: cl.vec_mle_fold(dstw, 0, one_word)):
        res = start()
        assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
        cl.set_data(NTTInput(1, bb))
        with pytest.raises(DriverClientError) as ei:
            cl.set_data(NTTInput(0, ab))
        assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
        for attempt in busy:
            with pytest.raises(DriverClientError):
                attempt()
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        if res is not None:
            assert bytes(res.download()) == _pack(round_ref([a, b], r, n, 3, False))
            res.free()
    assert bytes(dstw.download()) == _pack(fold_ref(a, r, 7, n, False)) + bytes(16 * n)
    cl.vec_mle_eq(dstw, words, 3)
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(0, ab))   # it names no buffer
    cl.wait_result()
    assert bytes(dstw.download()) == _pack(eq_ref(b[:3], r)) + _pack(fold_ref(a, r, 7, n, False))[256:] + bytes(16 * n)   # 8 words, not one more
    # reset with an op in flight: nothing is in flight afterwards, and the handle works
    for start in (lambda: cl.vec_mle_fold(1, 0, one_word, low=True), lambda: cl.vec_mle_round(0, 1, 1), lambda: cl.vec_mle_eq(1, words, logn)):
        start()
        cl.reset()
        with pytest.raises(DriverClientError):
            cl.wait_result()
    cl.set_data(NTTInput(1, bb))
    cl.vec_mle_fold(1, 1, one_word, low=True)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(fold_ref(b, r, 7, n, True)) + bb[16 * n:] and bytes(cl.result(0)) == ab
    cl.close()
    for d in (words, one_word, out, big, dstw):
        d.free()
