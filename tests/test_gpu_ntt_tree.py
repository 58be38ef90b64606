"""Product and fraction trees on resident buffers (blz_ntt_mle_tree) on the device: every layer of both trees under both
pairings against Python integers, the shapes of sources and destinations, the grid-stride loop's second sweep against the
per-layer sequence of existing ops, the order of checks with every refusal, and what the op is for - a GKR grand product
verified layer by layer.  Every comparison is byte for byte: any 256-bit input word counts as its residue, every word written
is canonical, exactly len - 1 words of a destination are written and no other byte - of a destination, of a source, of the other
buffer - changes."""
import ctypes as C

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_mle_util import check_order_of_checks, fill, interpolate
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, _client, _dev, _pack, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
PROD, FRAC = NTTClient.TREE_PROD, NTTClient.TREE_FRAC
# log len: k_tree_top alone up to 10; above it ceil((m - 10) / J) launches of k_tree_up, J = 3 (PROD) and 2 (FRAC): 11 .. 14 pass
# every residue of (m - 10) mod J for both, and 14 takes two launches of either
LOGS = {"BLS381": list(range(1, 15)), "BLS377": [1, 7, 10, 13], "BN254": [1, 7, 10, 13]}
CASES = [(f, m) for f in FIELDS for m in LOGS[f]]
COMBOS = [(op, low) for op in (PROD, FRAC) for low in (False, True)]


def tree_ref(op, r, length, low, a, a_q=None):
    """Layers 1 .. m on Python integers: [(P layer, Q layer or None)], the sources read periodically"""
    p = [a[i % len(a)] % r for i in range(length)]
    q = None if op == PROD else [a_q[i % len(a_q)] % r for i in range(length)]
    layers = []
    while len(p) > 1:
        half = len(p) // 2
        idx = [(2 * i, 2 * i + 1) for i in range(half)] if low else [(i, i + half) for i in range(half)]
        if op == PROD:
            p = [p[lo] * p[hi] % r for lo, hi in idx]
        else:
            p, q = [(p[lo] * q[hi] + p[hi] * q[lo]) % r for lo, hi in idx], [q[lo] * q[hi] % r for lo, hi in idx]
        layers.append((p, q))
    return layers


def tree_bytes(layers, which=0):
    """The len - 1 words a destination receives: layer 1 first, the root last"""
    return b"".join(_pack(layer[which]) for layer in layers)


_REFS = {}


def _reference(field, m):
    """The sources of (field, m) and the expected destination bytes of every combination, computed once"""
    if (field, m) not in _REFS:
        r = pyref.CURVES[field]["r"]
        n = 1 << m
        a, a_q = _inputs(r, n, 31000 + 10 * m + len(field)), _inputs(r, n, 32000 + 10 * m + len(field))[::-1]   # Q: the edge words last
        want = {}
        for op, low in COMBOS:
            layers = tree_ref(op, r, n, low, a, a_q)
            want[op, low] = (tree_bytes(layers), tree_bytes(layers, 1) if op == FRAC else None)
        _REFS[field, m] = (_pack(a), _pack(a_q), want)
    return _REFS[field, m]


def _bytes_of(cl, t):
    return bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))


@pytest.mark.parametrize("field,m", CASES)
def test_every_layer_against_python_integers(gpu, field, m):
    """Both ops, both pairings, device words to device words.  The destinations hold random bytes first: words [0, len - 1)
    become the layers, word len - 1 keeps its bytes, the sources keep theirs."""
    n = 1 << m
    ab, qb, want = _reference(field, m)
    cl = _client(field, m)
    a, a_q = _dev(ab), _dev(qb)
    dst, dst_q = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    for turn, (op, low) in enumerate(COMBOS):
        fp, fq = fill(n, 7 * m + turn), fill(n, 7 * m + turn + 100)
        dst.upload(fp)
        dst_q.upload(fq)
        if op == PROD:
            cl.mle_tree(dst, a, low=low)
        else:
            cl.mle_tree(dst, a, FRAC, low=low, dst_q=dst_q, a_q=a_q)
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        wp, wq = want[op, low]
        assert len(wp) == 32 * (n - 1)
        assert bytes(dst.download()) == wp + fp[32 * (n - 1):], (op, low, "dst")
        assert bytes(dst_q.download()) == (fq if op == PROD else wq + fq[32 * (n - 1):]), (op, low, "dst_q")
        assert bytes(a.download()) == ab and bytes(a_q.download()) == qb, (op, low, "a source changed")
    cl.close()
    for d in (a, a_q, dst, dst_q):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_shapes_of_sources_and_destinations(gpu, field):
    """At len = n = 2^11 (one launch of k_tree_up, then k_tree_top): buffer to the other buffer, words to a buffer, a buffer to
    words, FRAC into both transform buffers from device words, periodic sources of one and of four words, FRAC with a one-word
    numerator; and len = n / 4 on a buffer, with the words behind len - 1 kept."""
    m = 11
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    ab, qb, want = _reference(field, m)
    av, qv = _unpack(ab), _unpack(qb)
    cl = _client(field, m)
    a, a_q, out = _dev(ab), _dev(qb), DeviceBuffer(0, 32 * n)
    f0, f1 = fill(n, 501), fill(n, 502)
    tail0, tail1 = f0[32 * (n - 1):], f1[32 * (n - 1):]
    # buffer -> the other buffer, both pairings
    for low in (False, True):
        cl.set_data(NTTInput(0, ab))
        cl.set_data(NTTInput(1, f1))
        cl.mle_tree(1, 0, low=low)
        cl.wait_result()
        assert bytes(cl.result(1)) == want[PROD, low][0] + tail1 and bytes(cl.result(0)) == ab
    # words -> buffer
    cl.set_data(NTTInput(0, f0))
    cl.set_data(NTTInput(1, f1))
    cl.mle_tree(0, a)
    cl.wait_result()
    assert bytes(cl.result(0)) == want[PROD, False][0] + tail0 and bytes(cl.result(1)) == f1 and bytes(a.download()) == ab
    # buffer -> words
    cl.set_data(NTTInput(1, ab))
    out.upload(f0)
    cl.mle_tree(out, 1, low=True)
    cl.wait_result()
    assert bytes(out.download()) == want[PROD, True][0] + tail0 and bytes(cl.result(1)) == ab
    # FRAC into both transform buffers from device words; and the denominators into buffer 0
    for bp, bq in ((0, 1), (1, 0)):
        fills = {bp: f0, bq: f1}
        cl.set_data(NTTInput(bp, f0))
        cl.set_data(NTTInput(bq, f1))
        cl.mle_tree(bp, a, FRAC, dst_q=bq, a_q=a_q)
        cl.wait_result()
        assert bytes(cl.result(bp)) == want[FRAC, False][0] + fills[bp][32 * (n - 1):]
        assert bytes(cl.result(bq)) == want[FRAC, False][1] + fills[bq][32 * (n - 1):]
    assert bytes(a.download()) == ab and bytes(a_q.download()) == qb
    # FRAC from a buffer and words into words and a buffer
    cl.set_data(NTTInput(0, qb))
    cl.set_data(NTTInput(1, f1))
    out.upload(f0)
    cl.mle_tree(out, a, FRAC, low=True, dst_q=1, a_q=0)
    cl.wait_result()
    assert bytes(out.download()) == want[FRAC, True][0] + tail0 and bytes(cl.result(1)) == want[FRAC, True][1] + tail1 and bytes(cl.result(0)) == qb
    # periodic sources: one word and four words (the edge words r - 1, r, r + 1, 2^256 - 1 among them)
    for count, low in ((1, False), (4, False), (4, True)):
        src = av[2: 2 + count]
        per = _dev(_pack(src))
        out.upload(f0)
        cl.mle_tree(out, per, length=n, low=low)
        cl.wait_result()
        assert bytes(out.download()) == tree_bytes(tree_ref(PROD, r, n, low, src)) + tail0, (count, low)
        assert bytes(per.download()) == _pack(src)
        per.free()
    # sum 1 / Q: the one-word numerator 1; and a four-word numerator over a four-word denominator
    one = cl.scalar(1)
    for num, den in (([1], qv), (av[1:5], qv[-4:])):
        pn = one if num == [1] else _dev(_pack(num))
        pd = a_q if den is qv else _dev(_pack(den))
        cl.set_data(NTTInput(0, f0))
        out.upload(f1)
        cl.mle_tree(0, pn, FRAC, length=n, dst_q=out, a_q=pd)
        cl.wait_result()
        layers = tree_ref(FRAC, r, n, False, num, den)
        assert bytes(cl.result(0)) == tree_bytes(layers) + tail0 and bytes(out.download()) == tree_bytes(layers, 1) + tail1
    assert _word(one) == 1
    # len < n on a buffer: n / 4 words of the source, n / 4 - 1 words written
    length = n // 4
    for op, low in COMBOS:
        cl.set_data(NTTInput(0, ab))
        cl.set_data(NTTInput(1, f1))
        out.upload(f0)
        if op == PROD:
            cl.mle_tree(1, 0, length=length, low=low)
        else:
            cl.mle_tree(1, 0, FRAC, length=length, low=low, dst_q=out, a_q=a_q)
        cl.wait_result()
        layers = tree_ref(op, r, length, low, av[:length], qv[:length])
        assert bytes(cl.result(1)) == tree_bytes(layers) + f1[32 * (length - 1):], (op, low)
        assert bytes(out.download()) == (f0 if op == PROD else tree_bytes(layers, 1) + f0[32 * (length - 1):]), (op, low)
        assert bytes(cl.result(0)) == ab
    cl.close()
    for d in (a, a_q, out, one):
        d.free()


def _eq_product(tau, r, m):
    """prod over p < 2^m of eq(tau, p): every variable contributes tau_i (1 - tau_i) once per pair"""
    out = 1
    for t in tau:
        out = out * pow(t * (1 - t) % r, 1 << (m - 1), r) % r
    return out


def _layer_views(buf, length, k):
    """layer k of a destination of mle_tree as (lo half, hi half, whole) views; k == 0: of the source itself"""
    off, words = (0, length) if k == 0 else NTTClient.tree_layer(length, k)
    whole = buf.view(32 * off, 32 * words)
    if words == 1:
        return whole, whole, whole
    return buf.view(32 * off, 16 * words), buf.view(32 * off + 16 * words, 16 * words), whole


def test_second_sweep_product_tree_against_the_per_layer_sequence(gpu):
    """BLS12-381, PROD with the default pairing at len = 2^23: the first launch of k_tree_up has 2^23 / 2^3 = 2^20 nodes for
    2048 x 256 = 2^19 lanes - the smallest length at which its grid-stride loop takes a second sweep.  The source is an equality
    table, written by the device: no two runs of it repeat, and its product has a closed form.  Every layer equals what one
    blz_ntt_gate_eval per layer writes from views of the layer below, byte for byte; the root equals Python's product."""
    field, m = "BLS381", 23
    assert (1 << m) >> 3 == 2 * 2048 * 256
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    tau = [v % r for v in _words(2301, m)]
    cl = _client(field, m)
    point = _dev(_pack(tau))
    src, tree, seq = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    cl.vec_mle_eq(src, point)
    cl.wait_result()
    tail = fill(1, 2302)
    for d in (tree, seq):
        d.view(32 * (n - 1), 32).upload(tail)
    cl.mle_tree(tree, src)
    cl.wait_result()
    below = src
    for k in range(1, m + 1):
        lo, hi, _ = _layer_views(below, n, k - 1)
        _, _, dst = _layer_views(seq, n, k)
        cl.gate_eval(dst, [lo, hi], [(1, [0, 1])], length=n >> k)
        cl.wait_result()
        below = seq
    got = bytes(tree.download())
    assert got == bytes(seq.download())
    assert got[32 * (n - 1):] == tail
    assert int.from_bytes(got[32 * (n - 2): 32 * (n - 1)], "little") == _eq_product(tau, r, m)
    cl.close()
    for d in (point, src, tree, seq):
        d.free()


def test_second_sweep_fraction_tree_low_against_the_per_layer_sequence(gpu):
    """BLS12-381, FRAC with BLZ_MLE_LOW at len = 2^22: 2^22 / 2^2 = 2^20 nodes in the first launch, two sweeps (J = 2).
    Numerators eq(tau, .), denominators eq(sigma, .).  The sequence: per layer the even and the odd words of P and Q gathered
    (blz_ntt_vec_gather, stride 2) and copied out of the transform buffer, then one blz_ntt_gate_eval each for P' and Q'.  The
    root is sum_p P[p] / Q[p] = prod_i ((1 - tau_i) / (1 - sigma_i) + tau_i / sigma_i) over the product of the denominators."""
    field, m = "BLS381", 22
    assert (1 << m) >> 2 == 2 * 2048 * 256
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    tau, sigma = [v % r for v in _words(2201, m)], [v % r for v in _words(2202, m)]
    cl = _client(field, m)
    pt, ps = _dev(_pack(tau)), _dev(_pack(sigma))
    srcs = [DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)]
    trees = [DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)]
    seqs = [DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)]
    parts = [DeviceBuffer(0, 16 * n) for _ in range(4)]   # P even, P odd, Q even, Q odd
    for d, p in zip(srcs, (pt, ps)):
        cl.vec_mle_eq(d, p)
        cl.wait_result()
    tail = fill(1, 2203)
    for d in trees + seqs:
        d.view(32 * (n - 1), 32).upload(tail)
    cl.mle_tree(trees[0], srcs[0], FRAC, low=True, dst_q=trees[1], a_q=srcs[1])
    cl.wait_result()
    below = srcs
    for k in range(1, m + 1):
        half = n >> k
        for t in (0, 1):
            layer = _layer_views(below[t], n, k - 1)[2]
            for odd in (0, 1):
                cl.vec_gather(0, layer, offset=odd, stride=2, length=half)
                cl.wait_result()
                cl.gate_eval(parts[2 * t + odd], [0], [(1, [0])], length=half)
                cl.wait_result()
        cl.gate_eval(_layer_views(seqs[0], n, k)[2], parts, [(1, [0, 3]), (1, [1, 2])], length=half)
        cl.wait_result()
        cl.gate_eval(_layer_views(seqs[1], n, k)[2], parts[2:], [(1, [0, 1])], length=half)
        cl.wait_result()
        below = seqs
    got = [bytes(d.download()) for d in trees]
    for t in (0, 1):
        assert got[t] == bytes(seqs[t].download()), t
        assert got[t][32 * (n - 1):] == tail
    root_p, root_q = (int.from_bytes(g[32 * (n - 2): 32 * (n - 1)], "little") for g in got)
    total = 1
    for t, s in zip(tau, sigma):
        total = total * ((1 - t) * pow(1 - s, -1, r) + t * pow(s, -1, r)) % r
    assert root_q == _eq_product(sigma, r, m)
    assert root_p == total * root_q % r
    cl.close()
    for d in [pt, ps] + srcs + trees + seqs + parts:
        d.free()


def raw_tree(cl, op, flags, dst, dst_q, a, a_q, length):
    """The C entry point itself: operands ints (buffers) / DeviceBuffers / BlzVecArgs / None"""
    args = [x if isinstance(x, BlzVecArg) or x is None else cl._vec_arg(x) for x in (dst, dst_q, a, a_q)]
    return blaze_amd.lib().blz_ntt_mle_tree(cl._h, op, flags, *[None if v is None else C.byref(v) for v in args], length)


def test_order_of_checks_and_every_refusal(gpu):
    """The checks run in the documented order - op, flags, the operands an op takes, len, an op in flight, the sources' operand
    errors, then per destination its operand errors, its count and its overlaps with the sources, last the two destinations'
    overlap: a call wrong in two ways reports the earlier check, the later fault alone its own.  Nothing is enqueued by a refusal,
    made while an op is in flight or not, and a good call runs behind each."""
    field, m = "BLS381", 8
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    ab, qb = _pack(_inputs(r, n, 81)), _pack(_inputs(r, n, 82))
    cl = _client(field, m)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, qb))
    a, a_q, d, d_q = _dev(ab), _dev(qb), _dev(fill(n, 83)), _dev(fill(n, 84))
    big = _dev(bytes(64 * n))
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    A, AQ, D, DQ = (V(x.ptr, 0, 0, n) for x in (a, a_q, d, d_q))
    B0, B1 = V(None, 0, 0, 0), V(None, 1, 0, n)
    small_src = _inputs(r, 8, 85)
    small = _dev(_pack(small_src))
    small_out = DeviceBuffer(0, 32 * 8)
    small_want = tree_bytes(tree_ref(PROD, r, 8, False, small_src))

    def t(op, flags, dst, dst_q, x, x_q, length):
        return lambda: raw_tree(cl, op, flags, dst, dst_q, x, x_q, length)

    def flight():
        cl.vec_op(NTTClient.MUL, 1, 1, a)

    def good():
        small_out.upload(fill(8, 86))
        cl.mle_tree(small_out, small)
        cl.wait_result()
        assert bytes(small_out.download()) == small_want + fill(8, 86)[32 * 7:]

    assert L.blz_ntt_mle_tree(None, 9, 9, None, None, None, None, 3) == 4 and b"null handle" in L.blz_last_error_message()
    OP, FL, LEN, BUSY = "unknown tree op 2", "unknown multilinear flags 0x2", "len 3: the live length is 2^m with 2 <= len <= 256", "already running"
    TAKES_P, TAKES_F = "a product tree takes dst and a, and dst_q and a_q must be NULL", "a fraction tree takes dst, dst_q, a and a_q"
    OVER_A, OVER_AQ = "dst overlaps the words read of a:", "dst overlaps the words read of a_q:"
    Q_OVER_A, Q_OVER_AQ, BOTH = "dst_q overlaps the words read of a:", "dst_q overlaps the words read of a_q:", "dst and dst_q overlap in the words they receive"
    cases = [
        ("op before flags", (t(2, 2, D, None, A, None, n), OP, False), (t(PROD, 2, D, None, A, None, n), FL, False)),
        ("op 0xFFFFFFFF before the operands", (t(0xFFFFFFFF, 0, None, None, None, None, n), "unknown tree op 4294967295", False), (t(PROD, 0, None, None, None, None, n), TAKES_P, False)),
        ("flags before the operands", (t(PROD, 0x80000000, D, None, None, None, n), "unknown multilinear flags 0x80000000", False), (t(PROD, 0, D, None, None, None, n), TAKES_P, False)),
        ("PROD with a_q, before len", (t(PROD, 0, D, None, A, AQ, 3), TAKES_P, False), (t(PROD, 0, D, None, A, None, 3), LEN, False)),
        ("PROD with dst_q, before len", (t(PROD, 1, D, DQ, A, None, 0), TAKES_P, False), (t(PROD, 1, D, None, A, None, 0), "len 0: the live length", False)),
        ("PROD without dst", (t(PROD, 0, None, None, A, None, 1), TAKES_P, False), (t(PROD, 0, D, None, A, None, 1), "len 1: the live length", False)),
        ("FRAC without dst_q, before len", (t(FRAC, 0, D, None, A, AQ, 3), TAKES_F, False), (t(FRAC, 0, D, DQ, A, AQ, 3), LEN, False)),
        ("FRAC without a_q", (t(FRAC, 1, D, DQ, A, None, 2 * n), TAKES_F, False), (t(FRAC, 1, D, DQ, A, AQ, 2 * n), "len 512: the live length", False)),
        ("FRAC without a", (t(FRAC, 0, D, DQ, None, AQ, n), TAKES_F, False), (t(FRAC, 0, None, DQ, A, AQ, n), TAKES_F, False)),
        ("len before an op in flight", (t(PROD, 0, D, None, A, None, 3), LEN, True), (t(PROD, 0, D, None, A, None, n), BUSY, True)),
        ("the operands an op takes, in flight", (t(FRAC, 0, D, None, A, None, n), TAKES_F, True), (t(FRAC, 0, D, DQ, A, AQ, n), BUSY, True)),
        ("in flight before a source's errors", (t(PROD, 0, D, None, V(a.ptr + 8, 0, 0, 8), None, 8), BUSY, True),
         (t(PROD, 0, D, None, V(a.ptr + 8, 0, 0, 8), None, 8), "operand a: d_ptr is not 16-byte aligned", False)),
        ("a before a_q", (t(FRAC, 0, D, DQ, V(None, 0, 7, 0), V(None, 2, 0, 0), n), "operand a: reserved must be 0", False),
         (t(FRAC, 0, D, DQ, A, V(None, 2, 0, 0), n), "operand a_q: buf must be 0 or 1", False)),
        ("a source before dst", (t(FRAC, 0, V(d.ptr + 8, 0, 0, n), DQ, A, V(a_q.ptr, 0, 0, 3), n), "operand a_q: count 3 is not a power of two", False),
         (t(FRAC, 0, V(d.ptr + 8, 0, 0, n), DQ, A, AQ, n), "operand dst: d_ptr is not 16-byte aligned", False)),
        ("a in host memory", (t(PROD, 0, V(None, 2, 0, 0), None, V(host_ptr, 0, 0, n), None, n), "operand a: d_ptr is not", False),
         (t(PROD, 0, V(None, 2, 0, 0), None, A, None, n), "operand dst: buf must be 0 or 1", False)),
        ("a count 2n", (t(PROD, 0, V(host_ptr, 0, 0, n), None, V(big.ptr, 0, 0, 2 * n), None, n), "operand a: count 512 is not a power of two in [1, 256]", False),
         (t(PROD, 0, V(host_ptr, 0, 0, n), None, A, None, n), "operand dst: d_ptr is not", False)),
        ("a buffer's count", (t(PROD, 0, V(big.ptr, 0, 0, 2 * n), None, V(None, 1, 0, 8), None, n), "operand a: a transform buffer holds 256 elements, count says 8", False),
         (t(PROD, 0, V(big.ptr, 0, 0, 2 * n), None, A, None, n), "operand dst: count 512 is not a power of two in [1, 256]", False)),
        ("a_q past its allocation", (t(FRAC, 0, V(d.ptr, 0, 1, n), DQ, A, V(a_q.ptr + 32 * (n - 1), 0, 0, 2), n), "operand a_q: 2 elements run past the end", False),
         (t(FRAC, 0, V(d.ptr, 0, 1, n), DQ, A, AQ, n), "operand dst: reserved must be 0", False)),
        ("dst's count before its overlap", (t(PROD, 0, V(a.ptr, 0, 0, n // 2), None, A, None, n), "operand dst: count 128 is below the 255 words the op writes", False),
         (t(PROD, 0, A, None, A, None, n), OVER_A, False)),
        ("dst past its allocation", (t(PROD, 0, V(a.ptr + 32 * (n - 4), 0, 0, 8), None, A, None, 8), "operand dst: 8 elements run past the end", False),
         (t(PROD, 0, V(a.ptr + 32 * 7, 0, 0, 8), None, A, None, 8), OVER_A, False)),
        ("dst on a before dst on a_q", (t(FRAC, 0, B0, DQ, B0, B0, n), OVER_A, False), (t(FRAC, 0, B0, DQ, A, B0, n), OVER_AQ, False)),
        # len 2 reads two words of a source and writes one: a destination on word 1 meets it, one on word n - 1 does not
        ("dst's overlap before dst_q's errors", (t(FRAC, 0, V(a_q.ptr + 32, 0, 0, 1), V(d_q.ptr, 0, 1, n), A, AQ, 2), OVER_AQ, False),
         (t(FRAC, 0, V(a_q.ptr + 32 * (n - 1), 0, 0, 1), V(d_q.ptr, 0, 1, n), A, AQ, 2), "operand dst_q: reserved must be 0", False)),
        ("dst's overlap with a periodic source's one word", (t(FRAC, 0, V(a.ptr, 0, 0, n), V(None, 2, 0, 0), V(a.ptr + 32 * 3, 0, 0, 1), AQ, n), OVER_A, False),
         (t(FRAC, 0, D, V(None, 2, 0, 0), V(a.ptr + 32 * 3, 0, 0, 1), AQ, n), "operand dst_q: buf must be 0 or 1", False)),
        ("dst_q's count before its overlap", (t(FRAC, 0, D, V(a.ptr, 0, 0, 4), A, AQ, 8), "operand dst_q: count 4 is below the 7 words the op writes", False),
         (t(FRAC, 0, D, V(a.ptr, 0, 0, 8), A, AQ, 8), Q_OVER_A, False)),
        ("a destination on a source before the two destinations", (t(FRAC, 0, B1, B1, A, B1, n), OVER_AQ, False), (t(FRAC, 0, B1, B1, A, AQ, n), BOTH, False)),
        ("dst on a one-word a_q before the two destinations", (t(FRAC, 0, D, V(d.ptr, 0, 0, n), A, V(d.ptr + 32 * 6, 0, 0, 1), 8), OVER_AQ, False),
         (t(FRAC, 0, D, V(d.ptr + 32 * 6, 0, 0, 8), A, AQ, 8), BOTH, False)),
        # dst words 0 .. 6, dst_q words 4 .. 10 of d, a_q the one word 10
        ("dst_q on a_q before the two destinations", (t(FRAC, 0, V(d.ptr, 0, 0, 8), V(d.ptr + 32 * 4, 0, 0, 8), A, V(d.ptr + 32 * 10, 0, 0, 1), 8), Q_OVER_AQ, False),
         (t(FRAC, 0, V(d.ptr, 0, 0, 8), V(d.ptr + 32 * 4, 0, 0, 8), A, AQ, 8), BOTH, False)),
        ("dst_q is a_q", (t(FRAC, 1, D, AQ, A, AQ, n), Q_OVER_AQ, False), (t(FRAC, 1, D, B1, A, B1, n), Q_OVER_AQ, False)),
        ("an op in flight before the overlaps", (t(FRAC, 0, D, V(d.ptr + 32 * 6, 0, 0, 8), A, AQ, 8), BUSY, True), (t(PROD, 1, B0, None, B0, None, n), OVER_A, False)),
    ]
    check_order_of_checks(cl, cases, flight, good)
    # word len - 1 of dst is not written: dst_q may start there
    d.upload(fill(n, 83))
    assert raw_tree(cl, FRAC, 0, V(d.ptr, 0, 0, 8), V(d.ptr + 32 * 7, 0, 0, 8), small, small, 8) == 0
    cl.wait_result()
    layers = tree_ref(FRAC, r, 8, False, small_src, small_src)
    assert bytes(d.download()) == tree_bytes(layers) + tree_bytes(layers, 1) + fill(n, 83)[32 * 14:]
    # the refusals changed nothing
    assert bytes(a.download()) == ab and bytes(a_q.download()) == qb and bytes(d_q.download()) == fill(n, 84) and bytes(big.download()) == bytes(64 * n)
    assert bytes(cl.result(0)) == ab
    # the Python client: the library refuses, the client's own checks raise
    with pytest.raises(blaze_amd.DriverClientError) as ei:
        cl.mle_tree(d, a, FRAC)
    assert ei.value.variant == "InvalidPrimitiveParam"
    cl.close()
    for x in (a, a_q, d, d_q, big, small, small_out):
        x.free()


def test_in_flight_rules_with_two_written_buffers(gpu):
    """FRAC into both transform buffers: neither can be read or written until wait_result; a PROD tree into one buffer from the
    other leaves the source readable."""
    field, m = "BLS381", 8
    n = 1 << m
    ab, qb, want = _reference(field, m)
    cl = _client(field, m)
    a, a_q = _dev(ab), _dev(qb)
    cl.mle_tree(0, a, FRAC, dst_q=1, a_q=a_q)
    for attempt in (lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
                    lambda: cl.mle_tree(0, a), lambda: cl.start_process(0)):
        with pytest.raises(blaze_amd.DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert bytes(cl.result(0))[: 32 * (n - 1)] == want[FRAC, False][0] and bytes(cl.result(1))[: 32 * (n - 1)] == want[FRAC, False][1]
    cl.set_data(NTTInput(1, ab))
    cl.mle_tree(0, 1, low=True)
    assert bytes(cl.result(1)) == ab   # only read: readable
    with pytest.raises(blaze_amd.DriverClientError):
        cl.result(0)
    with pytest.raises(blaze_amd.DriverClientError):
        cl.set_data(NTTInput(1, ab))
    cl.wait_result()
    assert bytes(cl.result(0))[: 32 * (n - 1)] == want[PROD, True][0]
    cl.close()
    a.free()
    a_q.free()


def _eq_at(tau, p, r):
    out = 1
    for i, t in enumerate(tau):
        out = out * (t if (p >> i) & 1 else 1 - t) % r
    return out


def test_gkr_grand_product_layer_by_layer(gpu):
    """What the op is for: a GKR grand product over 2^6 leaves, BLS12-381.  mle_tree writes every layer; from the root down,
    layer k's claim V_k(tau) = sum_p eq(tau, p) lo[p] hi[p] - lo and hi the two halves of layer k - 1, views of the tree's memory
    taken as tables unchanged - is proven by a sumcheck on the device (vec_mle_eq, sumcheck_gate first without r, then with) and
    checked by a verifier on Python integers: s(0) + s(1) against the claim every round, the final eq lo hi, and the next claim
    lo + rho (hi - lo) down to the leaves' multilinear extension."""
    field, m = "BLS381", 6
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    leaves = [v % r for v in _words(6001, n)]
    cl = _client(field, m)
    src, tree, eq = _dev(_pack(leaves)), DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    cl.mle_tree(tree, src)
    cl.wait_result()
    layers = tree_ref(PROD, r, n, False, leaves)
    assert bytes(tree.download())[: 32 * (n - 1)] == tree_bytes(layers)
    rnd = iter(v % r for v in _words(6002, 64))
    root = _word(tree.view(32 * (n - 2), 32))
    prod = 1
    for v in leaves:
        prod = prod * v % r
    assert root == prod
    claim, tau = root, []
    terms = [(1, [1, 2])]
    for k in range(m, 0, -1):
        nv = m - k   # variables of layer k; lo and hi hold 2^nv words each
        below = src if k == 1 else tree
        lo, hi, _ = _layer_views(below, n, k - 1)
        if nv == 0:   # the root's own pair: no variable, no sumcheck
            lo_f, hi_f = _word(lo), _word(hi)
            assert lo_f * hi_f % r == claim
            z = []
        else:
            point = _dev(_pack(tau))
            cl.vec_mle_eq(eq, point, nv)
            cl.wait_result()
            point.free()
            tabs, length, z = [eq, lo, hi], 1 << nv, []
            out = cl.sumcheck_gate(tabs, terms, common=0, points=4, length=length)
            cl.wait_result()
            s = _unpack(out.download())
            while True:
                assert (s[0] + s[1]) % r == claim, (k, length)
                x = next(rnd)
                z.append(x)
                claim = interpolate(s, x, r)
                rb = cl.scalar(x)
                if length == 2:
                    cl.sumcheck_gate(tabs, terms, common=0, r=rb, points=0, length=length)
                    cl.wait_result()
                    break
                out = cl.sumcheck_gate(tabs, terms, common=0, r=rb, points=4, length=length)
                cl.wait_result()
                s = _unpack(out.download())
                length //= 2
            z = z[::-1]   # the steps bind the top variable first
            eq_f, lo_f, hi_f = _word(eq), _word(lo), _word(hi)
            want_eq = 1
            for t, x in zip(tau, z):
                want_eq = want_eq * (t * x + (1 - t) * (1 - x)) % r
            assert eq_f == want_eq
            assert eq_f * lo_f % r * hi_f % r == claim, k
        rho = next(rnd)
        claim = (lo_f + rho * (hi_f - lo_f)) % r
        tau = z + [rho]
    assert len(tau) == m
    assert claim == sum(_eq_at(tau, p, r) * leaves[p] for p in range(n)) % r
    cl.close()
    for d in (src, tree, eq):
        d.free()
