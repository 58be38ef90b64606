"""Gate evaluation on resident buffers (blz_ntt_gate_eval) on the device: a gate given as data evaluated at every position, with
periodic tables, rotations and in place; agreement with the existing ops where they overlap; the refusals and the in-flight
rules.  Every expected value is Python integer arithmetic (tests/ntt_gate_util.py: gate_value over gate_inputs) or, at 2^20, an
existing op, and every comparison is byte for byte: any 256-bit input word counts as its residue, every word written is
canonical, exactly len words of dst are written and no other byte - of dst, of a table, of the other buffer - changes."""
import ctypes as C
import itertools
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_gate_util import CATALOGUE, gate_inputs, gate_value, make_gate
from ntt_mle_util import fill
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
# (log n, len): below a wave, a single word, a ragged tail inside a wave's reach, one block, a ragged tail over several blocks,
# several full blocks
SIZES = [(1, 2), (2, 1), (6, 64), (10, 1024), (10, 777), (11, 2048)]
# the quotient numerator qL a + qR b + qM a b - qO c + qC over [qL, qR, qM, qO, qC, a, b, c]
PLONK = [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (-1, [3, 7]), (1, [4])]
M64 = (1 << 64) - 1


def _bytes_of(cl, t):
    return bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))


def _ref(vals, terms, common, r, length, rot=None):
    """dst[p], p < length: table i read at (p + rot[i]) mod 2^64 mod its count"""
    rot = rot or [0] * len(vals)
    return [gate_value([v[((p + k) & M64) % len(v)] for v, k in zip(vals, rot)], terms, common, r) for p in range(length)]


def raw_eval(cl, gate, dst, tables, rot, length):
    """The C entry point itself: gate a BlzSumGate (or None), dst / tables ints (buffers) / DeviceBuffers / BlzVecArgs (or None),
    rot a list of ints or None"""
    def arg(x):
        return x if isinstance(x, BlzVecArg) else cl._vec_arg(x)
    arr = None if tables is None else (BlzVecArg * max(len(tables), 1))(*[arg(x) for x in tables])
    vd = None if dst is None else arg(dst)
    rots = None if rot is None else (C.c_uint64 * max(len(rot), 1))(*[k & M64 for k in rot])
    return blaze_amd.lib().blz_ntt_gate_eval(cl._h, None if gate is None else C.byref(gate), None if vd is None else C.byref(vd), arr, rots, length)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_catalogue_against_python_integers(gpu, field, logn, length):
    """Every catalogue gate.  Two of the tables sit in the transform buffers - which two moves with the gate -, the rest in device
    words; dst is device words on even turns and a transform buffer on odd ones, where it may be the buffer a table sits in: in
    place.  Every table holds n known words; dst holds random bytes, or the table's."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    words = [DeviceBuffer(0, 32 * n) for _ in range(12)]
    out = DeviceBuffer(0, 32 * n)
    for turn, (name, (nt, terms, common)) in enumerate(CATALOGUE.items()):
        vals = gate_inputs(r, nt, n, 11000 * logn + 100 * turn + len(field))
        raw = [_pack(v) for v in vals]
        buffers = [turn % nt, (turn + 3) % nt] if nt > 1 else ([0] if turn % 2 == 0 else [])
        held = [fill(n, 2 * turn), fill(n, 2 * turn + 1)]   # what the transform buffers hold
        tabs, w = [], 0
        for j, b in enumerate(raw):
            if j in buffers:
                held[buffers.index(j)] = b
                tabs.append(buffers.index(j))
            else:
                words[w].upload(b)
                tabs.append(words[w])
                w += 1
        for b in (0, 1):
            cl.set_data(NTTInput(b, held[b]))
        dst = out if turn % 2 == 0 else (turn // 2) % 2
        before = fill(n, 90 + turn) if dst is out else held[dst]
        out.upload(fill(n, 90 + turn))
        want = _ref(vals, terms, common, r, length)
        cl.gate_eval(dst, tabs, terms, common, length=length)
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        assert _bytes_of(cl, dst) == _pack(want) + before[32 * length:], (name, "dst")
        for j, t in enumerate(tabs):
            if t is not dst and not (isinstance(t, int) and t == dst):
                assert _bytes_of(cl, t) == raw[j], (name, j, "a table changed")
        for b in (0, 1):
            if b != dst:
                assert bytes(cl.result(b)) == held[b], (name, b, "the other buffer changed")
        if dst is not out:
            assert bytes(out.download()) == fill(n, 90 + turn)
        if name == "G5Z":
            assert want == [0] * length
    cl.close()
    for d in words + [out]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_edge_words_in_every_factor_position(gpu, field):
    """A four-factor term over four tables whose first 6^4 positions hold every combination of 0, 1, r - 1, r, r + 1, 2^256 - 1 -
    2^256 - 1, r and r + 1 in every factor position among them - alone, negated beside a one-factor term, under a common
    factor, and as one table to the fourth power."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    edges = [0, 1, r - 1, r, r + 1, TOP]
    combos = list(itertools.product(edges, repeat=4))
    vals = [[c[j] for c in combos] + _words(400 + j + len(field), n - len(combos)) for j in range(4)]
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(vals[0])))
    tabs = [0] + [_dev(_pack(v)) for v in vals[1:]]
    out = DeviceBuffer(0, 32 * n)
    for terms, common in (([(1, [0, 1, 2, 3])], None), ([(-1, [3, 2, 1, 0]), (1, [1])], None), ([(1, [0, 1, 2, 3])], 3), ([(1, [1, 1, 1, 1]), (-1, [2, 2, 2])], 0)):
        cl.gate_eval(out, tabs, terms, common)
        cl.wait_result()
        assert bytes(out.download()) == _pack(_ref(vals, terms, common, r, n)), (terms, common)
    cl.close()
    for d in tabs[1:] + [out]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_periodic_tables(gpu, field):
    """The PLONK gate with selectors of 1, 4 and n words mixed, and a linear combination of six with one-word coefficients."""
    logn = 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 12, n, 12000 + len(field))
    counts = [1, 4, n, 4, 1, n, n, n]   # qL, qR, qM, qO, qC, a, b, c
    pv = [v[:k] for v, k in zip(vals, counts)]
    cl.set_data(NTTInput(0, _pack(pv[5])))
    cl.set_data(NTTInput(1, _pack(pv[6])))
    tabs = [_dev(_pack(v)) for v in pv[:5]] + [0, 1, _dev(_pack(pv[7]))]
    out = _dev(fill(n, 3))
    cl.gate_eval(out, tabs, PLONK, length=n - 5)
    cl.wait_result()
    assert bytes(out.download()) == _pack(_ref(pv, PLONK, None, r, n - 5)) + fill(n, 3)[32 * (n - 5):]
    for t, v in zip(tabs, pv):
        assert _bytes_of(cl, t) == _pack(v)
    # sum_{j < 6} c_j f_j: coefficients at even indices, polynomials at odd ones; r + 1 and 2^256 - 1 among the coefficients
    lv = []
    for j in range(6):
        lv += [[[r + 1, TOP, 0, 7, r - 1, vals[j][9]][j]], vals[6 + j]]
    lin = [(1, [2 * j, 2 * j + 1]) for j in range(6)]
    ltabs = [_dev(_pack(v)) for v in lv]
    cl.gate_eval(1, ltabs, lin)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(_ref(lv, lin, None, r, n))
    cl.close()
    for d in [t for t in tabs if isinstance(t, DeviceBuffer)] + ltabs + [out]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_rotations(gpu, field):
    """One rotation value on every table, different values on the tables of one gate, the same words under two indices with two
    rotations (Z and Z(wX)), and rot = NULL against all zeros."""
    logn = 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 8, n, 13000 + len(field))
    vals[3] = vals[3][:4]   # qO: a count-4 table
    cl.set_data(NTTInput(0, _pack(vals[5])))
    tabs = [_dev(_pack(v)) for v in vals[:5]] + [0] + [_dev(_pack(v)) for v in vals[6:]]
    out = DeviceBuffer(0, 32 * n)
    cases = [[k] * 8 for k in (0, 1, 4, n - 1, n, M64)]
    cases += [[0, 0, 0, 3, 0, 0, 0, 0], [1, 4, n - 1, 3, M64, 2 * n + 5, 0, (1 << 63) + 7]]
    for rot in cases:
        cl.gate_eval(out, tabs, PLONK, rot=rot, length=n - 3)
        cl.wait_result()
        assert bytes(out.download())[:32 * (n - 3)] == _pack(_ref(vals, PLONK, None, r, n - 3, rot)), rot
    # a negative rotation is taken modulo 2^64 by the client: -1 is the previous row
    cl.gate_eval(out, tabs, PLONK, rot=[-1] * 8)
    cl.wait_result()
    assert bytes(out.download()) == _pack(_ref(vals, PLONK, None, r, n, [M64] * 8))
    # Z (wX) a - Z b: the same words as tables 0 and 1, rotated by 1 and by 0; on buffer 0 and on device words
    z = tabs[6]
    for zt, zv in ((z, vals[6]), (0, vals[5])):
        terms, zvals = [(1, [0, 2]), (-1, [1, 3])], [zv, zv, vals[0], vals[1]]
        cl.gate_eval(out, [zt, zt, tabs[0], tabs[1]], terms, rot=[1, 0, 0, 0])
        cl.wait_result()
        assert bytes(out.download()) == _pack(_ref(zvals, terms, None, r, n, [1, 0, 0, 0]))
    # rot = NULL is all zeros
    cl.gate_eval(out, tabs, PLONK, rot=[0] * 8)
    cl.wait_result()
    zeros = bytes(out.download())
    out.upload(fill(n, 5))
    assert raw_eval(cl, make_gate(8, PLONK, None), out, tabs, None, n) == 0
    cl.wait_result()
    assert bytes(out.download()) == zeros == _pack(_ref(vals, PLONK, None, r, n))
    cl.close()
    for d in [t for t in tabs if isinstance(t, DeviceBuffer)] + [out]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_in_place(gpu, field):
    """dst a buffer that is also a table, dst device words that are also a table: the out-of-place bytes.  dst <- dst + alpha a b
    in one op, over a live length below n: the words behind keep their values."""
    logn = 10
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 9, n, 14000 + len(field))
    nt, terms, common = CATALOGUE["G3"]
    raw = [_pack(v) for v in vals]
    want = _pack(_ref(vals, terms, common, r, n))
    out = DeviceBuffer(0, 32 * n)
    for place in (0, 6, 8):   # the common factor, a table named twice, a table named once
        devs = [_dev(b) for b in raw]
        cl.gate_eval(out, devs, terms, common)
        cl.wait_result()
        assert bytes(out.download()) == want
        cl.gate_eval(devs[place], devs, terms, common)   # device words
        cl.wait_result()
        assert bytes(devs[place].download()) == want, place
        cl.set_data(NTTInput(1, raw[place]))
        tabs = devs[:place] + [1] + devs[place + 1:]
        cl.gate_eval(1, tabs, terms, common)   # a buffer
        cl.wait_result()
        assert bytes(cl.result(1)) == want, place
        for j, d in enumerate(devs):
            if j != place:
                assert bytes(d.download()) == raw[j], (place, j)
            d.free()
    alpha = cl.scalar(TOP)
    length = n - 77
    acc, a, b = _dev(raw[0]), _dev(raw[1]), _dev(raw[2])
    terms = [(1, [0]), (1, [1, 2, 3])]
    cl.gate_eval(acc, [acc, alpha, a, b], terms, length=length)
    cl.wait_result()
    assert bytes(acc.download()) == _pack(_ref([vals[0], [TOP], vals[1], vals[2]], terms, None, r, length)) + raw[0][32 * length:]
    assert bytes(a.download()) == raw[1] and bytes(b.download()) == raw[2] and _word(alpha) == TOP
    cl.close()
    for d in (out, alpha, acc, a, b):
        d.free()


def test_against_the_existing_ops_at_2_20(gpu):
    """BLS12-381, n = 2^20: two sweeps of the 2048 x 256 grid.  a b + c gives BLZ_VEC_MULADD's bytes; the sum of the PLONK gate's
    output is out[0] + out[1] of blz_ntt_sumcheck_gate without r at two points over the same tables."""
    field, logn = "BLS381", 20
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    raw = [random.Random(2400 + j).randbytes(32 * n) for j in range(8)]
    tabs = [_dev(b) for b in raw]
    cl.vec_op(NTTClient.MULADD, 0, tabs[0], tabs[1], tabs[2])
    cl.wait_result()
    cl.gate_eval(1, tabs[:3], [(1, [0, 1]), (1, [2])])
    cl.wait_result()
    assert bytes(cl.result(1)) == bytes(cl.result(0))
    cl.gate_eval(0, tabs, PLONK)
    cl.wait_result()
    total = cl.vec_reduce(NTTClient.FOLD_SUM, 0)
    cl.wait_result()
    s = cl.sumcheck_gate(tabs, PLONK, points=2)
    cl.wait_result()
    g = _unpack(s.download())
    assert _word(total) == (g[0] + g[1]) % r
    # and a few positions against Python integers: the first, the last, the two sides of the second sweep's start
    got = bytes(cl.result(0))
    for p in (0, n - 1, 2048 * 256 - 1, 2048 * 256, 777777):
        v = [int.from_bytes(b[32 * p: 32 * p + 32], "little") for b in raw]
        assert got[32 * p: 32 * p + 32] == gate_value(v, PLONK, None, r).to_bytes(32, "little"), p
    cl.close()
    for d in tabs + [total, s]:
        d.free()


def test_refusals(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM (InvalidPrimitiveParam) with a message that names the cause, and leaves dst,
    the tables and the in-flight state as they were."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    ab, bb = _pack(_inputs(r, n, 61)), _pack(_inputs(r, n, 62))
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words, words2 = _dev(bb), _dev(ab)
    big = _dev(bytes(64 * n))   # 2n words
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    B0, B1, W, W2 = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(words2.ptr, 0, 0, n)
    W8 = V(words.ptr, 0, 0, 8)
    ONE, AB = [(1, [0])], [(1, [0, 1])]

    def ev(gate, dst, tables, rot, length):
        return raw_eval(cl, gate, dst, tables, rot, length)

    def g(nt, terms, common=None, **kw):
        return make_gate(nt, terms, common, **kw)

    def bent(**fields):
        """the gate a b over two tables with fields of the description or of its first term overwritten"""
        x = g(2, AB)
        for k, v in fields.items():
            if k in ("ntables", "nterms", "common", "reserved"):
                setattr(x, k, v)
            elif k == "term_reserved":
                x.term[0].reserved[v] = 1
            elif k == "factor1":
                x.term[0].factor[1] = v
            else:
                setattr(x.term[0], k, v)
        return x

    T2 = [B1, W2]
    assert L.blz_ntt_gate_eval(None, None, None, None, None, 3) == 4 and b"null handle" in L.blz_last_error_message()
    refused = {
        "null gate": (lambda: ev(None, W, [B0], None, n), "gate is NULL"),
        "null dst": (lambda: ev(g(1, ONE), None, [B0], None, n), "dst is NULL"),
        "null tables": (lambda: ev(g(1, ONE), W, None, None, n), "tables is NULL"),
        # the description errors, with blz_ntt_sumcheck_gate's messages
        "ntables 0": (lambda: ev(bent(ntables=0), W, T2, None, n), "gate: ntables 0 is not in [1, 12]"),
        "ntables 13": (lambda: ev(bent(ntables=13), W, [B1] + [W2] * 12, None, n), "gate: ntables 13 is not in [1, 12]"),
        "nterms 0": (lambda: ev(bent(nterms=0), W, T2, None, n), "gate: nterms 0 is not in [1, 8]"),
        "nterms 9": (lambda: ev(bent(nterms=9), W, T2, None, n), "gate: nterms 9 is not in [1, 8]"),
        "nfactors 0": (lambda: ev(bent(nfactors=0), W, T2, None, n), "gate: term 0: nfactors 0 is not in [1, 4]"),
        "nfactors 5": (lambda: ev(bent(nfactors=5), W, T2, None, n), "gate: term 0: nfactors 5 is not in [1, 4]"),
        "a factor at ntables": (lambda: ev(bent(factor1=2), W, T2, None, n), "gate: term 0: factor 1 names table 2, ntables is 2"),
        "a factor of 255": (lambda: ev(bent(factor1=255), W, T2, None, n), "factor 1 names table 255"),
        "common at ntables": (lambda: ev(bent(common=2), W, T2, None, n), "gate: common 2 is neither -1 nor a table index below ntables 2"),
        "common -2": (lambda: ev(bent(common=-2), W, T2, None, n), "gate: common -2 is neither -1 nor a table index"),
        "gate reserved": (lambda: ev(bent(reserved=1), W, T2, None, n), "gate: reserved must be 0"),
        "term reserved 0": (lambda: ev(bent(term_reserved=0), W, T2, None, n), "gate: term 0: reserved must be 0"),
        "term reserved 1": (lambda: ev(bent(term_reserved=1), W, T2, None, n), "gate: term 0: reserved must be 0"),
        "negate 2": (lambda: ev(bent(negate=2), W, T2, None, n), "gate: term 0: negate 2 is not 0 or 1"),
        "a bad second term": (lambda: ev(g(2, [(1, [0]), (1, [1, 2])]), W, T2, None, n), "gate: term 1: factor 1 names table 2"),
        # len
        "len 0": (lambda: ev(g(1, ONE), W, [B0], None, 0), "len 0: a gate evaluation writes 1 <= len <= 256 words"),
        "len n + 1": (lambda: ev(g(1, ONE), V(big.ptr, 0, 0, n), [B0], None, n + 1), "len 257: a gate evaluation writes 1 <= len <= 256 words"),
        "len above dst's count": (lambda: ev(g(1, ONE), W8, [B0], None, 9), "operand dst: count 8 is below the 9 words the op writes"),
        # the overlap rules
        "a table meeting dst off its start": (lambda: ev(g(2, AB), V(words.ptr + 32 * 4, 0, 0, 8), [B0, W], None, 8), "dst overlaps the words of tables[1] without starting where they start"),
        "a table inside dst": (lambda: ev(g(2, AB), W, [B0, V(words.ptr + 32 * 16, 0, 0, 1)], None, n), "dst overlaps the words of tables[1] without starting"),
        "a table at dst's start, rotated": (lambda: ev(g(2, AB), W, [W, B0], [1, 0], n), "dst names the words of tables[0], which is rotated by 1"),
        "a buffer at dst's start, rotated": (lambda: ev(g(2, AB), B1, [B0, B1], [0, n], n), "dst names the words of tables[1], which is rotated by 256"),
        "a table at dst's start, shorter than len": (lambda: ev(g(2, AB), W, [W8, B0], None, 9), "dst names the 8 words of tables[0], read periodically over len 9"),
        "a scalar at dst's start": (lambda: ev(g(2, AB), W, [B0, V(words.ptr, 0, 0, 1)], None, 2), "dst names the 1 words of tables[1], read periodically over len 2"),
        # operands, dst among them
        "tables[0] misaligned": (lambda: ev(g(1, ONE), W, [V(words2.ptr + 8, 0, 0, 1)], None, n), "operand tables[0]: d_ptr is not 16-byte aligned"),
        "dst misaligned": (lambda: ev(g(1, ONE), V(words.ptr + 8, 0, 0, 8), [B0], None, 8), "operand dst: d_ptr is not 16-byte aligned"),
        "tables[1] in host memory": (lambda: ev(g(2, AB), W, [B0, V(host_ptr, 0, 0, n)], None, n), "operand tables[1]: d_ptr is not"),
        "dst in host memory": (lambda: ev(g(1, ONE), V(host_ptr, 0, 0, n), [B0], None, n), "operand dst: d_ptr is not"),
        "tables[0] reserved": (lambda: ev(g(1, ONE), W, [V(None, 0, 7, 0)], None, n), "operand tables[0]: reserved must be 0"),
        "dst reserved": (lambda: ev(g(1, ONE), V(words.ptr, 0, 1, n), [B0], None, n), "operand dst: reserved must be 0"),
        "tables[1] buf 2": (lambda: ev(g(2, AB), W, [B0, V(None, 2, 0, 0)], None, n), "operand tables[1]: buf must be 0 or 1"),
        "dst buf 2": (lambda: ev(g(1, ONE), V(None, 2, 0, 0), [B0], None, n), "operand dst: buf must be 0 or 1"),
        "tables[1] buffer count": (lambda: ev(g(2, AB), W, [B0, V(None, 1, 0, 8)], None, n), "operand tables[1]: a transform buffer holds 256 elements, count says 8"),
        "tables[1] count 3": (lambda: ev(g(2, AB), W, [B0, V(words2.ptr, 0, 0, 3)], None, n), "operand tables[1]: count 3 is not a power of two"),
        "tables[0] count 2n": (lambda: ev(g(1, ONE), W, [V(big.ptr, 0, 0, 2 * n)], None, n), "operand tables[0]: count 512 is not a power of two in [1, 256]"),
        "dst count 2n": (lambda: ev(g(1, ONE), V(big.ptr, 0, 0, 2 * n), [B0], None, n), "operand dst: count 512 is not a power of two in [1, 256]"),
        "tables[11] past its allocation": (lambda: ev(g(12, ONE), W, [B0] * 11 + [V(words2.ptr + 32 * (n - 1), 0, 0, 2)], None, n), "operand tables[11]: 2 elements run past the end"),
        "dst past its allocation": (lambda: ev(g(1, ONE), V(words.ptr + 32 * (n - 4), 0, 0, 8), [B0], None, 8), "operand dst: 8 elements run past the end"),
    }
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    with pytest.raises(DriverClientError) as ei:
        cl.gate_eval(0, [0, 1], [(1, [0, 1, 0, 1, 0])])   # five factors: the library's to refuse
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(ValueError):
        cl.gate_eval(0, [0, 1], AB, rot=[1])
    # an op already in flight
    cl.vec_op(NTTClient.MUL, 1, 1, words2)
    assert ev(g(1, ONE), W, [B0], None, n) == 4 and "already running" in L.blz_last_error_message().decode()
    cl.reset()
    assert bytes(cl.result(0)) == ab
    assert bytes(words.download()) == bb and bytes(words2.download()) == ab and bytes(big.download()) == bytes(64 * n)
    cl.close()
    for d in (words, words2, big):
        d.free()


def test_in_flight_rules(gpu):
    """With the op in flight the buffer written can be neither read, written nor exchanged, a buffer only read can be read but
    not written, and no transform, set_coset or op on the buffers starts.  wait_result finishes it, reset drops it."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c = (_inputs(r, n, 70 + i) for i in range(3))
    ab, bb, cb = _pack(a), _pack(b), _pack(c)
    cl = _client(field, logn)
    words, one_word, out = _dev(cb), _dev((7).to_bytes(32, "little")), DeviceBuffer(0, 32 * n)
    host_out = bytearray(32 * n)
    terms = [(1, [0, 1]), (-1, [1])]
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.sumcheck_gate([words], [(1, [0])]), lambda: cl.gate_eval(out, [words], [(1, [0])]),
            lambda: cl.gate_eval(1, [0, words], terms))
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    cl.gate_eval(1, [0, words], terms)   # writes buffer 1, reads buffer 0
    for attempt in busy + (lambda: cl.result(1), lambda: cl.set_data(NTTInput(1, ab)), lambda: cl.set_data(NTTInput(0, ab)),
                           lambda: cl.exchange(1, ab, host_out)):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    assert bytes(cl.result(0)) == ab   # read-only: readable
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want = _pack(_ref([a, c], terms, None, r, n))
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab
    # dst in device words: both buffers are at most read
    cl.gate_eval(out, [0, 1, words], [(1, [0, 1, 2])])
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == want
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(out.download()) == _pack(_ref([a, _unpack(want), c], [(1, [0, 1, 2])], None, r, n))
    # reset with the op in flight: nothing is in flight afterwards, and the handle works
    cl.gate_eval(1, [0, words], terms)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.result(0); cl.result(1)
    cl.set_data(NTTInput(1, bb))
    cl.gate_eval(1, [0, 1], [(1, [0, 1])])
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(_ref([a, b], [(1, [0, 1])], None, r, n))
    cl.close()
    for d in (words, one_word, out):
        d.free()
