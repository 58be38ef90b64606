"""The sumcheck step for caller-defined gates (blz_ntt_sumcheck_gate) on the device: the bind of every table in place and the
round polynomial of a gate given as data, the round alone, the bind alone, agreement with blz_ntt_sumcheck_step where the two
overlap, the refusals, the in-flight rules and a PLONK zerocheck driven through it.  Every expected value is Python integer
arithmetic (tests/ntt_gate_util.py) or, at 2^22, the existing step, and every comparison is byte for byte: any 256-bit input word
counts as its residue, every word written is canonical, exactly len / 2 words of each table are written and no byte outside them
- nor beside d_out - changes."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_gate_util import CATALOGUE, PLONK_TERMS, gate_inputs, gate_value, make_gate, raw_gate, sum_gate_ref
from ntt_mle_util import challenges, check_order_of_checks, fill, fold_ref, interpolate
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, _client, _dev, _pack, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
R1CS, PRODUCT = NTTClient.GATE_R1CS, NTTClient.GATE_PRODUCT
# (log n, len) - the launcher's boundaries are those of blz_ntt_sumcheck_step: with r one quad; less than a block; 256 quads,
# exactly one block: d_out written directly; two blocks: workspace and finish; a live length below n.  Without r the items are
# pairs: len = 512 is exactly one block, 1024 and 2048 take the workspace
SIZES = [(2, 4), (6, 64), (10, 1024), (11, 2048), (11, 512)]
MAXP = 6


def _bytes_of(cl, t):
    return bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))


def _place(cl, words, buffers, data):
    """Table j's bytes go to transform buffer b where buffers[b] == j, else to the next of `words`; returns the table operands"""
    tabs, w = [], 0
    for j, b in enumerate(data):
        if j in buffers:
            cl.set_data(NTTInput(buffers.index(j), b))
            tabs.append(buffers.index(j))
        else:
            words[w].upload(b)
            tabs.append(words[w])
            w += 1
    return tabs


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_bind_and_round_against_python_integers(gpu, field, logn, length):
    """Every catalogue gate at points = 1 .. 6.  r walks through 0, 1, r - 1, r + 1 and a random word >= r from gate to gate (the
    six points of one gate share r and the inputs, so the integer reference is taken once, at six points); two of the tables sit
    in the transform buffers - which two moves with the gate -, the rest in device words.  Before each call every table holds
    `length` known words with random bytes behind them."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    rs = challenges(r, logn)
    drs = [cl.scalar(v) for v in rs]
    words = [DeviceBuffer(0, 32 * n) for _ in range(12)]
    guard = DeviceBuffer(0, 32 * (MAXP + 2))
    half = length // 2
    for turn, (name, (nt, terms, common)) in enumerate(CATALOGUE.items()):
        which = (turn + logn + len(field)) % 5
        rr, dr = rs[which], drs[which]
        vals = gate_inputs(r, nt, length, 7000 * logn + 100 * turn + len(field))
        before = [_pack(v) + fill(n - length, turn * 12 + j) for j, v in enumerate(vals)]
        buffers = [turn % nt, (turn + 3) % nt] if nt > 1 else ([0] if turn % 2 == 0 else [])
        folded = [fold_ref(v, r, rr, length) for v in vals]
        want = sum_gate_ref(folded, terms, common, r, half, MAXP)
        gate = make_gate(nt, terms, common)
        for points in range(1, MAXP + 1):
            tabs = _place(cl, words, buffers, before)
            gfill = fill(MAXP + 2, turn + 50 + points)
            guard.upload(gfill)
            assert raw_gate(cl, gate, tabs, dr, points, length, guard.ptr + 32) == 0, blaze_amd.lib().blz_last_error_message()
            cl.wait_result()
            assert cl.last_kernel_ms() > 0
            for j, t in enumerate(tabs):
                got = _bytes_of(cl, t)
                assert got[:32 * half] == _pack(folded[j]), (name, points, j, rr)
                assert got[32 * half:] == before[j][32 * half:], (name, points, j, "bytes behind the words written")
            assert bytes(guard.download()) == gfill[:32] + _pack(want[:points]) + gfill[32 * (1 + points):], (name, points, rr)
        if name == "G5Z":
            assert want == [0] * MAXP
    cl.close()
    for d in drs + words + [guard]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_round_only(gpu, field, logn, length):
    """r = None: pairs in place of quads (one block up to len = 512, workspace and finish above).  Every catalogue gate, and the
    PLONK gate with periodic selectors - qC one word, qM four; each gate at two point counts, 1 .. 6 all met.  No table byte
    changes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 12, n, 8000 * logn + len(field))
    raw = [_pack(v) for v in vals]
    words = [_dev(b) for b in raw[2:]]
    cl.set_data(NTTInput(0, raw[0]))
    cl.set_data(NTTInput(1, raw[1]))
    tabs = [0, 1] + words
    p1, p4 = _dev(raw[5][:32]), _dev(raw[3][:128])
    cases = [(name, tabs[:nt], vals[:nt], terms, common) for name, (nt, terms, common) in CATALOGUE.items()]
    per_t, per_v = list(tabs[:9]), list(vals[:9])
    per_t[5], per_v[5], per_t[3], per_v[3] = p1, vals[5][:1], p4, vals[3][:4]
    cases.append(("G3 periodic", per_t, per_v, PLONK_TERMS, 0))
    mark = bytes(range(100, 132))
    for turn, (name, tt, vv, terms, common) in enumerate(cases):
        want = sum_gate_ref(vv, terms, common, r, length, MAXP)
        for points in (1 + turn % MAXP, 1 + (turn + 3) % MAXP):
            out = _dev(fill(points, points) + mark)
            got = cl.sumcheck_gate(tt, terms, common, points=points, length=length, out=out)
            cl.wait_result()
            assert got is out and bytes(out.download()) == _pack(want[:points]) + mark, (name, points)
            out.free()
    out = cl.sumcheck_gate(tabs[:9], PLONK_TERMS, 0, length=length)   # points: the degree + 1
    cl.wait_result()
    assert out.nbytes == 32 * 5 and bytes(out.download()) == _pack(sum_gate_ref(vals[:9], PLONK_TERMS, 0, r, length, 5))
    for t, b in zip(tabs, raw):
        assert _bytes_of(cl, t) == b
    assert bytes(p1.download()) == raw[5][:32] and bytes(p4.download()) == raw[3][:128]
    cl.close()
    for d in words + [p1, p4, out]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_bind_only(gpu, field):
    """points = 0, d_out NULL: all twelve tables of G4 - the two no term names among them - folded in one op, at len = 2 and at
    len = n; a thirteenth buffer of device words that is not a table keeps every byte."""
    logn = 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    nt, terms, common = CATALOGUE["G4"]
    cl = _client(field, logn)
    rs = challenges(r, 3)
    words = [DeviceBuffer(0, 32 * n) for _ in range(10)]
    for turn, length in enumerate((2, n)):
        rr = rs[(turn + 3 + len(field)) % 5]
        dr = cl.scalar(rr)
        vals = gate_inputs(r, nt, n, 9000 + 100 * turn + len(field))
        raw = [_pack(v) for v in vals]
        tabs = _place(cl, words, [11, 4], raw)
        other = _dev(raw[0])
        assert cl.sumcheck_gate(tabs, terms, common, r=dr, points=0, length=length) is None
        cl.wait_result()
        half = length // 2
        for j, t in enumerate(tabs):
            assert _bytes_of(cl, t) == _pack(fold_ref(vals[j], r, rr, length)) + raw[j][32 * half:], (length, j)
        assert bytes(other.download()) == raw[0] and _word(dr) == rr
        other.free()
        dr.free()
    cl.close()
    for d in words:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_agrees_with_the_existing_step(gpu, field):
    """G1, a b, a b c and G2 (R1CS as a sum gate) give the bytes of blz_ntt_sumcheck_step - d_out and the folded tables - on
    copies of the same inputs, len 2^12: sixteen blocks of quads, workspace and finish."""
    logn = 12
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    dr = cl.scalar(_words(len(field), 1)[0])
    raw = [_pack(_inputs(r, n, 9500 + j + len(field))) for j in range(4)]
    pairs = [(PRODUCT, 1, [(1, [0])], None), (PRODUCT, 2, [(1, [0, 1])], None), (PRODUCT, 3, [(1, [0, 1, 2])], None),
             (R1CS, 4, [(1, [1, 2]), (-1, [3])], 0)]
    for gate, k, terms, common in pairs:
        u = [_dev(raw[j]) for j in range(k)]
        want = cl.sumcheck_step(u, dr, gate=gate)
        cl.wait_result()
        f = [_dev(raw[j]) for j in range(2, k)]
        for b in range(min(k, 2)):
            cl.set_data(NTTInput(b, raw[b]))
        tabs = list(range(min(k, 2))) + f
        out = cl.sumcheck_gate(tabs, terms, common, r=dr)   # points: the gate's degree + 1, the existing step's default
        cl.wait_result()
        assert out.nbytes == want.nbytes and bytes(out.download()) == bytes(want.download()), (gate, k)
        for t, ut in zip(tabs, u):
            assert _bytes_of(cl, t) == bytes(ut.download()), (gate, k)
        for d in u + f + [out, want]:
            d.free()
    cl.close()
    dr.free()


def test_second_sweep_of_the_grid_stride_loop(gpu):
    """BLS12-381, len = n = 2^22: 2^20 quads are two sweeps of the 2048 x 256 grid.  G2 over both buffers and two device-word
    tables against BLZ_GATE_R1CS run beforehand on the same bytes: d_out, every folded word and the bytes behind them."""
    field, logn = "BLS381", 22
    n = 1 << logn
    half = n // 2
    r = pyref.CURVES[field]["r"]
    raw = [random.Random(2300 + j).randbytes(32 * n) for j in range(4)]
    rr = _words(2304, 1)[0]
    cl = _client(field, logn)
    dr = cl.scalar(rr)
    w = [DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)]
    tabs = [w[1], 0, 1, w[0]]   # eq, Az, Bz, Cz

    def load():
        w[1].upload(raw[0]); cl.set_data(NTTInput(0, raw[1])); cl.set_data(NTTInput(1, raw[2])); w[0].upload(raw[3])

    load()
    s = cl.sumcheck_step(tabs, dr, gate=R1CS)
    cl.wait_result()
    want, want_tabs = bytes(s.download()), [_bytes_of(cl, t) for t in tabs]
    load()
    nt, terms, common = CATALOGUE["G2"]
    out = cl.sumcheck_gate(tabs, terms, common, r=dr)
    cl.wait_result()
    assert out.nbytes == 128 and bytes(out.download()) == want
    rng = random.Random(2305)
    for t, e, src in zip(tabs, want_tabs, raw):
        got = _bytes_of(cl, t)
        assert got == e and got[32 * half:] == src[32 * half:]
        for p in [0, half - 1] + [rng.randrange(half) for _ in range(30)]:
            lo, hi = (int.from_bytes(src[32 * q: 32 * q + 32], "little") for q in (p, p + half))
            assert got[32 * p: 32 * p + 32] == ((lo + rr * (hi - lo)) % r).to_bytes(32, "little"), p
    cl.close()
    for d in w + [s, out, dr]:
        d.free()


def test_refusals(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM (InvalidPrimitiveParam) with a message that names the cause, and leaves the
    tables, d_out and the in-flight state as they were."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 61), _inputs(r, n, 62)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words, words2 = _dev(bb), _dev(ab)
    one_word = _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 225))
    out = _dev(mark)           # 7 words
    big = _dev(bytes(64 * n))  # 2n words
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    B0, B1, W, W2, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(words2.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    P4 = V(words2.ptr, 0, 0, 4)
    o = out.ptr
    ONE = [(1, [0])]
    AB = [(1, [0, 1])]
    G2 = CATALOGUE["G2"][1]

    def step(gate, tables, rr, points, length, d_out):
        return raw_gate(cl, gate, tables, rr, points, length, d_out)

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

    thirteen = [B0] + [W] * 12
    assert L.blz_ntt_sumcheck_gate(None, None, None, None, 77, 3, None) == 4 and b"null handle" in L.blz_last_error_message()
    refused = {
        "null gate": (lambda: step(None, [B0], R, 2, n, o), "gate is NULL"),
        "null tables": (lambda: step(g(1, ONE), None, R, 2, n, o), "tables is NULL"),
        "ntables 0": (lambda: step(bent(ntables=0), [B0, B1], R, 3, n, o), "ntables 0 is not in [1, 12]"),
        "ntables 13": (lambda: step(bent(ntables=13), thirteen, R, 3, n, o), "ntables 13 is not in [1, 12]"),
        "nterms 0": (lambda: step(bent(nterms=0), [B0, B1], R, 3, n, o), "nterms 0 is not in [1, 8]"),
        "nterms 9": (lambda: step(bent(nterms=9), [B0, B1], R, 3, n, o), "nterms 9 is not in [1, 8]"),
        "nfactors 0": (lambda: step(bent(nfactors=0), [B0, B1], R, 3, n, o), "term 0: nfactors 0 is not in [1, 4]"),
        "nfactors 5": (lambda: step(bent(nfactors=5), [B0, B1], R, 3, n, o), "term 0: nfactors 5 is not in [1, 4]"),
        "a factor at ntables": (lambda: step(bent(factor1=2), [B0, B1], R, 3, n, o), "term 0: factor 1 names table 2, ntables is 2"),
        "a factor of 255": (lambda: step(bent(factor1=255), [B0, B1], None, 3, n, o), "factor 1 names table 255"),
        "common at ntables": (lambda: step(bent(common=2), [B0, B1], R, 3, n, o), "common 2 is neither -1 nor a table index"),
        "common -2": (lambda: step(bent(common=-2), [B0, B1], R, 3, n, o), "common -2 is neither -1 nor a table index"),
        "gate reserved": (lambda: step(bent(reserved=1), [B0, B1], R, 3, n, o), "gate: reserved must be 0"),
        "term reserved 0": (lambda: step(bent(term_reserved=0), [B0, B1], R, 3, n, o), "term 0: reserved must be 0"),
        "term reserved 1": (lambda: step(bent(term_reserved=1), [B0, B1], None, 3, n, o), "term 0: reserved must be 0"),
        "negate 2": (lambda: step(bent(negate=2), [B0, B1], R, 3, n, o), "term 0: negate 2 is not 0 or 1"),
        "a bad second term": (lambda: step(g(2, [(1, [0]), (1, [1, 2])]), [B0, B1], R, 3, n, o), "term 1: factor 1 names table 2"),
        "points 7": (lambda: step(g(1, ONE), [B0], R, 7, n, o), "points 7 is not in [0, 6]"),
        "points 0 without r": (lambda: step(g(1, ONE), [B0], None, 0, n, None), "points 0 is a bind alone"),
        "points 0 with d_out": (lambda: step(g(1, ONE), [B0], R, 0, n, o), "points 0 is a bind alone"),
        "null d_out": (lambda: step(g(2, AB), [B0, B1], R, 3, n, None), "null d_out"),
        "null d_out, round only": (lambda: step(g(4, G2, 0), [B0, B1, W, W2], None, 4, n, None), "null d_out"),
        "len 0": (lambda: step(g(1, ONE), [B0], R, 2, 0, o), "len 0: the live length is 2^m with 2 <= len <= 256"),
        "len 1": (lambda: step(g(1, ONE), [B0], None, 2, 1, o), "len 1: the live length is 2^m"),
        "len 12": (lambda: step(g(1, ONE), [B0], R, 2, 12, o), "len 12: the live length is 2^m"),
        "len 2n": (lambda: step(g(1, ONE), [B0], R, 2, 2 * n, o), "len 512: the live length is 2^m"),
        "len 2 with r and a round": (lambda: step(g(1, ONE), [B0], R, 2, 2, o), "a bind and a round need len >= 4"),
        "r names a buffer": (lambda: step(g(1, ONE), [B0], B1, 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "r of two words": (lambda: step(g(1, ONE), [B0], V(words.ptr, 0, 0, 2), 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "r in host memory": (lambda: step(g(1, ONE), [B0], V(host_ptr, 0, 0, 1), 2, n, o), "operand r: d_ptr is not"),
        "periodic table with r": (lambda: step(g(2, AB), [B0, P4], R, 3, 8, o), "operand tables[1]: 4 words, read periodically over len 8"),
        "periodic table nobody names, with r": (lambda: step(g(2, ONE), [B0, P4], R, 3, 8, o), "operand tables[1]: 4 words, read periodically"),
        "periodic table, bind only": (lambda: step(g(1, ONE), [P4], R, 0, 8, None), "operand tables[0]: 4 words, read periodically over len 8"),
        "the same buffer twice": (lambda: step(g(2, AB), [B0, B0], R, 3, n, o), "tables[0] and tables[1] overlap"),
        "the same words twice": (lambda: step(g(4, G2, 0), [B0, W, B1, W], R, 4, n, o), "tables[1] and tables[3] overlap"),
        "tables that overlap in part": (lambda: step(g(2, AB), [V(words.ptr, 0, 0, 8), V(words.ptr + 32 * 4, 0, 0, 8)], R, 3, 8, o), "tables[0] and tables[1] overlap"),
        "r in the words written": (lambda: step(g(1, ONE), [W], V(words.ptr + 32 * 3, 0, 0, 1), 2, 8, o), "r lies in the words tables[0] receives"),
        "r in the words of tables[1] written": (lambda: step(g(2, AB), [B0, W], V(words.ptr, 0, 0, 1), 3, 8, o), "r lies in the words tables[1] receives"),
        "d_out in host memory": (lambda: step(g(1, ONE), [B0], R, 2, n, host_ptr), "operand d_out: d_ptr is not"),
        "d_out misaligned": (lambda: step(g(1, ONE), [B0], R, 2, n, o + 8), "operand d_out: d_ptr is not 16-byte aligned"),
        "d_out past its allocation": (lambda: step(g(1, ONE), [B0], R, 6, n, o + 64), "operand d_out: 6 elements run past the end"),
        "d_out on a table": (lambda: step(g(2, AB), [B0, W], R, 3, n, words.ptr + 32 * (n - 3)), "d_out overlaps the words of a d_ptr operand"),
        "d_out on a table, round only": (lambda: step(g(4, G2, 0), [B0, W, B1, W2], None, 4, n, words2.ptr), "d_out overlaps the words of a d_ptr operand"),
        "d_out on r": (lambda: step(g(1, ONE), [B0], R, 1, n, one_word.ptr), "d_out overlaps the words of a d_ptr operand"),
        "tables[0] reserved": (lambda: step(g(1, ONE), [V(None, 0, 7, 0)], R, 2, n, o), "operand tables[0]: reserved must be 0"),
        "tables[1] buf 2": (lambda: step(g(2, AB), [B0, V(None, 2, 0, 0)], R, 3, n, o), "operand tables[1]: buf must be 0 or 1"),
        "tables[1] buffer count": (lambda: step(g(2, AB), [B0, V(None, 1, 0, 8)], R, 3, n, o), "operand tables[1]: a transform buffer holds 256 elements, count says 8"),
        "tables[2] count 3": (lambda: step(g(3, AB), [B0, B1, V(words.ptr, 0, 0, 3)], R, 4, n, o), "operand tables[2]: count 3 is not a power of two"),
        "tables[2] count 0": (lambda: step(g(3, AB), [B0, B1, V(words.ptr, 0, 0, 0)], None, 4, n, o), "operand tables[2]: count 0 is not a power of two"),
        "tables[3] count 2n": (lambda: step(g(4, G2, 0), [B0, B1, W, V(big.ptr, 0, 0, 2 * n)], R, 4, n, o), "operand tables[3]: count 512 is not a power of two in [1, 256]"),
        "tables[3] in host memory": (lambda: step(g(4, G2, 0), [B0, B1, W, V(host_ptr, 0, 0, n)], None, 4, n, o), "operand tables[3]: d_ptr is not"),
        "tables[11] in host memory": (lambda: step(g(12, ONE), [B0] + [W] * 10 + [V(host_ptr, 0, 0, 1)], None, 2, n, o), "operand tables[11]: d_ptr is not"),
        "tables[0] misaligned": (lambda: step(g(1, ONE), [V(words.ptr + 8, 0, 0, 1)], None, 2, n, o), "operand tables[0]: d_ptr is not 16-byte aligned"),
        "tables[0] past its allocation": (lambda: step(g(1, ONE), [V(one_word.ptr, 0, 0, 2)], None, 2, n, o), "operand tables[0]: 2 elements run past the end"),
    }
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    with pytest.raises(DriverClientError) as ei:
        cl.sumcheck_gate([0, 0], AB, r=one_word)
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError):
        cl.sumcheck_gate([0, 1], [(1, [0, 1, 0, 1, 0])])   # five factors: the library's to refuse
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and bytes(words2.download()) == ab and _word(one_word) == 7 and bytes(out.download()) == mark
    # an op already in flight
    cl.vec_mle_round(0, words)
    assert step(g(1, ONE), [B0], R, 2, n, o) == 4 and "already running" in L.blz_last_error_message().decode()
    assert step(g(4, G2, 0), [B0, B1, W, W2], None, 4, n, o) == 4
    cl.wait_result()
    assert bytes(cl.result(0)) == ab and bytes(out.download()) == mark
    cl.close()
    for d in (words, words2, one_word, out, big):
        d.free()


def test_order_of_checks(gpu):
    """A call wrong in two ways reports the earlier check, in blz_ntt_sumcheck_step's order behind the description's own: the
    description, points, d_out, r's shape, the live length, len >= 4 for a bind with a round, an op in flight, the operands, then
    per table a periodic one, an overlap, r in the words it receives.  Checks that read the same argument cannot all meet in one
    call (points above 6 and points 0; points 0 and a NULL d_out with points): each is set against the nearest check it can meet."""
    field, logn = "BLS381", 3
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 83), _inputs(r, n, 84)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    words, big, one_word = _dev(bb), _dev(bytes(32 * 12)), _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 161))
    out, s = _dev(mark), DeviceBuffer(0, 128)   # 5 words; the op in flight's own
    V = BlzVecArg
    B0, B1, W, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    P4, BAD = V(words.ptr, 0, 0, 4), V(None, 2, 0, 0)
    # two tables that overlap in part, and r in the words the second receives but not in the first's
    LO, HI, R5 = V(big.ptr, 0, 0, 8), V(big.ptr + 32 * 4, 0, 0, 8), V(big.ptr + 32 * 5, 0, 0, 1)
    o = out.ptr
    ONE, AB = [(1, [0])], [(1, [0, 1])]
    g1, g2, g0 = make_gate(1, ONE, None), make_gate(2, AB, None), make_gate(2, AB, None)
    g0.ntables = 0

    def step(gate, tables, rr, points, length, d_out):
        return raw_gate(cl, gate, tables, rr, points, length, d_out)

    def good():
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); out.upload(mark)
        assert step(g2, [B0, B1], R, 3, n, o + 32) == 0, L.blz_last_error_message()
        cl.wait_result()
        fa, fb = fold_ref(a, r, 7, n), fold_ref(b, r, 7, n)
        assert bytes(cl.result(0)) == _pack(fa) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fb) + bb[16 * n:]
        assert bytes(out.download()) == mark[:32] + _pack(sum_gate_ref([fa, fb], AB, None, r, n // 2, 3)) + mark[128:]

    cases = [
        ("ntables, points", (lambda: step(g0, [B0, B1], R, 7, n, o), "gate: ntables 0 is not in [1, 12]", False), (lambda: step(g1, [B0], R, 7, n, o), "points 7 is not in [0, 6]", False)),
        ("points, null d_out", (lambda: step(g1, [B0], R, 7, n, None), "points 7 is not in [0, 6]", False), (lambda: step(g1, [B0], R, 3, n, None), "null d_out", False)),
        ("points 0, r", (lambda: step(g1, [B0], B1, 0, n, o), "points 0 is a bind alone", False), (lambda: step(g1, [B0], B1, 2, n, o), "r.d_ptr != NULL, r.count == 1", False)),
        ("null d_out, r", (lambda: step(g1, [B0], B1, 3, n, None), "null d_out", False), (lambda: step(g1, [B0], B1, 3, n, o), "r.d_ptr != NULL, r.count == 1", False)),
        ("r, len", (lambda: step(g1, [B0], B1, 2, 12, o), "r.d_ptr != NULL, r.count == 1", False), (lambda: step(g1, [B0], R, 2, 12, o), "len 12: the live length is 2^m", False)),
        ("len, len >= 4", (lambda: step(g1, [B0], R, 2, 3, o), "len 3: the live length is 2^m", False), (lambda: step(g1, [B0], R, 2, 2, o), "a bind and a round need len >= 4", False)),
        ("len >= 4, in flight", (lambda: step(g1, [B0], R, 2, 2, o), "a bind and a round need len >= 4", True), (lambda: step(g1, [B0], R, 2, n, o), "already running", True)),
        ("in flight, operand", (lambda: step(g1, [V(None, 0, 7, 0)], R, 2, n, o), "already running", True),
         (lambda: step(g1, [V(None, 0, 7, 0)], R, 2, n, o), "operand tables[0]: reserved must be 0", False)),
        ("operand, periodic", (lambda: step(g2, [P4, BAD], R, 3, 8, o), "operand tables[1]: buf must be 0 or 1", False),
         (lambda: step(g2, [P4, B1], R, 3, 8, o), "operand tables[0]: 4 words, read periodically over len 8", False)),
        ("periodic, overlap", (lambda: step(g2, [W, P4], R, 3, 8, o), "operand tables[1]: 4 words, read periodically over len 8", False),
         (lambda: step(g2, [W, W], R, 3, 8, o), "tables[0] and tables[1] overlap", False)),
        ("overlap, r in the words written", (lambda: step(g2, [LO, HI], R5, 3, 8, o), "tables[0] and tables[1] overlap", False),
         (lambda: step(g2, [B0, HI], R5, 3, 8, o), "r lies in the words tables[1] receives", False)),
    ]
    check_order_of_checks(cl, cases, lambda: cl.vec_mle_round(words, out=s), good)
    assert bytes(words.download()) == bb and bytes(big.download()) == bytes(32 * 12) and _word(one_word) == 7
    cl.close()
    for d in (words, big, one_word, out, s):
        d.free()


def test_in_flight_rules(gpu):
    """A gate step that writes BOTH buffers in flight: neither can be read, written or exchanged and nothing else starts.  A
    round alone writes none: both can be read, the ones it reads cannot be written.  reset drops the op."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c = (_inputs(r, n, 70 + i) for i in range(3))
    ab, bb, cb = _pack(a), _pack(b), _pack(c)
    cl = _client(field, logn)
    words, one_word = _dev(cb), _dev((7).to_bytes(32, "little"))
    host_out = bytearray(32 * n)
    terms = [(1, [0, 1]), (-1, [2, 2])]
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.vec_mle_round(words), lambda: cl.sumcheck_step([words]),
            lambda: cl.sumcheck_gate([words], [(1, [0])]), lambda: cl.sumcheck_gate([0, 1], [(1, [0, 1])], r=one_word),
            lambda: cl.sumcheck_gate([words], [(1, [0])], r=one_word, points=0))
    # the second buffer named is the second written buffer: 1 then 0, and 0 then 1
    for tabs, vals in (([1, 0, words], [b, a, c]), ([0, 1, words], [a, b, c])):
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb)
        out = cl.sumcheck_gate(tabs, terms, r=one_word)
        for attempt in busy + (lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
                               lambda: cl.exchange(0, ab, host_out), lambda: cl.exchange(1, ab, host_out)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        folded = [fold_ref(v, r, 7, n) for v in vals]
        assert bytes(out.download()) == _pack(sum_gate_ref(folded, terms, None, r, n // 2, 3))
        assert bytes(cl.result(0)) == _pack(fold_ref(a, r, 7, n)) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fold_ref(b, r, 7, n)) + bb[16 * n:]
        out.free()
    # a step on one buffer: the other one is free
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    out = cl.sumcheck_gate([1], [(1, [0, 0])], r=one_word)
    assert bytes(cl.result(0)) == ab
    cl.set_data(NTTInput(0, bb))
    for attempt in (lambda: cl.result(1), lambda: cl.set_data(NTTInput(1, ab))):
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(fold_ref(b, r, 7, n)) + bb[16 * n:] and bytes(cl.result(0)) == bb
    out.free()
    # a round alone over buffer 0 and device words: read-only, as for a reduce
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb)
    out = cl.sumcheck_gate([words, 0], [(1, [0, 1]), (-1, [1])], 0)
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(1, bb))   # not named
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(out.download()) == _pack(sum_gate_ref([c, a], [(1, [0, 1]), (-1, [1])], 0, r, n, 4))
    out.free()
    # reset with a gate step in flight: nothing is in flight afterwards, and the handle works
    for start in (lambda: cl.sumcheck_gate([0, 1], [(1, [0, 1])], r=one_word), lambda: cl.sumcheck_gate([0, 1, words], terms),
                  lambda: cl.sumcheck_gate([1, 0], [(1, [0])], r=one_word, points=0)):
        start()
        cl.reset()
        with pytest.raises(DriverClientError):
            cl.wait_result()
        cl.result(0); cl.result(1)
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    out = cl.sumcheck_gate([0, 1], [(1, [0, 1])], r=one_word)
    cl.wait_result()
    assert bytes(out.download()) == _pack(sum_gate_ref([fold_ref(a, r, 7, n), fold_ref(b, r, 7, n)], [(1, [0, 1])], None, r, n // 2, 3))
    cl.close()
    for d in (words, one_word, out):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_plonk_zerocheck_end_to_end(gpu, field):
    """A satisfied vanilla PLONK circuit of 2^10 rows: sum_p eq(p) (qL a + qR b + qM a b - qO c + qC)(p) = 0 in 12 ops - eq, a
    step without r, (a challenge uploaded as a device word, a step with r) x 9, a bind alone - over nine tables, a and b in the
    transform buffers.  What a verifier checks: every round's g(0) + g(1) is the running claim, 0 at first; the next claim is the
    degree-4 interpolation of the five points at the challenge; the last claim is G of the nine ten-times-bound words, which
    are the original tables at the challenges.  With one witness word flipped the first round's sum is not 0."""
    m = 10
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 190)
    qL, qR, qM, qC, a, b = ([rng.randrange(r) for _ in range(n)] for _ in range(6))
    qO = [rng.randrange(1, r) for _ in range(n)]
    c = [(qL[p] * a[p] + qR[p] * b[p] + qM[p] * a[p] * b[p] + qC[p]) * pow(qO[p], -1, r) % r for p in range(n)]
    tau = _words(len(field) + 191, m)
    cl = _client(field, m)
    point, d_eq = _dev(_pack(tau)), DeviceBuffer(0, 32 * n)
    cl.vec_mle_eq(d_eq, point); cl.wait_result()
    eq0 = _unpack(d_eq.download())
    orig = [eq0, qL, qR, qM, qO, qC, a, b, c]
    devs = [_dev(_pack(v)) for v in (qL, qR, qM, qO, qC, c)]
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    tabs = [d_eq] + devs[:5] + [0, 1, devs[5]]
    s_dev = DeviceBuffer(0, 32 * 5)
    claim, chal, dc = 0, [], None
    for rnd in range(m):
        length = n >> rnd   # the live length of this round's polynomial
        if rnd == 0:
            cl.sumcheck_gate(tabs, PLONK_TERMS, 0, length=length, out=s_dev)
        else:
            cl.sumcheck_gate(tabs, PLONK_TERMS, 0, r=dc, length=2 * length, out=s_dev)
        cl.wait_result()
        if dc is not None:
            dc.free()
        s = _unpack(s_dev.download())
        assert len(s) == 5 and (s[0] + s[1]) % r == claim, (rnd, "g(0) + g(1) = claim")
        x = rng.getrandbits(256)
        chal.append(x)
        dc = cl.scalar(x)
        claim = interpolate(s, x, r)
    assert cl.sumcheck_gate(tabs, PLONK_TERMS, 0, r=dc, points=0, length=2) is None
    cl.wait_result()
    finals = [_unpack(_bytes_of(cl, t)[:32])[0] for t in tabs]
    assert claim == gate_value(finals, PLONK_TERMS, 0, r)

    def at_challenges(table):
        for x in chal:
            h = len(table) // 2
            table = [(table[p] + x * (table[p + h] - table[p])) % r for p in range(h)]
        return table[0]

    assert finals == [at_challenges(t) for t in orig]
    # one witness word flipped: the circuit is not satisfied and the first round says so
    bad = list(c)
    bad[rng.randrange(n)] ^= 1
    devs[5].upload(_pack(bad))
    d_eq.upload(_pack(eq0))
    for t, v in zip(devs[:5], (qL, qR, qM, qO, qC)):
        t.upload(_pack(v))
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    cl.sumcheck_gate(tabs, PLONK_TERMS, 0, out=s_dev); cl.wait_result()
    s = _unpack(s_dev.download())
    assert (s[0] + s[1]) % r != 0
    cl.close()
    for d in devs + [point, d_eq, s_dev, dc]:
        d.free()
