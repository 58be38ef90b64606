"""The zerocheck step (blz_ntt_zerocheck_gate) on the device: the bind of every table in place, the weight summed in place and the
weighted round polynomial of a gate given as data; the round alone; the identity s(t) = c eq(tau_top, t) u(t) that ties it to
blz_ntt_sumcheck_gate with common = eq; a PLONK zerocheck driven through it; the refusals and the in-flight rules.  Every expected
value is Python integer arithmetic (tests/ntt_zerocheck_util.py) or, at 2^22, the existing step through the identity, and every
comparison of stored words is byte for byte: any 256-bit input word counts as its residue, every word written is canonical,
exactly len / 2 words of each table and len / 4 of the weight are written and no byte outside them - nor beside d_out - changes."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_gate_util import CATALOGUE, PLONK_TERMS, gate_inputs, gate_value, make_gate
from ntt_mle_util import challenges, check_order_of_checks, fill, fold_ref, interpolate
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, _client, _dev, _pack, _unpack, _word, _words
from ntt_zerocheck_util import PLONK8_TERMS, R1CS3_TERMS, eq1, raw_zerocheck, weight_step_ref, weighted_sum_gate_ref
from oracle import pyref

pytestmark = pytest.mark.gpu
# (log n, len) - the launcher's boundaries are blz_ntt_sumcheck_gate's: with r one quad; less than a block; 256 quads, exactly one
# block: d_out written directly; two blocks: workspace and finish; a live length below n.  Without r the items are pairs: len = 512
# is exactly one block, 1024 and 2048 take the workspace
SIZES = [(2, 4), (6, 64), (10, 1024), (11, 2048), (11, 512)]
MAXP = 6
R1CS_EQ = CATALOGUE["G2"]   # (4, eq (Az Bz - Cz)): the gate the existing step takes for the same zerocheck


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
    """Every catalogue gate (G2, G3 and G5 keep their common factor beside the weight) at points = 1 .. 6.  r walks through 0, 1,
    r - 1, r + 1 and a random word >= r from gate to gate; two of the tables sit in the transform buffers, the rest and the weight
    in device words.  The weight holds len / 2 known words - the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 among them - in a
    buffer of len / 2 or of n words by turns, random bytes behind."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    rs = challenges(r, logn)
    drs = [cl.scalar(v) for v in rs]
    words = [DeviceBuffer(0, 32 * n) for _ in range(12)]
    half, quarter = length // 2, length // 4
    wdev = [DeviceBuffer(0, 32 * half), DeviceBuffer(0, 32 * n)]
    guard = DeviceBuffer(0, 32 * (MAXP + 2))
    for turn, (name, (nt, terms, common)) in enumerate(CATALOGUE.items()):
        which = (turn + logn + len(field)) % 5
        rr, dr = rs[which], drs[which]
        vals = gate_inputs(r, nt, length, 7100 * logn + 100 * turn + len(field))
        before = [_pack(v) + fill(n - length, turn * 12 + j) for j, v in enumerate(vals)]
        buffers = [turn % nt, (turn + 3) % nt] if nt > 1 else ([0] if turn % 2 == 0 else [])
        wd = wdev[turn % 2]
        wv = _inputs(r, half, 7150 * logn + turn + len(field))
        wv = wv[turn % half:] + wv[:turn % half]
        wbefore = _pack(wv) + fill(wd.nbytes // 32 - half, turn + 77)
        folded = [fold_ref(v, r, rr, length) for v in vals]
        wnew = weight_step_ref(wv, r, length)
        want = weighted_sum_gate_ref(folded, wnew, terms, common, r, half, MAXP)
        gate = make_gate(nt, terms, common)
        for points in range(1, MAXP + 1):
            tabs = _place(cl, words, buffers, before)
            wd.upload(wbefore)
            gfill = fill(MAXP + 2, turn + 50 + points)
            guard.upload(gfill)
            assert raw_zerocheck(cl, gate, tabs, wd, dr, points, length, guard.ptr + 32) == 0, blaze_amd.lib().blz_last_error_message()
            cl.wait_result()
            assert cl.last_kernel_ms() > 0
            for j, t in enumerate(tabs):
                got = _bytes_of(cl, t)
                assert got[:32 * half] == _pack(folded[j]), (name, points, j, rr)
                assert got[32 * half:] == before[j][32 * half:], (name, points, j, "bytes behind the words written")
            got = bytes(wd.download())
            assert got[:32 * quarter] == _pack(wnew), (name, points, "the weight's sums")
            assert got[32 * quarter:] == wbefore[32 * quarter:], (name, points, "weight bytes behind the words written")
            assert bytes(guard.download()) == gfill[:32] + _pack(want[:points]) + gfill[32 * (1 + points):], (name, points, rr)
    cl.close()
    for d in drs + words + wdev + [guard]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_round_only(gpu, field, logn, length):
    """r = None: pairs in place of quads.  Every catalogue gate, and the eight-table PLONK gate with periodic selectors - qC one
    word, qM four -, under weights of len / 2 words, of n, and periodic ones of 1 and 4; each case at two point counts, 1 .. 6 all
    met.  No table byte and no weight byte changes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 12, n, 8100 * logn + len(field))
    raw = [_pack(v) for v in vals]
    words = [_dev(b) for b in raw[2:]]
    cl.set_data(NTTInput(0, raw[0]))
    cl.set_data(NTTInput(1, raw[1]))
    tabs = [0, 1] + words
    wvals = _inputs(r, n, 8150 * logn + len(field))
    wvals = wvals[3:] + wvals[:3]
    counts = sorted({length // 2, n, 1, min(4, n)})
    weights = {c: _dev(_pack(wvals[:c])) for c in counts}
    p1, p4 = _dev(raw[4][:32]), _dev(raw[2][:128])
    cases = [(name, tabs[:nt], vals[:nt], terms, common) for name, (nt, terms, common) in CATALOGUE.items()]
    per_t, per_v = list(tabs[:8]), list(vals[:8])
    per_t[4], per_v[4], per_t[2], per_v[2] = p1, vals[4][:1], p4, vals[2][:4]
    cases.append(("PLONK periodic", per_t, per_v, PLONK8_TERMS, None))
    mark = bytes(range(100, 132))
    for turn, (name, tt, vv, terms, common) in enumerate(cases):
        for k, points in enumerate((1 + turn % MAXP, 1 + (turn + 3) % MAXP)):
            count = counts[(turn + k) % len(counts)]
            want = weighted_sum_gate_ref(vv, wvals[:count], terms, common, r, length, points)
            out = _dev(fill(points, points) + mark)
            got = cl.zerocheck_gate(tt, terms, weights[count], common, points=points, length=length, out=out)
            cl.wait_result()
            assert got is out and bytes(out.download()) == _pack(want) + mark, (name, points, count)
            out.free()
    for count in counts:   # every weight shape under one gate, points by default: the degree + 1, nothing added for the weight
        out = cl.zerocheck_gate(tabs[:8], PLONK8_TERMS, weights[count], length=length)
        cl.wait_result()
        assert out.nbytes == 32 * 4
        assert bytes(out.download()) == _pack(weighted_sum_gate_ref(vals[:8], wvals[:count], PLONK8_TERMS, None, r, length, 4)), count
        out.free()
    for t, b in zip(tabs, raw):
        assert _bytes_of(cl, t) == b
    for count, w in weights.items():
        assert bytes(w.download()) == _pack(wvals[:count])
    assert bytes(p1.download()) == raw[4][:32] and bytes(p4.download()) == raw[2][:128]
    cl.close()
    for d in words + [p1, p4] + list(weights.values()):
        d.free()


def _identity(s, u, c, tau_top, r):
    """s(t) = c eq(tau_top, t) u(t) at every point of s; u, one point shorter, is extended by interpolation"""
    assert len(s) == len(u) + 1
    for t, st in enumerate(s):
        ut = u[t] if t < len(u) else interpolate(u, t, r)
        assert st == c * eq1(tau_top, t, r) * ut % r, t


@pytest.mark.parametrize("field", FIELDS)
def test_identity_with_the_existing_step(gpu, field):
    """E = vec_mle_eq(tau, m) drives blz_ntt_sumcheck_gate as the common factor, W = vec_mle_eq over tau's first m - 1 words drives
    the new op, on copies of the same tables: R1CS and PLONK at m = 10, the first round and a bound round, and R1CS at 2^12 with r
    (sixteen blocks of quads).  At every t, s(t) = c eq(tau_top, t) u(t); the folded tables are equal bytes; the summed weight is
    the equality table over one variable fewer."""
    r = pyref.CURVES[field]["r"]
    for m, gates in ((10, (("R1CS", 3, R1CS3_TERMS, R1CS_EQ[1]), ("PLONK", 8, PLONK8_TERMS, PLONK_TERMS))), (12, (("R1CS", 3, R1CS3_TERMS, R1CS_EQ[1]),))):
        n = 1 << m
        cl = _client(field, m)
        tau = _words(len(field) + 40 + m, m)
        point = _dev(_pack(tau))
        d_e, d_w, d_w2 = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * (n // 2)), DeviceBuffer(0, 32 * (n // 4))
        cl.vec_mle_eq(d_w2, point, m - 2); cl.wait_result()
        w2 = bytes(d_w2.download())
        x = _words(len(field) + 41 + m, 1)[0]
        dx = cl.scalar(x)
        for name, nt, terms, eq_terms in gates:
            deg = max(len(f) for _, f in terms)
            raw = [_pack(_inputs(r, n, 9600 + 10 * m + j + len(field))) for j in range(nt)]
            cl.vec_mle_eq(d_e, point); cl.wait_result()
            cl.vec_mle_eq(d_w, point, m - 1); cl.wait_result()
            # the existing step: tables in device words behind eq
            old = [_dev(b) for b in raw]
            new = [_dev(b) for b in raw[2:]]
            cl.set_data(NTTInput(0, raw[0])); cl.set_data(NTTInput(1, raw[1]))
            tabs = [0, 1] + new
            if m == 10:
                s = cl.sumcheck_gate([d_e] + old, eq_terms, 0); cl.wait_result()
                u = cl.zerocheck_gate(tabs, terms, d_w); cl.wait_result()
                assert s.nbytes == 32 * (deg + 2) and u.nbytes == 32 * (deg + 1)
                _identity(_unpack(s.download()), _unpack(u.download()), 1, tau[m - 1], r)
                s.free(); u.free()
            s = cl.sumcheck_gate([d_e] + old, eq_terms, 0, r=dx); cl.wait_result()
            u = cl.zerocheck_gate(tabs, terms, d_w, r=dx); cl.wait_result()
            _identity(_unpack(s.download()), _unpack(u.download()), eq1(tau[m - 1], x, r), tau[m - 2], r)
            for t, o, b in zip(tabs, old, raw):
                got = _bytes_of(cl, t)
                assert got == bytes(o.download()) and got[16 * n:] == b[16 * n:], name
            assert bytes(d_w.download())[:8 * n] == w2, name
            for d in old + new + [s, u]:
                d.free()
        cl.close()
        for d in (point, d_e, d_w, d_w2, dx):
            d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_plonk_zerocheck_end_to_end(gpu, field):
    """The satisfied 2^10-row PLONK circuit of tests/test_gpu_ntt_sumcheck_gate.py through the new op: eight tables, no eq table,
    4 points a round.  The host rebuilds s_i(t) = c_i eq(tau_{m-1-i}, t) u_i(t) at five points (u_i extended by interpolation):
    s_i(0) + s_i(1) is the running claim, 0 at first; the next claim is s_i at the challenge; the last claim is c_m G of the eight
    ten-times-bound words, which are the original tables at the challenges.  One flipped witness word makes round 0's sum
    nonzero."""
    m = 10
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 290)
    qL, qR, qM, qC, a, b = ([rng.randrange(r) for _ in range(n)] for _ in range(6))
    qO = [rng.randrange(1, r) for _ in range(n)]
    c = [(qL[p] * a[p] + qR[p] * b[p] + qM[p] * a[p] * b[p] + qC[p]) * pow(qO[p], -1, r) % r for p in range(n)]
    tau = _words(len(field) + 291, m)
    cl = _client(field, m)
    point, d_w = _dev(_pack(tau)), DeviceBuffer(0, 32 * (n // 2))
    cl.vec_mle_eq(d_w, point, m - 1); cl.wait_result()
    w0 = bytes(d_w.download())
    orig = [qL, qR, qM, qO, qC, a, b, c]
    devs = [_dev(_pack(v)) for v in (qL, qR, qM, qO, qC, c)]
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    tabs = devs[:5] + [0, 1, devs[5]]
    u_dev = DeviceBuffer(0, 32 * 4)

    def rebuilt(u, coef, top):
        return [coef * eq1(top, t, r) * (u[t] if t < 4 else interpolate(u, t, r)) % r for t in range(5)]

    claim, coef, chal, dc = 0, 1, [], None
    for rnd in range(m):
        length = n >> rnd   # the live length of this round's polynomial
        if rnd == 0:
            cl.zerocheck_gate(tabs, PLONK8_TERMS, d_w, length=length, out=u_dev)
        else:
            cl.zerocheck_gate(tabs, PLONK8_TERMS, d_w, r=dc, length=2 * length, out=u_dev)
        cl.wait_result()
        if dc is not None:
            dc.free()
        u = _unpack(u_dev.download())
        assert len(u) == 4
        s = rebuilt(u, coef, tau[m - 1 - rnd])
        assert (s[0] + s[1]) % r == claim, (rnd, "s(0) + s(1) = claim")
        x = rng.getrandbits(256)
        chal.append(x)
        dc = cl.scalar(x)
        claim = interpolate(s, x, r)
        coef = coef * eq1(tau[m - 1 - rnd], x, r) % r
    assert cl.sumcheck_gate(tabs, PLONK8_TERMS, None, r=dc, points=0, length=2) is None
    cl.wait_result()
    finals = [_unpack(_bytes_of(cl, t)[:32])[0] for t in tabs]
    assert claim == coef * gate_value(finals, PLONK8_TERMS, None, r) % r

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
    d_w.upload(w0)
    for t, v in zip(devs[:5], (qL, qR, qM, qO, qC)):
        t.upload(_pack(v))
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    cl.zerocheck_gate(tabs, PLONK8_TERMS, d_w, out=u_dev); cl.wait_result()
    s = rebuilt(_unpack(u_dev.download()), 1, tau[m - 1])
    assert (s[0] + s[1]) % r != 0
    cl.close()
    for d in devs + [point, d_w, u_dev, dc]:
        d.free()


def test_second_sweep_of_the_grid_stride_loop(gpu):
    """BLS12-381, len = n = 2^22 with r: 2^20 quads are two sweeps of the 2048 x 256 grid.  W (Az Bz - Cz) over both buffers and one
    device-word table against eq (Az Bz - Cz) through blz_ntt_sumcheck_gate on the same bytes, by the identity; the folded tables
    are equal bytes, and 32 sampled weight and table words are checked against Python integers."""
    field, m = "BLS381", 22
    n = 1 << m
    half, quarter = n // 2, n // 4
    r = pyref.CURVES[field]["r"]
    raw = [random.Random(2400 + j).randbytes(32 * n) for j in range(3)]
    tau = _words(2410, m)
    rr = _words(2404, 1)[0]
    cl = _client(field, m)
    dr, point = cl.scalar(rr), _dev(_pack(tau))
    d_e, d_w, cz = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * half), DeviceBuffer(0, 32 * n)
    tabs = [0, 1, cz]

    def load():
        cl.set_data(NTTInput(0, raw[0])); cl.set_data(NTTInput(1, raw[1])); cz.upload(raw[2])

    load()
    cl.vec_mle_eq(d_e, point); cl.wait_result()
    s = cl.sumcheck_gate([d_e] + tabs, R1CS_EQ[1], 0, r=dr)
    cl.wait_result()
    want_tabs = [_bytes_of(cl, t) for t in tabs]
    load()
    cl.vec_mle_eq(d_w, point, m - 1); cl.wait_result()
    w0 = bytes(d_w.download())
    u = cl.zerocheck_gate(tabs, R1CS3_TERMS, d_w, r=dr)
    cl.wait_result()
    assert s.nbytes == 128 and u.nbytes == 96
    _identity(_unpack(s.download()), _unpack(u.download()), eq1(tau[m - 1], rr, r), tau[m - 2], r)
    rng = random.Random(2405)
    sample = [0, quarter - 1] + [rng.randrange(quarter) for _ in range(30)]
    w1 = bytes(d_w.download())
    assert w1[32 * quarter:] == w0[32 * quarter:]
    for q in sample:
        lo, hi = (int.from_bytes(w0[32 * p: 32 * p + 32], "little") for p in (q, q + quarter))
        assert w1[32 * q: 32 * q + 32] == ((lo + hi) % r).to_bytes(32, "little"), q
    for t, e, src in zip(tabs, want_tabs, raw):
        got = _bytes_of(cl, t)
        assert got == e and got[32 * half:] == src[32 * half:]
        for p in [2 * q for q in sample]:
            lo, hi = (int.from_bytes(src[32 * q: 32 * q + 32], "little") for q in (p, p + half))
            assert got[32 * p: 32 * p + 32] == ((lo + rr * (hi - lo)) % r).to_bytes(32, "little"), p
    cl.close()
    for d in (dr, point, d_e, d_w, cz, s, u):
        d.free()


def test_refusals(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM (InvalidPrimitiveParam) with a message that names the cause, and leaves the
    tables, the weight, d_out and the in-flight state as they were: the new ones, and a sample of blz_ntt_sumcheck_gate's."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b, w = _inputs(r, n, 61), _inputs(r, n, 62), _inputs(r, n, 63)
    ab, bb, wb = _pack(a), _pack(b), _pack(w)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words, weight = _dev(bb), _dev(wb)
    one_word = _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 225))
    out = _dev(mark)           # 7 words
    big = _dev(bytes(64 * n))  # 2n words
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    B0, B1, T, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    WT, W4, P4 = V(weight.ptr, 0, 0, n), V(weight.ptr, 0, 0, 4), V(words.ptr, 0, 0, 4)
    o = out.ptr
    ONE, AB = [(1, [0])], [(1, [0, 1])]

    def step(gate, tables, wt, rr, points, length, d_out):
        return raw_zerocheck(cl, gate, tables, wt, rr, points, length, d_out)

    def g(nt, terms, common=None, **kw):
        return make_gate(nt, terms, common, **kw)

    bad_terms = g(2, AB)
    bad_terms.nterms = 9
    assert L.blz_ntt_zerocheck_gate(None, None, None, None, None, 77, 3, None) == 4 and b"null handle" in L.blz_last_error_message()
    assert L.blz_ntt_zerocheck_gate(None, C.byref(bad_terms), None, C.byref(B1), C.byref(B0), 0, 12, o + 8) == 4 and b"null handle" in L.blz_last_error_message()
    refused = {
        # the new ones
        "null gate": (lambda: step(None, [B0], WT, R, 2, n, o), "gate is NULL"),
        "null tables": (lambda: step(g(1, ONE), None, WT, R, 2, n, o), "tables is NULL"),
        "null weight": (lambda: step(g(1, ONE), [B0], None, R, 2, n, o), "weight is NULL"),
        "points 0": (lambda: step(g(1, ONE), [B0], WT, R, 0, n, None), "blz_ntt_sumcheck_gate"),
        "points 0, round only": (lambda: step(g(1, ONE), [B0], WT, None, 0, n, o), "points 0: a zerocheck step takes a round"),
        "weight names a buffer": (lambda: step(g(1, ONE), [B0], B1, R, 2, n, o), "operand weight: the weight is device words"),
        "weight names a buffer, round only": (lambda: step(g(1, ONE), [B0], V(None, 1, 0, 0), None, 2, n, o), "operand weight: the weight is device words"),
        "weight reserved": (lambda: step(g(1, ONE), [B0], V(weight.ptr, 0, 7, n), R, 2, n, o), "operand weight: reserved must be 0"),
        "weight count 3": (lambda: step(g(1, ONE), [B0], V(weight.ptr, 0, 0, 3), None, 2, n, o), "operand weight: count 3 is not a power of two"),
        "weight count 0": (lambda: step(g(1, ONE), [B0], V(weight.ptr, 0, 0, 0), None, 2, n, o), "operand weight: count 0 is not a power of two"),
        "weight count 2n": (lambda: step(g(1, ONE), [B0], V(big.ptr, 0, 0, 2 * n), R, 2, n, o), "operand weight: count 512 is not a power of two in [1, 256]"),
        "weight in host memory": (lambda: step(g(1, ONE), [B0], V(host_ptr, 0, 0, n), None, 2, n, o), "operand weight: d_ptr is not"),
        "weight misaligned": (lambda: step(g(1, ONE), [B0], V(weight.ptr + 8, 0, 0, 1), None, 2, n, o), "operand weight: d_ptr is not 16-byte aligned"),
        "weight past its allocation": (lambda: step(g(1, ONE), [B0], V(one_word.ptr, 0, 0, 2), None, 2, n, o), "operand weight: 2 elements run past the end"),
        "weight below len / 2 with r": (lambda: step(g(1, ONE), [B0], V(weight.ptr, 0, 0, n // 4), R, 2, n, o), "operand weight: 64 words, a step with r sums len / 2 = 128"),
        "periodic weight with r": (lambda: step(g(2, AB), [B0, B1], W4, R, 3, 16, o), "operand weight: 4 words, a step with r sums len / 2 = 8"),
        "weight on a table": (lambda: step(g(2, AB), [B0, T], V(words.ptr, 0, 0, n), R, 3, n, o), "the weight's first len / 2 words meet the first len words of tables[1]"),
        "weight on a table's live words, in part": (lambda: step(g(1, ONE), [T], V(words.ptr + 32 * 4, 0, 0, 4), R, 2, 8, o), "the weight's first len / 2 words meet the first len words of tables[0]"),
        "r in the weight words written": (lambda: step(g(1, ONE), [B0], WT, V(weight.ptr + 32, 0, 0, 1), 2, 8, o), "r lies in the words the weight receives"),
        "d_out in the weight words read": (lambda: step(g(1, ONE), [B0], WT, R, 2, 8, weight.ptr + 32 * 3), "d_out overlaps the words of a d_ptr operand"),
        "d_out on the weight, round only": (lambda: step(g(1, ONE), [B0], WT, None, 2, n, weight.ptr + 32 * (n - 2)), "d_out overlaps the words of a d_ptr operand"),
        "d_out on a periodic weight": (lambda: step(g(1, ONE), [B0], W4, None, 3, n, weight.ptr + 32), "d_out overlaps the words of a d_ptr operand"),
        # blz_ntt_sumcheck_gate's, a sample
        "ntables 0": (lambda: step(g(0, ONE), [B0], WT, R, 2, n, o), "ntables 0 is not in [1, 12]"),
        "nterms 9": (lambda: step(bad_terms, [B0, B1], WT, R, 3, n, o), "nterms 9 is not in [1, 8]"),
        "a factor at ntables": (lambda: step(g(2, [(1, [0, 2])]), [B0, B1], WT, R, 3, n, o), "term 0: factor 1 names table 2, ntables is 2"),
        "common at ntables": (lambda: step(g(2, AB, 2), [B0, B1], WT, R, 3, n, o), "common 2 is neither -1 nor a table index"),
        "gate reserved": (lambda: step(g(2, AB, reserved=1), [B0, B1], WT, R, 3, n, o), "gate: reserved must be 0"),
        "points 7": (lambda: step(g(1, ONE), [B0], WT, R, 7, n, o), "points 7 is not in [0, 6]"),
        "null d_out": (lambda: step(g(2, AB), [B0, B1], WT, R, 3, n, None), "null d_out"),
        "null d_out, round only": (lambda: step(g(2, AB), [B0, B1], WT, None, 3, n, None), "null d_out"),
        "r names a buffer": (lambda: step(g(1, ONE), [B0], WT, B1, 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "r of two words": (lambda: step(g(1, ONE), [B0], WT, V(words.ptr, 0, 0, 2), 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "len 12": (lambda: step(g(1, ONE), [B0], WT, R, 2, 12, o), "len 12: the live length is 2^m"),
        "len 2n": (lambda: step(g(1, ONE), [B0], WT, R, 2, 2 * n, o), "len 512: the live length is 2^m"),
        "len 1": (lambda: step(g(1, ONE), [B0], WT, None, 2, 1, o), "len 1: the live length is 2^m"),
        "len 2 with r": (lambda: step(g(1, ONE), [B0], WT, R, 2, 2, o), "a bind and a round need len >= 4"),
        "periodic table with r": (lambda: step(g(2, AB), [B0, P4], WT, R, 3, 8, o), "operand tables[1]: 4 words, read periodically over len 8"),
        "the same buffer twice": (lambda: step(g(2, AB), [B0, B0], WT, R, 3, n, o), "tables[0] and tables[1] overlap"),
        "r in the words a table receives": (lambda: step(g(1, ONE), [T], WT, V(words.ptr + 32 * 3, 0, 0, 1), 2, 8, o), "r lies in the words tables[0] receives"),
        "d_out on a table": (lambda: step(g(2, AB), [B0, T], WT, R, 3, n, words.ptr + 32 * (n - 3)), "d_out overlaps the words of a d_ptr operand"),
        "d_out misaligned": (lambda: step(g(1, ONE), [B0], WT, R, 2, n, o + 8), "operand d_out: d_ptr is not 16-byte aligned"),
        "tables[1] buf 2": (lambda: step(g(2, AB), [B0, V(None, 2, 0, 0)], WT, R, 3, n, o), "operand tables[1]: buf must be 0 or 1"),
        "r in host memory": (lambda: step(g(1, ONE), [B0], WT, V(host_ptr, 0, 0, 1), 2, n, o), "operand r: d_ptr is not"),
    }
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    with pytest.raises(DriverClientError) as ei:
        cl.zerocheck_gate([0, 1], AB, weight, r=one_word, points=0)
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError):
        cl.zerocheck_gate([0, 1], AB, 1)   # a transform buffer as the weight
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and bytes(weight.download()) == wb and _word(one_word) == 7 and bytes(out.download()) == mark
    # an op already in flight
    cl.vec_mle_round(0, words)
    assert step(g(1, ONE), [B0], WT, R, 2, n, o) == 4 and "already running" in L.blz_last_error_message().decode()
    assert step(g(2, AB), [B0, B1], WT, None, 3, n, o) == 4
    cl.wait_result()
    assert bytes(cl.result(0)) == ab and bytes(weight.download()) == wb and bytes(out.download()) == mark
    cl.close()
    for d in (words, weight, one_word, out, big):
        d.free()


def test_order_of_checks(gpu):
    """A call wrong in two ways reports the earlier check: the description, points == 0, a weight that names a buffer, then
    blz_ntt_sumcheck_gate's order - points, d_out, r's shape, the live length, len >= 4, an op in flight, the operands (tables, r,
    the weight, d_out), per table a periodic one, an overlap, r in the words it receives - and the weight's own rules last: its
    count, its meeting a table, r in the words it receives."""
    field, logn = "BLS381", 3
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b, w = _inputs(r, n, 83), _inputs(r, n, 84), _inputs(r, n, 85)
    ab, bb, wb = _pack(a), _pack(b), _pack(w)
    cl = _client(field, logn)
    words, weight, one_word = _dev(bb), _dev(wb), _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 161))
    out, s = _dev(mark), DeviceBuffer(0, 128)   # 5 words; the op in flight's own
    V = BlzVecArg
    B0, B1, T, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    WT, W2, P4, BAD = V(weight.ptr, 0, 0, n), V(weight.ptr, 0, 0, 2), V(words.ptr, 0, 0, 4), V(None, 2, 0, 0)
    RW = V(weight.ptr + 32, 0, 0, 1)      # r in the weight words a step at len 8 writes
    RT = V(words.ptr + 32 * 3, 0, 0, 1)   # r in the words table T receives at len 8
    o = out.ptr
    ONE, AB = [(1, [0])], [(1, [0, 1])]
    g1, g2, g0 = make_gate(1, ONE, None), make_gate(2, AB, None), make_gate(2, AB, None)
    g0.ntables = 0

    def step(gate, tables, wt, rr, points, length, d_out):
        return raw_zerocheck(cl, gate, tables, wt, rr, points, length, d_out)

    def good():
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); out.upload(mark); weight.upload(wb)
        assert step(g2, [B0, B1], WT, R, 3, n, o + 32) == 0, L.blz_last_error_message()
        cl.wait_result()
        fa, fb, wn = fold_ref(a, r, 7, n), fold_ref(b, r, 7, n), weight_step_ref(w, r, n)
        assert bytes(cl.result(0)) == _pack(fa) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fb) + bb[16 * n:]
        assert bytes(weight.download()) == _pack(wn) + wb[8 * n:]
        assert bytes(out.download()) == mark[:32] + _pack(weighted_sum_gate_ref([fa, fb], wn, AB, None, r, n // 2, 3)) + mark[128:]

    cases = [
        ("ntables, points 0", (lambda: step(g0, [B0, B1], WT, R, 0, n, None), "gate: ntables 0 is not in [1, 12]", False),
         (lambda: step(g1, [B0], WT, R, 0, n, None), "points 0: a zerocheck step takes a round", False)),
        ("points 0, weight names a buffer", (lambda: step(g1, [B0], B1, R, 0, n, None), "points 0: a zerocheck step takes a round", False),
         (lambda: step(g1, [B0], B1, R, 2, n, o), "operand weight: the weight is device words", False)),
        ("weight names a buffer, points 7", (lambda: step(g1, [B0], B1, R, 7, n, o), "operand weight: the weight is device words", False),
         (lambda: step(g1, [B0], WT, R, 7, n, o), "points 7 is not in [0, 6]", False)),
        ("points, null d_out", (lambda: step(g1, [B0], WT, R, 7, n, None), "points 7 is not in [0, 6]", False), (lambda: step(g1, [B0], WT, R, 3, n, None), "null d_out", False)),
        ("null d_out, r", (lambda: step(g1, [B0], WT, B1, 3, n, None), "null d_out", False), (lambda: step(g1, [B0], WT, B1, 3, n, o), "r.d_ptr != NULL, r.count == 1", False)),
        ("r, len", (lambda: step(g1, [B0], WT, B1, 2, 12, o), "r.d_ptr != NULL, r.count == 1", False), (lambda: step(g1, [B0], WT, R, 2, 12, o), "len 12: the live length is 2^m", False)),
        ("len, len >= 4", (lambda: step(g1, [B0], WT, R, 2, 3, o), "len 3: the live length is 2^m", False), (lambda: step(g1, [B0], WT, R, 2, 2, o), "a bind and a round need len >= 4", False)),
        ("len >= 4, in flight", (lambda: step(g1, [B0], WT, R, 2, 2, o), "a bind and a round need len >= 4", True), (lambda: step(g1, [B0], WT, R, 2, n, o), "already running", True)),
        ("in flight, weight operand", (lambda: step(g1, [B0], V(weight.ptr, 0, 7, n), R, 2, n, o), "already running", True),
         (lambda: step(g1, [B0], V(weight.ptr, 0, 7, n), R, 2, n, o), "operand weight: reserved must be 0", False)),
        ("table operand, weight operand", (lambda: step(g2, [B0, BAD], V(weight.ptr, 0, 0, 3), R, 3, n, o), "operand tables[1]: buf must be 0 or 1", False),
         (lambda: step(g2, [B0, B1], V(weight.ptr, 0, 0, 3), R, 3, n, o), "operand weight: count 3 is not a power of two", False)),
        ("weight operand, d_out", (lambda: step(g1, [B0], V(weight.ptr, 0, 0, 3), R, 2, n, o + 8), "operand weight: count 3 is not a power of two", False),
         (lambda: step(g1, [B0], WT, R, 2, n, o + 8), "operand d_out: d_ptr is not 16-byte aligned", False)),
        ("d_out on the weight, periodic table", (lambda: step(g2, [B0, P4], WT, R, 3, 8, weight.ptr + 32 * 5), "d_out overlaps the words of a d_ptr operand", False),
         (lambda: step(g2, [B0, P4], WT, R, 3, 8, o), "operand tables[1]: 4 words, read periodically over len 8", False)),
        ("periodic table, weight count", (lambda: step(g2, [B0, P4], W2, R, 3, 8, o), "operand tables[1]: 4 words, read periodically over len 8", False),
         (lambda: step(g2, [B0, B1], W2, R, 3, 8, o), "operand weight: 2 words, a step with r sums len / 2 = 4", False)),
        ("overlapping tables, weight on a table", (lambda: step(g2, [T, T], V(words.ptr, 0, 0, n), R, 3, 8, o), "tables[0] and tables[1] overlap", False),
         (lambda: step(g2, [B0, T], V(words.ptr, 0, 0, n), R, 3, 8, o), "the weight's first len / 2 words meet the first len words of tables[1]", False)),
        ("r in a table's words, weight count", (lambda: step(g1, [T], W2, RT, 2, 8, o), "r lies in the words tables[0] receives", False),
         (lambda: step(g1, [B0], W2, R, 2, 8, o), "operand weight: 2 words, a step with r sums len / 2 = 4", False)),
        ("weight count, r in the weight's words", (lambda: step(g1, [B0], W2, RW, 2, 8, o), "operand weight: 2 words, a step with r sums len / 2 = 4", False),
         (lambda: step(g1, [B0], WT, RW, 2, 8, o), "r lies in the words the weight receives", False)),
    ]
    check_order_of_checks(cl, cases, lambda: cl.vec_mle_round(words, out=s), good)
    assert bytes(words.download()) == bb and _word(one_word) == 7
    cl.close()
    for d in (words, weight, one_word, out, s):
        d.free()


def test_in_flight_rules(gpu):
    """A zerocheck step that writes BOTH buffers in flight: neither can be read, written or exchanged and nothing else starts.  A
    round alone writes none: both can be read, the one it reads cannot be written.  reset drops the step."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c, w = (_inputs(r, n, 170 + i) for i in range(4))
    ab, bb, cb, wb = _pack(a), _pack(b), _pack(c), _pack(w[:n // 2])
    cl = _client(field, logn)
    words, weight, one_word = _dev(cb), _dev(wb), _dev((7).to_bytes(32, "little"))
    host_out = bytearray(32 * n)
    terms = [(1, [0, 1]), (-1, [2, 2])]
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.vec_mle_round(words), lambda: cl.sumcheck_step([words]),
            lambda: cl.sumcheck_gate([words], [(1, [0])]), lambda: cl.zerocheck_gate([words], [(1, [0])], weight),
            lambda: cl.zerocheck_gate([0, 1], [(1, [0, 1])], weight, r=one_word), lambda: cl.sumcheck_gate([words], [(1, [0])], r=one_word, points=0))
    for tabs, vals in (([1, 0, words], [b, a, c]), ([0, 1, words], [a, b, c])):
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb); weight.upload(wb)
        out = cl.zerocheck_gate(tabs, terms, weight, r=one_word)
        for attempt in busy + (lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
                               lambda: cl.exchange(0, ab, host_out), lambda: cl.exchange(1, ab, host_out)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        folded, wn = [fold_ref(v, r, 7, n) for v in vals], weight_step_ref(w, r, n)
        assert out.nbytes == 96 and bytes(out.download()) == _pack(weighted_sum_gate_ref(folded, wn, terms, None, r, n // 2, 3))
        assert bytes(cl.result(0)) == _pack(fold_ref(a, r, 7, n)) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fold_ref(b, r, 7, n)) + bb[16 * n:]
        assert bytes(weight.download()) == _pack(wn) + wb[8 * n:]
        out.free()
    # a round alone over buffer 0 and device words: read-only, as for a reduce
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb); weight.upload(wb)
    out = cl.zerocheck_gate([words, 0], [(1, [0, 1]), (-1, [1])], weight)
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(1, bb))   # not named
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(out.download()) == _pack(weighted_sum_gate_ref([c, a], w[:n // 2], [(1, [0, 1]), (-1, [1])], None, r, n, 3))
    assert bytes(weight.download()) == wb
    out.free()
    # reset with a zerocheck step in flight: nothing is in flight afterwards, and the handle works
    for start in (lambda: cl.zerocheck_gate([0, 1], [(1, [0, 1])], weight, r=one_word), lambda: cl.zerocheck_gate([0, 1, words], terms, weight)):
        start()
        cl.reset()
        with pytest.raises(DriverClientError):
            cl.wait_result()
        cl.result(0); cl.result(1)
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); weight.upload(wb)
    out = cl.zerocheck_gate([0, 1], [(1, [0, 1])], weight, r=one_word)
    cl.wait_result()
    assert bytes(out.download()) == _pack(weighted_sum_gate_ref([fold_ref(a, r, 7, n), fold_ref(b, r, 7, n)], weight_step_ref(w, r, n), [(1, [0, 1])], None, r, n // 2, 3))
    cl.close()
    for d in (words, weight, one_word, out):
        d.free()
