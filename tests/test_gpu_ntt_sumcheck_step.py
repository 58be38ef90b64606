"""The fused sumcheck step (blz_ntt_sumcheck_step) on the device: bind the top variable of every table in place and take the next
round polynomial of the gate in the same pass; the round alone; the bind alone; and a whole sumcheck for
sum eq (Az o Bz - Cz) = 0 driven through it.  Every expected value is Python integer arithmetic (or, at 2^22, the existing
unfused ops) and every comparison is byte for byte: any 256-bit input word counts as its residue, every word written is
canonical, exactly len / 2 words of each table are written and no byte outside them - nor beside d_out - changes.  The input
recipe is the house one (tests/ntt_vec_util.py): the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random 256-bit
words behind."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_mle_util import challenges, check_order_of_checks, fill, fold_ref, interpolate
from ntt_spmv_util import _inputs, _u32, sparse_rows, spmv_ref
from ntt_vec_util import FIELDS, _client, _dev, _pack, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
PRODUCT, R1CS = NTTClient.GATE_PRODUCT, NTTClient.GATE_R1CS
GATES = [(PRODUCT, 1), (PRODUCT, 2), (PRODUCT, 3), (R1CS, 4)]
# (log n, len): one quad; less than a block; 256 quads, exactly one block: d_out written directly; two blocks: workspace and
# finish; a live length below n
SIZES = [(2, 4), (6, 64), (10, 1024), (11, 2048), (11, 512)]


def gate_ref(tables, r, length, points, gate):
    """out[t] = sum over the pairs (T[p], T[p + length / 2]) of the gate at lo + t (hi - lo); tables are read periodically"""
    half = length // 2
    out = []
    for t in range(points):
        s = 0
        for p in range(half):
            v = [a[p % len(a)] + t * (a[(p + half) % len(a)] - a[p % len(a)]) for a in tables]
            if gate == R1CS:
                s += v[0] * (v[1] * v[2] - v[3])
            else:
                term = 1
                for x in v:
                    term = term * x % r
                s += term
        out.append(s % r)
    return out


def _ref(v):
    return None if v is None else C.byref(v)


def _raw_step(cl, gate, tables, r, points, length, d_out):
    """The C entry point itself: tables are ints (buffers) / DeviceBuffers, d_out an address"""
    args = [cl._vec_arg(x) for x in list(tables) + [None] * (4 - len(tables)) + [r]]
    return blaze_amd.lib().blz_ntt_sumcheck_step(cl._h, gate, *[_ref(v) for v in args], points, length, d_out)


# where the k tables of a call live: 0 / 1 the transform buffers, "w" device words of n words
PLACES = {1: [(0,), ("w",), (1,)], 2: [(0, 1), ("w", "w"), ("w", 0)], 3: [(1, "w", 0), ("w", "w", "w"), (0, "w", "w")],
          4: [(0, 1, "w", "w"), ("w", "w", "w", "w"), ("w", 1, "w", 0)]}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_bind_and_round_against_python_integers(gpu, field, logn, length):
    """Both gates at every k x points = 1 .. 4; r walks through 0, 1, r - 1, r + 1 and a random word >= r; the tables sit in both
    buffers, in device words, and mixed.  Before each call every table holds `length` known words with random bytes behind them."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    rs = challenges(r, logn)
    drs = [cl.scalar(v) for v in rs]
    words = [DeviceBuffer(0, 32 * n) for _ in range(4)]
    guard = DeviceBuffer(0, 32 * 6)
    half, turn = length // 2, 0
    for gate, k in GATES:
        for points in (1, 2, 3, 4):
            places = PLACES[k][turn % 3]
            rr, dr = rs[turn % 5], drs[turn % 5]
            vals = [_inputs(r, length, 7000 * logn + 100 * turn + 10 * j + len(field)) for j in range(k)]
            if turn % 2:   # the edge words against each other, not only against themselves
                vals = [v[j:] + v[:j] for j, v in enumerate(vals)]
            before, tabs, w = [], [], 0
            for j, place in enumerate(places):
                b = _pack(vals[j]) + fill(n - length, turn * 4 + j)
                before.append(b)
                if place == "w":
                    words[w].upload(b)
                    tabs.append(words[w])
                    w += 1
                else:
                    cl.set_data(NTTInput(place, b))
                    tabs.append(place)
            gfill = fill(6, turn + 50)
            guard.upload(gfill)
            assert _raw_step(cl, gate, tabs, dr, points, length, guard.ptr + 32) == 0, blaze_amd.lib().blz_last_error_message()
            cl.wait_result()
            assert cl.last_kernel_ms() > 0
            folded = [fold_ref(v, r, rr, length) for v in vals]
            for j, t in enumerate(tabs):
                got = bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))
                assert got[:32 * half] == _pack(folded[j]), (gate, k, points, places, j, rr)
                assert got[32 * half:] == before[j][32 * half:], (gate, k, points, places, j, "bytes behind the words written")
            want = gate_ref(folded, r, half, points, gate)
            assert bytes(guard.download()) == gfill[:32] + _pack(want) + gfill[32 * (1 + points):], (gate, k, points, places, rr)
            turn += 1
    assert turn == 16
    cl.close()
    for d in drs + words + [guard]:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_round_only(gpu, field, logn, length):
    """r = None: the R1CS round at points 1 .. 4 over buffers, device words and periodic tables of 1 and of 4 words (len / 2 pairs:
    one block up to len = 512, workspace and finish above), and PRODUCT, which is vec_mle_round.  No table changes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    t = [_inputs(r, n, 8000 * logn + j + len(field)) for j in range(4)]
    t = [v[j:] + v[:j] for j, v in enumerate(t)]
    cl.set_data(NTTInput(0, _pack(t[0])))
    cl.set_data(NTTInput(1, _pack(t[1])))
    w2, w3 = _dev(_pack(t[2])), _dev(_pack(t[3]))
    p1, p4 = _dev(_pack(t[2][:1])), _dev(_pack(t[3][:4]))
    tab = {"b0": (0, t[0]), "b1": (1, t[1]), "w2": (w2, t[2]), "w3": (w3, t[3]), "p1": (p1, t[2][:1]), "p4": (p4, t[3][:4])}
    combos = [("w3", "b0", "b1", "w2"), ("p4", "b0", "b1", "p1"), ("b0", "p1", "p4", "b1"), ("b1", "b1", "p1", "w2")]
    guard = bytes(range(100, 132))
    for points in (1, 2, 3, 4):
        names = combos[points - 1]
        out = _dev(fill(points, points) + guard)
        got = cl.sumcheck_step([tab[x][0] for x in names], gate=R1CS, points=points, length=length, out=out)
        cl.wait_result()
        assert got is out
        assert bytes(out.download()) == _pack(gate_ref([tab[x][1] for x in names], r, length, points, R1CS)) + guard, (names, points)
        out.free()
    out = cl.sumcheck_step([0, 1, w2], length=length)   # PRODUCT, points = k + 1
    cl.wait_result()
    assert out.nbytes == 128 and bytes(out.download()) == _pack(gate_ref(t[:3], r, length, 4, PRODUCT))
    out4 = cl.sumcheck_step([w3, 0, 1, w2], gate=R1CS, length=length)   # R1CS: 4 points
    cl.wait_result()
    assert out4.nbytes == 128 and bytes(out4.download()) == _pack(gate_ref([t[3], t[0], t[1], t[2]], r, length, 4, R1CS))
    assert bytes(cl.result(0)) == _pack(t[0]) and bytes(cl.result(1)) == _pack(t[1])
    assert bytes(w2.download()) == _pack(t[2]) and bytes(w3.download()) == _pack(t[3])
    cl.close()
    for d in (w2, w3, p1, p4, out, out4):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_bind_only(gpu, field):
    """points = 0: all four tables folded in one op, at len = 2 and at len = n; d_out is NULL and the call returns None."""
    logn = 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    rs = challenges(r, 3)
    for turn, length in enumerate((2, n, 2, n)):
        rr = rs[(turn + 3) % 5]
        dr = cl.scalar(rr)
        vals = [_inputs(r, n, 9000 + 10 * turn + j + len(field)) for j in range(4)]
        vals = [v[j:] + v[:j] for j, v in enumerate(vals)]
        w = [_dev(_pack(vals[2])), _dev(_pack(vals[3]))]
        cl.set_data(NTTInput(0, _pack(vals[0])))
        cl.set_data(NTTInput(1, _pack(vals[1])))
        tabs = [0, 1, w[0], w[1]] if turn < 2 else [w[1], 1, 0]
        order = [0, 1, 2, 3] if turn < 2 else [3, 1, 0]
        assert cl.sumcheck_step(tabs, dr, gate=R1CS if turn < 2 else PRODUCT, points=0, length=length) is None
        cl.wait_result()
        half = length // 2
        for t, j in zip(tabs, order):
            got = bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))
            assert got == _pack(fold_ref(vals[j], r, rr, length)) + _pack(vals[j])[32 * half:], (length, j)
        if turn >= 2:
            assert bytes(w[0].download()) == _pack(vals[2])   # not named: not touched
        for d in w + [dr]:
            d.free()
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
def test_agrees_with_the_unfused_ops(gpu, field):
    """vec_mle_fold per table followed by vec_mle_round (for R1CS: round(a, b, c; 4) - round(a, d; 4)) gives the same bytes."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    dr = cl.scalar(_words(len(field), 1)[0])
    raw = [_pack(_inputs(r, n, 9500 + j + len(field))) for j in range(4)]
    for gate, k in GATES:
        # unfused, in device words
        u = [_dev(raw[j]) for j in range(k)]
        for t in u:
            cl.vec_mle_fold(t, t, dr, n); cl.wait_result()
        if gate == R1CS:
            s1 = cl.vec_mle_round(u[0], u[1], u[2], points=4, length=n // 2); cl.wait_result()
            s2 = cl.vec_mle_round(u[0], u[3], points=4, length=n // 2); cl.wait_result()
            want = _pack([(x - y) % r for x, y in zip(_unpack(s1.download()), _unpack(s2.download()))])
            s1.free(); s2.free()
        else:
            s = cl.vec_mle_round(*u, length=n // 2); cl.wait_result()
            want = bytes(s.download())
            s.free()
        # fused: the first two tables in the buffers
        f = [_dev(raw[j]) for j in range(2, k)]
        for b in range(min(k, 2)):
            cl.set_data(NTTInput(b, raw[b]))
        tabs = list(range(min(k, 2))) + f
        out = cl.sumcheck_step(tabs, dr, gate=gate)   # points: the gate's degree + 1
        cl.wait_result()
        assert out.nbytes == 32 * (4 if gate == R1CS else k + 1)
        assert bytes(out.download()) == want, (gate, k)
        for t, ut in zip(tabs, u):
            got = bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))
            assert got == bytes(ut.download()), (gate, k)
        for d in u + f + [out]:
            d.free()
    cl.close()
    dr.free()


def test_second_sweep_of_the_grid_stride_loop(gpu):
    """BLS12-381, len = n = 2^22: 2^20 quads are two sweeps of the 2048 x 256 grid.  R1CS over both buffers and two device-word
    tables.  The expected bytes come from the existing ops - four vec_mle_fold into separate device buffers, round(eq, Az, Bz; 4)
    - round(eq, Cz; 4) on those - run beforehand; every byte is compared, and 256 sampled folded words against Python."""
    field, logn = "BLS381", 22
    n = 1 << logn
    half = n // 2
    r = pyref.CURVES[field]["r"]
    raw = [random.Random(2200 + j).randbytes(32 * n) for j in range(4)]
    rr = _words(2204, 1)[0]
    cl = _client(field, logn)
    dr = cl.scalar(rr)
    w = [_dev(raw[2]), _dev(raw[3])]
    cl.set_data(NTTInput(0, raw[0]))
    cl.set_data(NTTInput(1, raw[1]))
    tabs = [w[1], 0, 1, w[0]]   # eq, Az, Bz, Cz
    exp = [DeviceBuffer(0, 32 * half) for _ in range(4)]
    for e, t in zip(exp, tabs):
        cl.vec_mle_fold(e, t, dr); cl.wait_result()
    s1 = cl.vec_mle_round(exp[0], exp[1], exp[2], points=4); cl.wait_result()
    s2 = cl.vec_mle_round(exp[0], exp[3], points=4); cl.wait_result()
    want = _pack([(x - y) % r for x, y in zip(_unpack(s1.download()), _unpack(s2.download()))])
    out = cl.sumcheck_step(tabs, dr, gate=R1CS)
    cl.wait_result()
    assert bytes(out.download()) == want
    rng = random.Random(2205)
    for t, e, src in zip(tabs, exp, (raw[3], raw[0], raw[1], raw[2])):
        got = bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))
        assert got[:32 * half] == bytes(e.download())
        assert got[32 * half:] == src[32 * half:]
        for p in [0, half - 1] + [rng.randrange(half) for _ in range(62)]:
            lo, hi = (int.from_bytes(src[32 * q: 32 * q + 32], "little") for q in (p, p + half))
            assert got[32 * p: 32 * p + 32] == ((lo + rr * (hi - lo)) % r).to_bytes(32, "little"), p
    cl.close()
    for d in w + exp + [s1, s2, out, dr]:
        d.free()


def test_refusals(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM (InvalidPrimitiveParam) and leaves the tables, d_out and the in-flight state as
    they were."""
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
    mark = bytes(range(1, 161))
    out = _dev(mark)           # 5 words
    big = _dev(bytes(64 * n))  # 2n words
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    B0, B1, W, W2, R = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(words2.ptr, 0, 0, n), V(one_word.ptr, 0, 0, 1)
    P4 = V(words2.ptr, 0, 0, 4)

    def step(gate, x, y, z, d, rr, points, length, o):
        return L.blz_ntt_sumcheck_step(cl._h, gate, _ref(x), _ref(y), _ref(z), _ref(d), _ref(rr), points, length, o)

    o = out.ptr
    refused = {
        "gate 2": (lambda: step(2, B0, None, None, None, R, 2, n, o), "unknown gate 2"),
        "gate 2^31": (lambda: step(1 << 31, B0, B1, W, W2, R, 4, n, o), "unknown gate"),
        "product: no table": (lambda: step(0, None, None, None, None, R, 2, n, o), "BLZ_GATE_PRODUCT takes 1 to 3 tables"),
        "product: b missing": (lambda: step(0, B0, None, W, None, R, 2, n, o), "b is NULL while c is set"),
        "product: a missing": (lambda: step(0, None, B1, None, None, R, 2, n, o), "a is NULL while b is set"),
        "product: d given": (lambda: step(0, B0, B1, W, W2, R, 4, n, o), "BLZ_GATE_PRODUCT takes 1 to 3 tables"),
        "product: d alone behind a": (lambda: step(0, B0, None, None, W2, R, 2, n, o), "b is NULL while d is set"),
        "r1cs: three tables": (lambda: step(1, B0, B1, W, None, R, 4, n, o), "BLZ_GATE_R1CS takes the four tables"),
        "r1cs: c missing": (lambda: step(1, B0, B1, None, W2, R, 4, n, o), "c is NULL while d is set"),
        "points 5": (lambda: step(0, B0, None, None, None, R, 5, n, o), "points 5 is not in [0, 4]"),
        "points 0 without r": (lambda: step(0, B0, None, None, None, None, 0, n, None), "points 0 is a bind alone"),
        "points 0 with d_out": (lambda: step(0, B0, None, None, None, R, 0, n, o), "points 0 is a bind alone"),
        "null d_out": (lambda: step(0, B0, B1, None, None, R, 3, n, None), "null d_out"),
        "null d_out, round only": (lambda: step(1, B0, B1, W, W2, None, 4, n, None), "null d_out"),
        "len 0": (lambda: step(0, B0, None, None, None, R, 2, 0, o), "len 0: the live length is 2^m with 2 <= len <= 256"),
        "len 1": (lambda: step(0, B0, None, None, None, None, 2, 1, o), "len 1: the live length is 2^m"),
        "len 12": (lambda: step(0, B0, None, None, None, R, 2, 12, o), "len 12: the live length is 2^m"),
        "len 2n": (lambda: step(0, B0, None, None, None, R, 2, 2 * n, o), "len 512: the live length is 2^m"),
        "len 2 with r and a round": (lambda: step(0, B0, None, None, None, R, 2, 2, o), "a bind and a round need len >= 4"),
        "r names a buffer": (lambda: step(0, B0, None, None, None, B1, 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "r of two words": (lambda: step(0, B0, None, None, None, V(words.ptr, 0, 0, 2), 2, n, o), "r.d_ptr != NULL, r.count == 1"),
        "r in host memory": (lambda: step(0, B0, None, None, None, V(host_ptr, 0, 0, 1), 2, n, o), "operand r: d_ptr is not"),
        "periodic table with r": (lambda: step(0, B0, P4, None, None, R, 3, 8, o), "operand b: 4 words, read periodically over len 8"),
        "periodic table, bind only": (lambda: step(0, P4, None, None, None, R, 0, 8, None), "operand a: 4 words, read periodically over len 8"),
        "the same buffer twice": (lambda: step(0, B0, B0, None, None, R, 3, n, o), "tables a and b overlap"),
        "the same words twice": (lambda: step(1, B0, W, B1, W, R, 4, n, o), "tables b and d overlap"),
        "tables that overlap in part": (lambda: step(0, V(words.ptr, 0, 0, 8), V(words.ptr + 32 * 4, 0, 0, 8), None, None, R, 3, 8, o), "tables a and b overlap"),
        "r in the words written": (lambda: step(0, W, None, None, None, V(words.ptr + 32 * 3, 0, 0, 1), 2, 8, o), "r lies in the words table a receives"),
        "r in the words of b written": (lambda: step(0, B0, W, None, None, V(words.ptr, 0, 0, 1), 3, 8, o), "r lies in the words table b receives"),
        "d_out in host memory": (lambda: step(0, B0, None, None, None, R, 2, n, host_ptr), "operand d_out: d_ptr is not"),
        "d_out misaligned": (lambda: step(0, B0, None, None, None, R, 2, n, o + 8), "operand d_out: d_ptr is not 16-byte aligned"),
        "d_out past its allocation": (lambda: step(0, B0, None, None, None, R, 4, n, o + 64), "operand d_out: 4 elements run past the end"),
        "d_out on a table": (lambda: step(0, B0, W, None, None, R, 3, n, words.ptr + 32 * (n - 3)), "d_out overlaps the words of a d_ptr operand"),
        "d_out on a table, round only": (lambda: step(1, B0, W, B1, W2, None, 4, n, words2.ptr), "d_out overlaps the words of a d_ptr operand"),
        "d_out on r": (lambda: step(0, B0, None, None, None, R, 1, n, one_word.ptr), "d_out overlaps the words of a d_ptr operand"),
        "a reserved": (lambda: step(0, V(None, 0, 7, 0), None, None, None, R, 2, n, o), "operand a: reserved must be 0"),
        "b buf 2": (lambda: step(0, B0, V(None, 2, 0, 0), None, None, R, 3, n, o), "operand b: buf must be 0 or 1"),
        "c count 3": (lambda: step(0, B0, B1, V(words.ptr, 0, 0, 3), None, R, 4, n, o), "operand c: count 3 is not a power of two"),
        "d count 2n": (lambda: step(1, B0, B1, W, V(big.ptr, 0, 0, 2 * n), R, 4, n, o), "operand d: count 512 is not a power of two in [1, 256]"),
        "d in host memory": (lambda: step(1, B0, B1, W, V(host_ptr, 0, 0, n), None, 4, n, o), "operand d: d_ptr is not"),
        "a misaligned": (lambda: step(0, V(words.ptr + 8, 0, 0, 1), None, None, None, None, 2, n, o), "operand a: d_ptr is not 16-byte aligned"),
        "a past its allocation": (lambda: step(0, V(one_word.ptr, 0, 0, 2), None, None, None, None, 2, n, o), "operand a: 2 elements run past the end"),
    }
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    with pytest.raises(DriverClientError) as ei:
        cl.sumcheck_step([0, 0], one_word)
    assert ei.value.variant == "InvalidPrimitiveParam"
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and bytes(words2.download()) == ab and _word(one_word) == 7 and bytes(out.download()) == mark
    # an op already in flight
    cl.vec_mle_round(0, words)
    assert step(0, B0, None, None, None, R, 2, n, o) == 4 and "already running" in L.blz_last_error_message().decode()
    assert step(1, B0, B1, W, W2, None, 4, n, o) == 4
    cl.wait_result()
    assert bytes(cl.result(0)) == ab and bytes(out.download()) == mark
    cl.close()
    for d in (words, words2, one_word, out, big):
        d.free()


def test_order_of_checks(gpu):
    """A call wrong in two ways reports the earlier check: gate, points, d_out, r's shape, the live length, len >= 4 for a bind
    with a round, an op in flight, the operands, then per table a periodic one, an overlap, r in the words it receives.  Checks
    that read the same argument cannot all meet in one call (points above 4 and points 0; points 0 and a NULL d_out with points):
    each is set against the nearest check it can meet."""
    field, logn = "BLS381", 3
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 81), _inputs(r, n, 82)
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

    def step(gate, x, y, rr, points, length, d_out):
        return L.blz_ntt_sumcheck_step(cl._h, gate, _ref(x), _ref(y), None, None, _ref(rr), points, length, d_out)

    def good():
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); out.upload(mark)
        assert step(PRODUCT, B0, B1, R, 3, n, o + 32) == 0, L.blz_last_error_message()
        cl.wait_result()
        fa, fb = fold_ref(a, r, 7, n), fold_ref(b, r, 7, n)
        assert bytes(cl.result(0)) == _pack(fa) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fb) + bb[16 * n:]
        assert bytes(out.download()) == mark[:32] + _pack(gate_ref([fa, fb], r, n // 2, 3, PRODUCT)) + mark[128:]

    P = PRODUCT
    cases = [
        ("gate, points", (lambda: step(2, B0, None, R, 5, n, o), "unknown gate 2", False), (lambda: step(P, B0, None, R, 5, n, o), "points 5 is not in [0, 4]", False)),
        ("points, null d_out", (lambda: step(P, B0, None, R, 5, n, None), "points 5 is not in [0, 4]", False), (lambda: step(P, B0, None, R, 3, n, None), "null d_out", False)),
        ("points 0, r", (lambda: step(P, B0, None, B1, 0, n, o), "points 0 is a bind alone", False), (lambda: step(P, B0, None, B1, 2, n, o), "r.d_ptr != NULL, r.count == 1", False)),
        ("null d_out, r", (lambda: step(P, B0, None, B1, 3, n, None), "null d_out", False), (lambda: step(P, B0, None, B1, 3, n, o), "r.d_ptr != NULL, r.count == 1", False)),
        ("r, len", (lambda: step(P, B0, None, B1, 2, 12, o), "r.d_ptr != NULL, r.count == 1", False), (lambda: step(P, B0, None, R, 2, 12, o), "len 12: the live length is 2^m", False)),
        ("len, len >= 4", (lambda: step(P, B0, None, R, 2, 3, o), "len 3: the live length is 2^m", False), (lambda: step(P, B0, None, R, 2, 2, o), "a bind and a round need len >= 4", False)),
        ("len >= 4, in flight", (lambda: step(P, B0, None, R, 2, 2, o), "a bind and a round need len >= 4", True), (lambda: step(P, B0, None, R, 2, n, o), "already running", True)),
        ("in flight, operand", (lambda: step(P, V(None, 0, 7, 0), None, R, 2, n, o), "already running", True),
         (lambda: step(P, V(None, 0, 7, 0), None, R, 2, n, o), "operand a: reserved must be 0", False)),
        ("operand, periodic", (lambda: step(P, P4, BAD, R, 3, 8, o), "operand b: buf must be 0 or 1", False),
         (lambda: step(P, P4, B1, R, 3, 8, o), "operand a: 4 words, read periodically over len 8", False)),
        ("periodic, overlap", (lambda: step(P, W, P4, R, 3, 8, o), "operand b: 4 words, read periodically over len 8", False), (lambda: step(P, W, W, R, 3, 8, o), "tables a and b overlap", False)),
        ("overlap, r in the words written", (lambda: step(P, LO, HI, R5, 3, 8, o), "tables a and b overlap", False),
         (lambda: step(P, B0, HI, R5, 3, 8, o), "r lies in the words table b receives", False)),
    ]
    check_order_of_checks(cl, cases, lambda: cl.vec_mle_round(words, out=s), good)
    assert bytes(words.download()) == bb and bytes(big.download()) == bytes(32 * 12) and _word(one_word) == 7
    cl.close()
    for d in (words, big, one_word, out, s):
        d.free()


def test_in_flight_rules(gpu):
    """A step that writes BOTH buffers in flight: neither can be read, written or exchanged and nothing else starts.  A round alone
    writes none: both can be read, the ones it reads cannot be written.  reset drops the op."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c = (_inputs(r, n, 70 + i) for i in range(3))
    ab, bb, cb = _pack(a), _pack(b), _pack(c)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words, one_word = _dev(cb), _dev((7).to_bytes(32, "little"))
    host_out = bytearray(32 * n)
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.vec_mle_round(words), lambda: cl.sumcheck_step([words]),
            lambda: cl.sumcheck_step([0, 1], one_word), lambda: cl.sumcheck_step([words], one_word, points=0))
    # the second table is the second written buffer: 1 then 0, and 0 then 1
    for tabs, vals in (([1, words, 0], [b, c, a]), ([0, 1], [a, b])):
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb)
        out = cl.sumcheck_step(tabs, one_word)
        for attempt in busy + (lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
                               lambda: cl.exchange(0, ab, host_out), lambda: cl.exchange(1, ab, host_out)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        folded = [fold_ref(v, r, 7, n) for v in vals]
        assert bytes(out.download()) == _pack(gate_ref(folded, r, n // 2, len(tabs) + 1, PRODUCT))
        assert bytes(cl.result(0)) == _pack(fold_ref(a, r, 7, n)) + ab[16 * n:] and bytes(cl.result(1)) == _pack(fold_ref(b, r, 7, n)) + bb[16 * n:]
        out.free()
    # a step on one buffer: the other one is free
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    out = cl.sumcheck_step([1], one_word)
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
    out = cl.sumcheck_step([words, 0, 0, words], gate=R1CS)
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(1, bb))   # not named
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(out.download()) == _pack(gate_ref([c, a, a, c], r, n, 4, R1CS))
    out.free()
    # a transform afterwards records one buffer again: the other can be read while it runs or after
    cl.sumcheck_step([0, 1], one_word, points=0); cl.wait_result()
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    cl.vec_mle_fold(1, 0, one_word)
    assert bytes(cl.result(0)) == ab
    cl.wait_result()
    # reset with a step in flight: nothing is in flight afterwards, and the handle works
    for start in (lambda: cl.sumcheck_step([0, 1], one_word), lambda: cl.sumcheck_step([0, 1, words, words], gate=R1CS),
                  lambda: cl.sumcheck_step([1, 0], one_word, points=0)):
        start()
        cl.reset()
        with pytest.raises(DriverClientError):
            cl.wait_result()
        cl.result(0); cl.result(1)
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    out = cl.sumcheck_step([0, 1], one_word)
    cl.wait_result()
    assert bytes(out.download()) == _pack(gate_ref([fold_ref(a, r, 7, n), fold_ref(b, r, 7, n)], r, n // 2, 3, PRODUCT))
    cl.close()
    for d in (words, one_word, out):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_end_to_end(gpu, field):
    """A satisfied random R1CS of 2^10 constraints through vec_spmv to Az, Bz, Cz, then the sumcheck for
    sum_p eq(p) (Az(p) Bz(p) - Cz(p)) = 0 in 12 ops: eq, a step without r, (a challenge uploaded as a device word, a step with r)
    x 9, a bind alone.  Az and Bz stay in the buffers, Cz and eq in device words.  Every round's s(0) + s(1) is the previous
    claim, the last claim is the gate of the four final words, and the same transcript through vec_mle_round / vec_mle_fold on
    copies of the tables gives the same bytes every round."""
    m = 10
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 90)
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
    arrays = [_dev(b) for b in (_u32(rpC), _u32(colC), _pack(valC), _u32(A[0]), _u32(A[1]), _pack(A[2]), _u32(B[0]), _u32(B[1]), _pack(B[2]))]
    cl.vec_spmv(0, dz, arrays[1], row_ptr=arrays[0], val=arrays[2]); cl.wait_result()
    cl.result_device(0, d_cz)
    cl.vec_spmv(0, dz, arrays[4], row_ptr=arrays[3], val=arrays[5]); cl.wait_result()
    cl.vec_spmv(1, dz, arrays[7], row_ptr=arrays[6], val=arrays[8]); cl.wait_result()
    assert bytes(cl.result(0)) == _pack(az) and bytes(cl.result(1)) == _pack(bz) and bytes(d_cz.download()) == _pack(cz)
    tau = _words(len(field) + 91, m)
    point = _dev(_pack(tau))
    cl.vec_mle_eq(d_eq, point); cl.wait_result()
    eq0 = _unpack(d_eq.download())
    # the unfused transcript's tables: copies, all in device words
    u_eq, u_az, u_bz, u_cz = (_dev(_pack(v)) for v in (eq0, az, bz, cz))
    s_dev, s1, s2 = DeviceBuffer(0, 128), DeviceBuffer(0, 128), DeviceBuffer(0, 128)
    fused = [d_eq, 0, 1, d_cz]
    claim, challenges, dc = 0, [], None
    for rnd in range(m):
        length = n >> rnd   # the live length of this round's polynomial
        if rnd == 0:
            cl.sumcheck_step(fused, gate=R1CS, length=length, out=s_dev); cl.wait_result()
        else:
            cl.sumcheck_step(fused, dc, gate=R1CS, length=2 * length, out=s_dev); cl.wait_result()
            for t in (u_eq, u_az, u_bz, u_cz):
                cl.vec_mle_fold(t, t, dc, 2 * length); cl.wait_result()
            dc.free()
        cl.vec_mle_round(u_eq, u_az, u_bz, points=4, length=length, out=s1); cl.wait_result()
        cl.vec_mle_round(u_eq, u_cz, points=4, length=length, out=s2); cl.wait_result()
        got = bytes(s_dev.download())
        assert got == _pack([(x - y) % r for x, y in zip(_unpack(s1.download()), _unpack(s2.download()))]), (rnd, "the unfused ops")
        s = _unpack(got)
        assert (s[0] + s[1]) % r == claim, (rnd, "s(0) + s(1) = claim")
        c = rng.getrandbits(256)
        challenges.append(c)
        dc = cl.scalar(c)
        claim = interpolate(s, c, r)
    assert cl.sumcheck_step(fused, dc, gate=R1CS, points=0, length=2) is None
    cl.wait_result()
    for t in (u_eq, u_az, u_bz, u_cz):
        cl.vec_mle_fold(t, t, dc, 2); cl.wait_result()
    finals = [_word(d_eq), _unpack(cl.result(0))[0], _unpack(cl.result(1))[0], _word(d_cz)]
    assert finals == [_word(t) for t in (u_eq, u_az, u_bz, u_cz)]
    assert claim == finals[0] * (finals[1] * finals[2] - finals[3]) % r
    # each final word is the original table at the challenges (the top variable was bound first), in integers

    def atchallenges(table):
        for c in challenges:
            h = len(table) // 2
            table = [(table[p] + c * (table[p + h] - table[p])) % r for p in range(h)]
        return table[0]

    assert finals == [atchallenges(t) for t in (eq0, az, bz, cz)]
    cl.close()
    for d in arrays + [dz, d_cz, d_eq, point, u_eq, u_az, u_bz, u_cz, s_dev, s1, s2, dc]:
        d.free()
