"""Folds along a resident buffer (blz_ntt_vec_reduce, blz_ntt_vec_scan) on the device: sum, inner product and evaluation at a
point; running sums and products.  Every expected value is Python integer arithmetic and every comparison is byte for byte:
any 256-bit input word counts as its residue, every output word is canonical.  The input recipe is test_gpu_ntt_vec.py's:
the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random 256-bit words (more than half of them >= r) behind."""
import ctypes as C
import itertools
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_vec_util import FIELDS, GENERATOR, _client, _dev, _edges, _pack, _transform, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
TILE = 1024   # csrc/ntt_engine.hpp NTT_FOLD_TILE: positions per block of a scan
SUM, DOT, EVAL = NTTClient.FOLD_SUM, NTTClient.FOLD_DOT, NTTClient.FOLD_EVAL
SSUM, SPROD = NTTClient.SCAN_SUM, NTTClient.SCAN_PROD


def _inputs(field, n, seed):
    """a, b: the 6 x 6 combinations of the edge words first (as far as n reaches), random 256-bit words behind them."""
    r = pyref.CURVES[field]["r"]
    e = _edges(r)
    a, b = _words(seed, n), _words(seed + 1, n)
    for i in range(min(n, 36)):
        a[i], b[i] = e[i % 6], e[(i // 6) % 6]
    return a, b


def _nonzero(vals, r):
    return [v if v % r else 1 for v in vals]


def _reduce(cl, op, a, b=None, out=None):
    out = cl.vec_reduce(op, a, b, out)
    cl.wait_result()
    return _word(out)


def _horner(a, z, r):
    acc = 0
    for v in reversed(a):
        acc = (acc * z + v) % r
    return acc


def _scan_want(op, a, r, exclusive):
    """(dst, total) as Python integers"""
    if op == SSUM:
        inc = list(itertools.accumulate(a, lambda x, y: (x + y) % r, initial=0))[1:]
        ident = 0
    else:
        inc = list(itertools.accumulate(a, lambda x, y: x * y % r, initial=1))[1:]
        ident = 1
    return ([ident] + inc[:-1] if exclusive else inc), inc[-1]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 8, 11, 14])
def test_reduce_against_python_integers(gpu, field, logn):
    """Less than a wave, a wave, one block, several blocks, 64 blocks.  a from a transform buffer and from device words; b a full
    vector (a transform buffer, device words) and periodic; z among 0 (0^0 = 1), 1, r - 1, r + 1, a random word >= r and the
    generator.  The buffers read keep their bytes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b = _inputs(field, n, 300 * logn + len(field))
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    da, db = _dev(ab), _dev(bb)
    out = DeviceBuffer(0, 32)
    want = sum(a) % r
    assert _reduce(cl, SUM, 0) == want, "SUM, buffer 0"
    assert _reduce(cl, SUM, da, None, out) == want, "SUM, device words"
    want = sum(x * y for x, y in zip(a, b)) % r
    assert _reduce(cl, DOT, 0, 1, out) == want, "DOT, buffer 0 . buffer 1"
    assert _reduce(cl, DOT, da, db, out) == want, "DOT, device words . device words"
    assert _reduce(cl, DOT, 1, da, out) == want, "DOT, buffer 1 . device words"
    assert _reduce(cl, DOT, 0, 0) == sum(x * x for x in a) % r, "DOT, a == b"
    for count in sorted({1, min(4, n), n}):
        dp = _dev(_pack(b[:count]))
        want = sum(a[p] * b[p & (count - 1)] for p in range(n)) % r
        assert _reduce(cl, DOT, 0, dp, out) == want, f"DOT, b of {count} words"
        dp.free()
    big = next(w for w in _words(logn, 64) if w >= r)
    for k, z in enumerate((0, 1, r - 1, r + 1, big, GENERATOR[field])):
        dz = cl.scalar(z)
        assert _reduce(cl, EVAL, 0, dz, out) == _horner(a, z % r, r), f"EVAL at z #{k}, buffer 0"
        if k >= 4:
            assert _reduce(cl, EVAL, db, dz) == _horner(b, z % r, r), f"EVAL at z #{k}, device words"
        dz.free()
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.close()
    for d in (da, db, out):
        d.free()


def test_reduce_second_grid_stride_step(gpu):
    """2^20 elements on a grid of 2^19 lanes: every lane takes two steps (EVAL: two Horner steps with z^(2^19)).  BLS12-381 only,
    one set of inputs, plain integer Horner."""
    field, logn = "BLS381", 20
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b = _inputs(field, n, 2020)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    assert _reduce(cl, DOT, 0, 1) == sum(x * y for x, y in zip(a, b)) % r
    z = b[77]
    assert z >= 1 << 200
    dz = cl.scalar(z)
    assert _reduce(cl, EVAL, 0, dz) == _horner(a, z % r, r)
    assert _reduce(cl, SUM, 1) == sum(b) % r
    dz.free()
    cl.close()


def _scan(cl, op, dst, a, exclusive, total):
    cl.vec_scan(op, dst, a, exclusive=exclusive, total=total)
    cl.wait_result()
    return bytes(cl.result(dst))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 8, 10, 11, 12])
def test_scan_against_python_integers(gpu, field, logn):
    """Part of a tile, exactly one tile (2^10), two tiles - the carry crosses a tile edge - and four.  Inclusive and exclusive; out
    of place, in place and from device words; with and without d_total, which is the last inclusive value.  The product scan
    runs on words without a zero, then with one planted: at position 0, at the last position of a tile, at the first position of
    the next tile (where there is one), and as the word r - everything behind a zero is 0, everything before it unaffected."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, _ = _inputs(field, n, 500 * logn + len(field))
    cl = _client(field, logn)
    total = DeviceBuffer(0, 32)
    for op in (SSUM, SPROD):
        x = a if op == SSUM else _nonzero(a, r)
        xb = _pack(x)
        dx = _dev(xb)
        for exclusive in (False, True):
            want, tot = _scan_want(op, [v % r for v in x], r, exclusive)
            want = _pack(want)
            what = f"{field} 2^{logn} op {op} exclusive {exclusive}"
            cl.set_data(NTTInput(0, xb))
            assert _scan(cl, op, 1, 0, exclusive, total) == want, what + ": buffer 0 -> buffer 1"
            assert _word(total) == tot, what
            assert bytes(cl.result(0)) == xb
            assert _scan(cl, op, 0, 0, exclusive, None) == want, what + ": in place, no d_total"
            total.upload(bytes(32))
            assert _scan(cl, op, 0, dx, exclusive, total) == want, what + ": device words -> buffer 0"
            assert _word(total) == tot, what
        dx.free()
    # planted zeros
    tile = min(TILE, n)
    plants = [(0, 0), (tile - 1, 0), (n // 2, r)]
    if n > TILE:
        plants.append((TILE, 0))
    base = _nonzero(a, r)
    for pos, word in plants:
        x = list(base)
        x[pos] = word
        for exclusive in (False, True):
            want, tot = _scan_want(SPROD, [v % r for v in x], r, exclusive)
            first_zero = pos + 1 if exclusive else pos
            assert tot == 0 and not any(want[first_zero:]) and all(want[:first_zero])
            cl.set_data(NTTInput(1, _pack(x)))
            assert _scan(cl, SPROD, 1, 1, exclusive, total) == _pack(want), f"{field} 2^{logn}: zero {word:#x} at {pos}"
            assert _word(total) == 0
    total.free()
    cl.close()


def test_scan_second_level_of_the_totals(gpu):
    """2^21 elements are 2048 tiles of 1024: the tiles' totals no longer fit the one block that scans up to 1024 of them, and
    the totals are themselves scanned in two tiles with a second level of two totals above them.  BLS12-381 only, the inclusive
    product scan in place, against a running Python product."""
    field, logn = "BLS381", 21
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    x = _nonzero(_words(2121, n), r)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(x)))
    total = DeviceBuffer(0, 32)
    got = _scan(cl, SPROD, 0, 0, False, total)
    want = list(itertools.accumulate(x, lambda u, v: u * v % r, initial=1))[1:]
    assert got == _pack(want)
    assert _word(total) == want[-1]
    total.free()
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
def test_exclusive_product_scan_of_one_word_writes_its_powers(gpu, field):
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    z = next(w for w in _words(11, 64) if w >= r)
    cl = _client(field, logn)
    dz = cl.scalar(z)
    total = DeviceBuffer(0, 32)
    assert _scan(cl, SPROD, 1, dz, True, total) == _pack([pow(z, p, r) for p in range(n)])
    assert _word(total) == pow(z, n, r)
    dz.free()
    total.free()
    cl.close()


@pytest.mark.parametrize("field", ["BLS381", "BN254"])
def test_grand_product_and_evaluation_at_a_point(gpu, orc, field):
    """What the folds are for.  (a) The grand-product column of a permutation argument: den a permutation of num, Z[0] = 1,
    Z[p + 1] = Z[p] num[p] / den[p] - the batch inversion, the product and an exclusive product scan, whose total is 1.  (b) The
    transform's output word k IS the polynomial's value at w^k, w = g^((r - 1) / n) the documented default root: EVAL of the
    coefficients at w^k against the transform, for k = 0, 1, n / 2, n - 1.  Between the first set_data and the checks everything
    stays on the device."""
    logn = 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field))
    num = [rng.randrange(1, r) for _ in range(n)]
    den = list(num)
    rng.shuffle(den)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(num)))
    cl.set_data(NTTInput(1, _pack(den)))
    total = DeviceBuffer(0, 32)
    cl.vec_op(NTTClient.INV, 1, 1)
    cl.wait_result()
    cl.vec_op(NTTClient.MUL, 0, 0, 1)
    cl.wait_result()
    cl.vec_scan(SPROD, 0, 0, exclusive=True, total=total)
    cl.wait_result()
    z = [1]
    for p in range(n - 1):
        z.append(z[-1] * num[p] * pow(den[p], -1, r) % r)
    assert bytes(cl.result(0)) == _pack(z)
    assert _word(total) == 1
    # (b)
    c = [rng.randrange(r) for _ in range(n)]
    cb = _pack(c)
    d_c = DeviceBuffer(0, 32 * n)
    cl.set_data(NTTInput(0, cb))
    cl.result_device(0, d_c)
    _transform(cl, 0)
    w = pow(GENERATOR[field], (r - 1) >> logn, r)
    outs = []
    for k in (0, 1, n // 2, n - 1):
        dz = cl.scalar(pow(w, k, r))
        outs.append((k, cl.vec_reduce(EVAL, d_c, dz), dz))
        cl.wait_result()
    spectrum = bytes(cl.result(0))
    assert spectrum == bytes(orc.ntt(field, cb, logn))
    X = _unpack(spectrum)
    for k, out, dz in outs:
        assert _word(out) == X[k] == _horner(c, pow(w, k, r), r), k
        out.free()
        dz.free()
    for d in (total, d_c):
        d.free()
    cl.close()


def test_protocol_and_refusals(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(field, n, 5)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    mark = bytes(range(1, 65))   # device memory comes as it is: give the words no op may write bytes of their own
    out = _dev(mark)
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def ref(v):
        return None if v is None else C.byref(v)

    def reduce(op, x, y, o):
        return L.blz_ntt_vec_reduce(cl._h, op, ref(x), ref(y), o)

    def scan(op, flags, dst, x, t):
        return L.blz_ntt_vec_scan(cl._h, op, flags, dst, ref(x), t)

    B0, B1, W, Z = BlzVecArg(None, 0, 0, 0), BlzVecArg(None, 1, 0, n), BlzVecArg(words.ptr, 0, 0, n), BlzVecArg(one_word.ptr, 0, 0, 1)
    refused = {
        "unknown reduction 3": lambda: reduce(3, B0, B1, out.ptr),
        "unknown reduction -1": lambda: reduce(-1, B0, B1, out.ptr),
        "no a": lambda: reduce(DOT, None, B1, out.ptr),
        "DOT without b": lambda: reduce(DOT, B0, None, out.ptr),
        "EVAL without b": lambda: reduce(EVAL, B0, None, out.ptr),
        "SUM with b": lambda: reduce(SUM, B0, B1, out.ptr),
        "EVAL at a transform buffer": lambda: reduce(EVAL, B0, B1, out.ptr),
        "EVAL at two words": lambda: reduce(EVAL, B0, BlzVecArg(words.ptr, 0, 0, 2), out.ptr),
        "EVAL at n words": lambda: reduce(EVAL, B0, W, out.ptr),
        "null d_out": lambda: reduce(SUM, B0, None, None),
        "d_out in host memory": lambda: reduce(SUM, B0, None, host_ptr),
        "d_out misaligned": lambda: reduce(SUM, B0, None, out.ptr + 8),
        "d_out runs past its allocation": lambda: reduce(SUM, B0, None, out.ptr + 48),
        "d_out on a's words": lambda: reduce(SUM, W, None, words.ptr + 32 * (n - 1)),
        "d_out on b's words": lambda: reduce(DOT, B0, W, words.ptr),
        "d_out on the point": lambda: reduce(EVAL, B0, Z, one_word.ptr),
        "buf 2": lambda: reduce(SUM, BlzVecArg(None, 2, 0, 0), None, out.ptr),
        "reserved": lambda: reduce(DOT, B0, BlzVecArg(None, 1, 7, 0), out.ptr),
        "count 3": lambda: reduce(DOT, B0, BlzVecArg(words.ptr, 0, 0, 3), out.ptr),
        "count 2n": lambda: reduce(SUM, BlzVecArg(words.ptr, 0, 0, 2 * n), None, out.ptr),
        "count of a transform buffer": lambda: reduce(SUM, BlzVecArg(None, 1, 0, n // 2), None, out.ptr),
        "operand in host memory": lambda: reduce(SUM, BlzVecArg(host_ptr, 0, 0, n), None, out.ptr),
        "operand misaligned": lambda: reduce(DOT, B0, BlzVecArg(words.ptr + 8, 0, 0, 1), out.ptr),
        "unknown scan 2": lambda: scan(2, 0, 0, B0, None),
        "unknown scan -1": lambda: scan(-1, 0, 0, B0, None),
        "unknown flag bit 1": lambda: scan(SSUM, 2, 0, B0, None),
        "unknown flag bit 31": lambda: scan(SPROD, 0x80000001, 0, B0, None),
        "buf_dst 2": lambda: scan(SSUM, 0, 2, B0, None),
        "scan without a": lambda: scan(SSUM, 0, 0, None, None),
        "d_total in host memory": lambda: scan(SSUM, 0, 0, B0, host_ptr),
        "d_total misaligned": lambda: scan(SSUM, 1, 0, B0, out.ptr + 4),
        "d_total runs past its allocation": lambda: scan(SSUM, 1, 0, B0, out.ptr + 48),
        "d_total on a's words": lambda: scan(SPROD, 0, 1, W, words.ptr + 64),
        "scan: count 0": lambda: scan(SSUM, 0, 0, BlzVecArg(words.ptr, 0, 0, 0), None),
        "scan: reserved": lambda: scan(SSUM, 0, 0, BlzVecArg(None, 0, 1, 0), None),
        "scan: operand past its allocation": lambda: scan(SSUM, 0, 0, BlzVecArg(one_word.ptr, 0, 0, 2), None),
    }
    for what, attempt in refused.items():
        assert attempt() == 4, what
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and _word(one_word) == 7 and bytes(out.download()) == mark
    # a reduce in flight: buffer 0 . words
    busy = (lambda: cl.start_process(1), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words),
            lambda: cl.vec_reduce(SUM, 1), lambda: cl.vec_scan(SSUM, 1, 1))
    res = cl.vec_reduce(DOT, 0, words)
    sink = bytearray(32 * n)
    for attempt in (lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(0, words)), lambda: cl.exchange(0, ab, sink)):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    assert bytes(cl.result(0)) == ab          # the operand it reads can be read
    cl.set_data(NTTInput(1, ab))              # the buffer it does not name is free
    assert bytes(cl.result(1)) == ab
    cl.set_data(NTTInput(1, bb))
    for attempt in busy:
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    assert _word(res) == sum(x * y for x, y in zip(a, b)) % r
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    # a scan in flight: buffer 1 = the running sums of buffer 0
    cl.vec_scan(SSUM, 1, 0)
    for buf in (0, 1):
        for attempt in (lambda: cl.set_data(NTTInput(buf, ab)), lambda: cl.exchange(buf, ab, sink)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam" and f"buffer {buf}" in str(ei.value)
    assert bytes(cl.result(0)) == ab
    for attempt in busy + (lambda: cl.result(1),):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want = _pack(_scan_want(SSUM, [v % r for v in a], r, False)[0])
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab and cl.coset == 1
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with an op in flight: nothing is in flight afterwards, and the handle works
    for start in (lambda: cl.vec_scan(SPROD, 1, 0), lambda: cl.vec_reduce(EVAL, 0, one_word)):
        start()
        cl.reset()
        with pytest.raises(DriverClientError):
            cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    assert _reduce(cl, EVAL, 0, one_word) == _horner(a, 7, r)
    assert _scan(cl, SSUM, 1, 0, False, None) == want
    cl.close()
    for d in (words, one_word, out, res):
        d.free()
