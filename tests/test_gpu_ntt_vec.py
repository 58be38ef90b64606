"""Element-wise ops on resident buffers (blz_ntt_vec_op) on the device: dst = a + b, a - b, a * b, a * b + c, a * b - c and the
batch inversion, position by position over the handle's field.  Every expected value is Python integer arithmetic: the ops are
exact, so every comparison is byte for byte - any 256-bit input word counts as its residue, every output word is canonical."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput, VEC_INV_TILE
from ntt_vec_util import FIELDS, GENERATOR, TOP, _client, _dev, _edges, _pack, _transform, _unpack, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
OPS = {
    NTTClient.ADD: lambda x, y, z, r: (x + y) % r,
    NTTClient.SUB: lambda x, y, z, r: (x - y) % r,
    NTTClient.MUL: lambda x, y, z, r: x * y % r,
    NTTClient.MULADD: lambda x, y, z, r: (x * y + z) % r,
    NTTClient.MULSUB: lambda x, y, z, r: (x * y - z) % r,
}
TAKES_C = (NTTClient.MULADD, NTTClient.MULSUB)


def _inputs(field, n, seed):
    """a, b, c: the 6 x 6 x 6 combinations of the edge words first (as far as n reaches), random 256-bit words behind them."""
    r = pyref.CURVES[field]["r"]
    e = _edges(r)
    a, b, c = _words(seed, n), _words(seed + 1, n), _words(seed + 2, n)
    for i in range(min(n, 216)):
        a[i], b[i], c[i] = e[i % 6], e[(i // 6) % 6], e[(i // 36) % 6]
    return a, b, c


def _run(cl, op, dst, a, b=None, c=None):
    cl.vec_op(op, dst, a, b, c)
    cl.wait_result()
    return bytes(cl.result(dst))


def _check_arithmetic(field, logn, ops, inputs):
    r = pyref.CURVES[field]["r"]
    a, b, c = inputs
    ab, bb, cb = _pack(a), _pack(b), _pack(c)
    cl = _client(field, logn)
    da, db, dc = _dev(ab), _dev(bb), _dev(cb)
    for op in ops:
        want = _pack([OPS[op](x, y, z, r) for x, y, z in zip(a, b, c)])
        third = op in TAKES_C
        # a in a transform buffer, b (and c) device words, the result lands on the other buffer
        cl.set_data(NTTInput(0, ab))
        got = _run(cl, op, 1, 0, db, dc if third else None)
        assert got == want, f"{field} 2^{logn} op {op}: a = buffer 0, b = device words"
        assert bytes(cl.result(0)) == ab
        # a device words, b (and c) transform buffers, in place on b
        cl.set_data(NTTInput(1, bb))
        if third:
            cl.set_data(NTTInput(0, cb))
        got = _run(cl, op, 1, da, 1, 0 if third else None)
        assert got == want, f"{field} 2^{logn} op {op}: a = device words, b = buffer 1 = dst"
    cl.close()
    for d in (da, db, dc):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 11, 14])
def test_arithmetic_ops_against_python_integers(gpu, field, logn):
    """Less than a wave, exactly a wave, several blocks, 64 blocks.  (The grid is capped at 2048 blocks of 256 lanes: the
    grid-stride loop takes its second step from 2^20 on - test_arithmetic_ops_second_grid_stride_step.)"""
    _check_arithmetic(field, logn, sorted(OPS), _inputs(field, 1 << logn, 100 * logn + len(field)))


_BIG = {}


@pytest.mark.parametrize("op", sorted(OPS))
def test_arithmetic_ops_second_grid_stride_step(gpu, op):
    """2^20 elements on a grid of 2^19 lanes: every lane takes two steps.  BLS12-381 only; one set of inputs for the five ops."""
    if "in" not in _BIG:
        _BIG["in"] = _inputs("BLS381", 1 << 20, 2020)
    _check_arithmetic("BLS381", 20, [op], _BIG["in"])


@pytest.mark.parametrize("field", FIELDS)
def test_periodic_operands(gpu, field):
    """b of 1, 2, 4, 64 and n words, c of one word: position p reads word p & (count - 1)."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c = _inputs(field, n, 4711)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(a)))
    dc = _dev(_pack(c[:1]))
    for count in (1, 2, 4, 64, n):
        db = _dev(_pack(b[:count]))
        for op in (NTTClient.SUB, NTTClient.MUL, NTTClient.MULSUB):
            want = _pack([OPS[op](a[p], b[p & (count - 1)], c[0], r) for p in range(n)])
            got = _run(cl, op, 1, 0, db, dc if op in TAKES_C else None)
            assert got == want, f"{field} count {count} op {op}"
        db.free()
    # the periodic operand first: a of 4 words against a full vector
    da = _dev(_pack(a[:4]))
    cl.set_data(NTTInput(1, _pack(b)))
    assert _run(cl, NTTClient.MULADD, 0, da, 1, cl.scalar(c[5])) == _pack([(a[p & 3] * b[p] + c[5]) % r for p in range(n)])
    da.free()
    dc.free()
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
def test_aliasing(gpu, field):
    """dst == a, dst == b, a == b (a square), all three the same buffer; the buffer that is not the destination keeps its bytes."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, _ = _inputs(field, n, 99)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)

    def fresh():
        cl.set_data(NTTInput(0, ab))
        cl.set_data(NTTInput(1, bb))

    fresh()
    assert _run(cl, NTTClient.MUL, 0, 0, 1) == _pack([x * y % r for x, y in zip(a, b)]), "dst == a"
    assert bytes(cl.result(1)) == bb
    fresh()
    assert _run(cl, NTTClient.SUB, 1, 0, 1) == _pack([(x - y) % r for x, y in zip(a, b)]), "dst == b"
    assert bytes(cl.result(0)) == ab
    fresh()
    assert _run(cl, NTTClient.MUL, 1, 0, 0) == _pack([x * x % r for x in a]), "a == b"
    assert bytes(cl.result(0)) == ab
    fresh()
    assert _run(cl, NTTClient.MUL, 0, 0, 0) == _pack([x * x % r for x in a]), "dst == a == b"
    assert bytes(cl.result(1)) == bb
    fresh()
    assert _run(cl, NTTClient.MULADD, 1, 1, 1, 1) == _pack([(y * y + y) % r for y in b]), "dst == a == b == c"
    assert bytes(cl.result(0)) == ab
    cl.close()


def _inverse_input(field, n, seed):
    """Random 256-bit words with zeros where the batch inversion can trip: alone, adjacent, at the first and the last position of
    a tile, as the word r, and a whole tile of them."""
    r = pyref.CURVES[field]["r"]
    x = _words(seed, n)
    x = [v if v % r else 1 for v in x]
    if n < 8:                          # one inverse, one zero
        x[n - 1] = r
        return x
    tile = min(VEC_INV_TILE, n)
    zeros = {n // 3, 0, tile - 1}
    if n >= 8:
        zeros |= {n // 2, n // 2 + 1}
    if n > VEC_INV_TILE:
        zeros |= {VEC_INV_TILE, 2 * VEC_INV_TILE - 1}
    if n >= 4 * VEC_INV_TILE:
        zeros |= set(range(2 * VEC_INV_TILE, 3 * VEC_INV_TILE))
    elif n >= 2 * VEC_INV_TILE:
        zeros |= set(range(VEC_INV_TILE, 2 * VEC_INV_TILE))
    for p in zeros:
        x[p] = 0
    x[n // 5] = r                      # a non-canonical zero
    if n >= 64:
        x[n // 7] = 2 * r if 2 * r <= TOP else r
        x[n // 7 + 1] = r + 1          # and a non-canonical one
    return x


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 8, 11, 12])
def test_batch_inverse(gpu, field, logn):
    """Part of a tile, one tile, two and four tiles against pow(x, -1, r); zeros map to 0.  Out of place from a transform buffer and
    from device words, and in place; an all-zero vector."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    x = _inverse_input(field, n, 7 * logn + len(field))
    xb = _pack(x)
    want = _pack([pow(v % r, -1, r) if v % r else 0 for v in x])
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, xb))
    assert _run(cl, NTTClient.INV, 1, 0) == want, "buffer 0 -> buffer 1"
    assert bytes(cl.result(0)) == xb
    assert _run(cl, NTTClient.INV, 0, 0) == want, "in place"
    dx = _dev(xb)
    assert _run(cl, NTTClient.INV, 0, dx) == want, "device words -> buffer 0"
    dx.free()
    cl.set_data(NTTInput(1, bytes(32 * n)))
    assert _run(cl, NTTClient.INV, 1, 1) == bytes(32 * n), "an all-zero vector"
    cl.close()


@pytest.mark.parametrize("field,logn", [("BLS381", 17), ("BLS377", 17), ("BN254", 17), ("BLS381", 20)])
def test_batch_inverse_many_tiles(gpu, field, logn):
    """128 and 1024 tiles (the totals' own inversion takes them eight to a lane: 16 and 128 lanes), in place: y is canonical and
    x y = 1 - which is unique - or y = 0 where x = 0."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    x = _words(1000 + logn, n)
    for p in (0, 1, n // 2, n - 1, 3 * VEC_INV_TILE + 5):
        x[p] = 0
    x[77] = r
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(x)))
    y = _unpack(_run(cl, NTTClient.INV, 0, 0))
    cl.close()
    assert max(y) < r
    bad = [p for p in range(n) if (x[p] * y[p] % r != 1 if x[p] % r else y[p] != 0)]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("field", ["BLS381", "BN254"])
def test_polynomial_product_and_coset_quotient(gpu, field):
    """What the ops are for.  a b = hi X^n + lo = hi (X^n - 1) + (lo + hi): on the coset g H, where X^n = g^n, the quotient's
    values are (a b - c) / (g^n - 1) with c = lo + hi - evaluate, combine, interpolate, and hi's coefficients come back; on the
    plain domain of 2n points the product of the transforms is the transform of the product.  Between the first set_data and the
    last result, everything moves by result_device / set_data_device / device-word operands."""
    logn = 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    g = GENERATOR[field]
    rng = random.Random(len(field))
    a = [rng.randrange(r) for _ in range(n)]
    b = [rng.randrange(r) for _ in range(n)]
    prod = [0] * (2 * n)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            prod[i + j] += x * y
    prod = [v % r for v in prod]
    lo, hi = prod[:n], prod[n:]
    c = [(x + y) % r for x, y in zip(lo, hi)]
    fwd, inv = _client(field, logn), _client(field, logn, inverse=True)
    fwd.set_coset(g)
    inv.set_coset(g)
    d_a, d_q = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    fwd.set_data(NTTInput(0, _pack(a)))
    _transform(fwd, 0)
    fwd.result_device(0, d_a)
    fwd.set_data(NTTInput(0, _pack(b)))
    _transform(fwd, 0)
    fwd.set_data(NTTInput(1, _pack(c)))
    _transform(fwd, 1)
    fwd.vec_op(NTTClient.MULSUB, 0, d_a, 0, 1)
    fwd.wait_result()
    fwd.vec_op(NTTClient.MUL, 0, 0, fwd.scalar(pow(pow(g, n, r) - 1, -1, r)))
    fwd.wait_result()
    fwd.result_device(0, d_q)
    inv.set_data(NTTInput(0, d_q))
    _transform(inv, 0)
    assert bytes(inv.result(0)) == _pack(hi), "the quotient by X^n - 1 on the coset"
    for cl in (fwd, inv):
        cl.close()
    # the plain domain, 2n points
    fwd, inv = _client(field, logn + 1), _client(field, logn + 1, inverse=True)
    d_a2, d_p = DeviceBuffer(0, 64 * n), DeviceBuffer(0, 64 * n)
    fwd.set_data(NTTInput(0, _pack(a + [0] * n)))
    _transform(fwd, 0)
    fwd.result_device(0, d_a2)
    fwd.set_data(NTTInput(0, _pack(b + [0] * n)))
    _transform(fwd, 0)
    fwd.vec_op(NTTClient.MUL, 0, d_a2, 0)
    fwd.wait_result()
    fwd.result_device(0, d_p)
    inv.set_data(NTTInput(1, d_p))
    _transform(inv, 1)
    assert bytes(inv.result(1)) == _pack(prod), "the product on the plain domain"
    for cl in (fwd, inv):
        cl.close()
    for d in (d_a, d_q, d_a2, d_p):
        d.free()


def test_protocol_and_refusals(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b, _ = _inputs(field, n, 5)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    one_word = _dev(bytes(32))
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def call(op, dst, x, y, z):
        return L.blz_ntt_vec_op(cl._h, op, dst, *[None if v is None else C.byref(v) for v in (x, y, z)])

    B0, B1, W = BlzVecArg(None, 0, 0, 0), BlzVecArg(None, 1, 0, n), BlzVecArg(words.ptr, 0, 0, n)
    MUL, ADD, MULADD, INV = NTTClient.MUL, NTTClient.ADD, NTTClient.MULADD, NTTClient.INV
    refused = {
        "unknown op 6": (6, 0, B0, B1, None),
        "unknown op -1": (-1, 0, B0, B1, None),
        "buf_dst 2": (MUL, 2, B0, B1, None),
        "buf 2": (MUL, 0, BlzVecArg(None, 2, 0, 0), B1, None),
        "reserved": (MUL, 0, B0, BlzVecArg(None, 1, 7, 0), None),
        "reserved, device words": (MUL, 0, B0, BlzVecArg(words.ptr, 0, 1, n), None),
        "count 0": (MUL, 0, B0, BlzVecArg(words.ptr, 0, 0, 0), None),
        "count 3": (MUL, 0, B0, BlzVecArg(words.ptr, 0, 0, 3), None),
        "count 2n": (MUL, 0, B0, BlzVecArg(words.ptr, 0, 0, 2 * n), None),
        "count of a transform buffer": (MUL, 0, B0, BlzVecArg(None, 1, 0, n // 2), None),
        "no a": (MUL, 0, None, B1, None),
        "no b": (MUL, 0, B0, None, None),
        "no c": (MULADD, 0, B0, B1, None),
        "surplus c": (ADD, 0, B0, B1, W),
        "surplus b": (INV, 0, B0, B1, None),
        "surplus c, inversion": (INV, 0, B0, None, W),
        "host memory": (MUL, 0, B0, BlzVecArg(host_ptr, 0, 0, n), None),
        "misaligned": (MUL, 0, B0, BlzVecArg(words.ptr + 8, 0, 0, 1), None),
        "past the allocation": (MUL, 0, B0, BlzVecArg(one_word.ptr, 0, 0, 2), None),
    }
    for what, args in refused.items():
        assert call(*args) == 4, what
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    # an op in flight: buffer 1 = buffer 0 x words
    cl.vec_op(MUL, 1, 0, words)
    out = bytearray(32 * n)
    for buf in (0, 1):
        for attempt in (lambda: cl.set_data(NTTInput(buf, ab)), lambda: cl.set_data(NTTInput(buf, words)),
                        lambda: cl.exchange(buf, ab, out)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam" and f"buffer {buf}" in str(ei.value)
    assert bytes(cl.result(0)) == ab                         # the operand it reads can be read
    for attempt in (lambda: cl.result(1), lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(MUL, 0, 0, words),
                    lambda: cl.vec_op(INV, 0, 0)):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want = _pack([x * y % r for x, y in zip(a, b)])
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab and cl.coset == 1
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with an op in flight: nothing is in flight afterwards, and the handle works
    cl.set_data(NTTInput(1, bb))
    cl.vec_op(INV, 1, 0)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    assert _run(cl, NTTClient.ADD, 1, 0, 1) == _pack([(x + y) % r for x, y in zip(a, b)])
    cl.close()
    words.free()
    one_word.free()
