"""Weighted (Horner) scans along a resident buffer (blz_ntt_vec_horner) on the device: dst[p] = a[p] + z dst[p -+ 1] in both
directions, inclusive and exclusive, and what it is for - division by X - z.  Every expected value is Python integer
arithmetic and every comparison is byte for byte: any 256-bit input word counts as its residue, every output word is canonical.
The input recipe is test_gpu_ntt_fold.py's: the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random 256-bit
words (more than half of them >= r) behind."""
import ctypes as C
import itertools
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_vec_util import FIELDS, GENERATOR, TOP, _client, _dev, _pack, _transform, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
EX, REV = NTTClient.HORNER_EXCLUSIVE, NTTClient.HORNER_REVERSE
EVAL, SSUM = NTTClient.FOLD_EVAL, NTTClient.SCAN_SUM
MODES = [(False, False), (True, False), (False, True), (True, True)]   # (exclusive, reverse)


def _inputs(field, n, seed):
    """The edge words first (as far as n reaches), random 256-bit words behind them."""
    r = pyref.CURVES[field]["r"]
    a = _words(seed, n)
    for i, e in enumerate([0, 1, r - 1, r, r + 1, TOP][:n]):
        a[i] = e
    return a


def _want(a, z, r, exclusive, reverse):
    """(dst, total) as Python integers: the recurrence, one step per position"""
    z %= r
    seq = a[::-1] if reverse else a
    inc = list(itertools.accumulate(seq, lambda acc, v: (acc * z + v) % r, initial=0))[1:]
    out = [0] + inc[:-1] if exclusive else inc
    return (out[::-1] if reverse else out), inc[-1]


def _run(cl, dst, a, dz, exclusive, reverse, total):
    cl.vec_horner(dst, a, dz, exclusive=exclusive, reverse=reverse, total=total)
    cl.wait_result()
    return bytes(cl.result(dst))


def test_the_expected_values_are_the_documented_sums():
    """The Python recurrence above against the closed forms of include/blaze_hip.h, 0^0 = 1 included (no device needed, but it
    is this file's reference)."""
    r = 97
    a = [5, 0, 96, 3, 1, 44, 7, 0]
    n = len(a)
    for z in (0, 1, 96, 10):
        p = lambda e: pow(z, e, r)   # noqa: E731  (pow(0, 0, r) == 1)
        assert _want(a, z, r, False, False)[0] == [sum(a[j] * p(q - j) for j in range(q + 1)) % r for q in range(n)]
        assert _want(a, z, r, True, False)[0] == [sum(a[j] * p(q - 1 - j) for j in range(q)) % r for q in range(n)]
        assert _want(a, z, r, False, True)[0] == [sum(a[j] * p(j - q) for j in range(q, n)) % r for q in range(n)]
        assert _want(a, z, r, True, True)[0] == [sum(a[j] * p(j - q - 1) for j in range(q + 1, n)) % r for q in range(n)]
        assert _want(a, z, r, True, False)[1] == sum(a[j] * p(n - 1 - j) for j in range(n)) % r
        assert _want(a, z, r, True, True)[1] == sum(a[j] * p(j) for j in range(n)) % r


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 8, 10, 11, 12])
def test_horner_against_python_integers(gpu, field, logn):
    """Fewer elements than a lane holds, a wave, one block, exactly one tile (2^10), two tiles - the carry crosses a tile edge -
    and four.  The four flag combinations; z among 0 (0^0 = 1: a copy / a shift), 1, r - 1, r + 1, a random word >= r and the
    generator; buffer 0 -> buffer 1 with d_total (the source keeps its bytes), in place without, from device words with; `a`
    periodic with 1 and 4 words.  d_total is the last inclusive value whatever the flags."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(field, n, 700 * logn + len(field))
    ab = _pack(a)
    ar = [v % r for v in a]
    cl = _client(field, logn)
    total = DeviceBuffer(0, 32)
    da = _dev(ab)
    big = next(w for w in _words(logn, 64) if w >= r)
    for k, z in enumerate((0, 1, r - 1, r + 1, big, GENERATOR[field])):
        dz = cl.scalar(z)
        for exclusive, reverse in MODES:
            want, tot = _want(ar, z, r, exclusive, reverse)
            want = _pack(want)
            what = f"{field} 2^{logn} z #{k} exclusive {exclusive} reverse {reverse}"
            cl.set_data(NTTInput(0, ab))
            total.upload(bytes(32))
            assert _run(cl, 1, 0, dz, exclusive, reverse, total) == want, what + ": buffer 0 -> buffer 1"
            assert _word(total) == tot, what
            assert bytes(cl.result(0)) == ab, what
            assert _run(cl, 0, 0, dz, exclusive, reverse, None) == want, what + ": in place, no d_total"
            total.upload(bytes(32))
            assert _run(cl, 0, da, dz, exclusive, reverse, total) == want, what + ": device words -> buffer 0"
            assert _word(total) == tot, what
        if z == 0:   # nothing is special-cased: the inclusive scan copies a, the exclusive one shifts it
            assert _want(ar, 0, r, False, True)[0] == ar and _want(ar, 0, r, True, True)[0] == ar[1:] + [0]
            assert _want(ar, 0, r, True, False)[0] == [0] + ar[:-1]
        dz.free()
    dz = cl.scalar(big)
    for count in sorted({1, min(4, n)}):
        dp = _dev(ab[:32 * count])
        per = [ar[p & (count - 1)] for p in range(n)]
        for exclusive, reverse in MODES:
            want, tot = _want(per, big, r, exclusive, reverse)
            total.upload(bytes(32))
            assert _run(cl, 1, dp, dz, exclusive, reverse, total) == _pack(want), f"{field} 2^{logn}: a of {count} words"
            assert _word(total) == tot
        dp.free()
    cl.close()
    for d in (total, da, dz):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_division_identity(gpu, field):
    """q = a div (X - z) and rem: a[k] = q[k - 1] - z q[k] (+ rem at k = 0), q[n - 1] = 0, and rem is byte-equal to what
    vec_reduce(EVAL) writes for the same a and z."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(field, n, 1100 + len(field))
    z = next(w for w in _words(5, 64) if w >= r)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(a)))
    dz = cl.scalar(z)
    rem = DeviceBuffer(0, 32)
    cl.vec_divide(1, 0, dz, rem)
    cl.wait_result()
    q = _unpack(cl.result(1))
    y = cl.vec_reduce(EVAL, 0, dz)
    cl.wait_result()
    assert bytes(rem.download(32)) == bytes(y.download(32))
    rm = _word(rem)
    assert all(v < r for v in q) and rm < r and q[n - 1] == 0
    assert (rm - z * q[0] - a[0]) % r == 0
    for k in range(1, n):
        assert (q[k - 1] - z * q[k] - a[k]) % r == 0, k
    cl.close()
    for d in (dz, rem, y):
        d.free()


def test_z_one_is_a_sum_scan(gpu):
    """Forward with z = 1 equals vec_scan(SCAN_SUM) byte for byte, inclusive and exclusive; reverse equals the suffix sums."""
    field, logn = "BLS377", 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(field, n, 1111)
    ar = [v % r for v in a]
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(a)))
    one = cl.scalar(1)
    t1, t2 = DeviceBuffer(0, 32), DeviceBuffer(0, 32)
    for exclusive in (False, True):
        got = _run(cl, 1, 0, one, exclusive, False, t1)
        cl.vec_scan(SSUM, 1, 0, exclusive=exclusive, total=t2)
        cl.wait_result()
        assert got == bytes(cl.result(1)), exclusive
        assert bytes(t1.download(32)) == bytes(t2.download(32))
        suffix = list(itertools.accumulate(reversed(ar), lambda x, y: (x + y) % r))[::-1]
        want = suffix[1:] + [0] if exclusive else suffix
        assert _run(cl, 1, 0, one, exclusive, True, t1) == _pack(want), exclusive
        assert _word(t1) == sum(ar) % r
    cl.close()
    for d in (one, t1, t2):
        d.free()


def test_second_level_of_the_totals(gpu):
    """2^21 elements are 2048 tiles of 1024: the tiles' totals are themselves scanned in two tiles with a second level of two
    totals above them, whose multiplier is z^(2^20).  BLS12-381 only: the division in place with d_total against a Python Horner
    loop, and the forward inclusive run at the same size, whose last word is its d_total."""
    field, logn = "BLS381", 21
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _words(2121, n)
    z = a[77]
    assert z >= 1 << 200
    ab = _pack(a)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    dz = cl.scalar(z)
    total = DeviceBuffer(0, 32)
    got = _run(cl, 0, 0, dz, True, True, total)
    want, tot = _want([v % r for v in a], z, r, True, True)
    assert got == _pack(want)
    assert _word(total) == tot
    cl.set_data(NTTInput(0, ab))
    got = _run(cl, 1, 0, dz, False, False, total)
    want, tot = _want([v % r for v in a], z, r, False, False)
    assert got == _pack(want)
    assert got[-32:] == bytes(total.download(32)) and _word(total) == tot
    cl.close()
    for d in (dz, total):
        d.free()


@pytest.mark.parametrize("field", ["BLS381", "BN254"])
def test_opening_pipeline(gpu, field):
    """What the op is for.  Evaluations of a random f on H -> inverse transform -> EVAL at z gives y -> vec_divide gives q ->
    forward transform of q; on the host, for every i, q^[i] (w^i - z) = f^[i] - y, w = g^((r - 1) / n) the documented default
    root.  Between the first set_data and the last result everything stays on the device."""
    logn = 12
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 12)
    fhat = [rng.randrange(r) for _ in range(n)]
    z = rng.randrange(r)
    inv = _client(field, logn, inverse=True)
    inv.set_data(NTTInput(0, _pack(fhat)))
    _transform(inv, 0)
    coeffs = DeviceBuffer(0, 32 * n)
    inv.result_device(0, coeffs)
    inv.close()
    cl = _client(field, logn)
    dz = cl.scalar(z)
    y = cl.vec_reduce(EVAL, coeffs, dz)
    cl.wait_result()
    rem = DeviceBuffer(0, 32)
    cl.vec_divide(0, coeffs, dz, rem)
    cl.wait_result()
    assert bytes(rem.download(32)) == bytes(y.download(32))
    _transform(cl, 0)
    qhat = _unpack(cl.result(0))
    yv = _word(y)
    w = pow(GENERATOR[field], (r - 1) >> logn, r)
    wi = 1
    for i in range(n):
        assert (qhat[i] * (wi - z) - (fhat[i] - yv)) % r == 0, i
        wi = wi * w % r
    cl.close()
    for d in (coeffs, dz, y, rem):
        d.free()


def test_protocol_and_refusals(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(field, n, 5), _inputs(field, n, 6)
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

    def horner(flags, dst, x, z, t):
        return L.blz_ntt_vec_horner(cl._h, flags, dst, ref(x), ref(z), t)

    B0, B1, W, Z = BlzVecArg(None, 0, 0, 0), BlzVecArg(None, 1, 0, n), BlzVecArg(words.ptr, 0, 0, n), BlzVecArg(one_word.ptr, 0, 0, 1)
    refused = {
        "flag bit 2": lambda: horner(4, 0, B0, Z, None),
        "flag bit 31": lambda: horner(0x80000000, 0, B0, Z, None),
        "flag bit 2 beside the known ones": lambda: horner(7, 0, B0, Z, None),
        "buf_dst 2": lambda: horner(0, 2, B0, Z, None),
        "no a": lambda: horner(0, 0, None, Z, None),
        "no z": lambda: horner(3, 0, B0, None, None),
        "z names a transform buffer": lambda: horner(3, 0, B0, B1, None),
        "z of two words": lambda: horner(0, 0, B0, BlzVecArg(words.ptr, 0, 0, 2), None),
        "z of n words": lambda: horner(0, 0, B0, W, None),
        "z in host memory": lambda: horner(0, 0, B0, BlzVecArg(host_ptr, 0, 0, 1), None),
        "z misaligned": lambda: horner(0, 0, B0, BlzVecArg(one_word.ptr + 8, 0, 0, 1), None),
        "z reserved": lambda: horner(0, 0, B0, BlzVecArg(one_word.ptr, 0, 3, 1), None),
        "d_total in host memory": lambda: horner(0, 0, B0, Z, host_ptr),
        "d_total misaligned": lambda: horner(1, 0, B0, Z, out.ptr + 4),
        "d_total runs past its allocation": lambda: horner(2, 0, B0, Z, out.ptr + 48),
        "d_total on z": lambda: horner(3, 0, B0, Z, one_word.ptr),
        "d_total on a's words": lambda: horner(3, 1, W, Z, words.ptr + 64),
        "a: buf 2": lambda: horner(0, 0, BlzVecArg(None, 2, 0, 0), Z, None),
        "a: reserved": lambda: horner(0, 0, BlzVecArg(None, 0, 1, 0), Z, None),
        "a: count 0": lambda: horner(0, 0, BlzVecArg(words.ptr, 0, 0, 0), Z, None),
        "a: count 3": lambda: horner(0, 0, BlzVecArg(words.ptr, 0, 0, 3), Z, None),
        "a: count 2n": lambda: horner(0, 0, BlzVecArg(words.ptr, 0, 0, 2 * n), Z, None),
        "a: count of a transform buffer": lambda: horner(0, 0, BlzVecArg(None, 1, 0, n // 2), Z, None),
        "a in host memory": lambda: horner(0, 0, BlzVecArg(host_ptr, 0, 0, n), Z, None),
        "a misaligned": lambda: horner(0, 0, BlzVecArg(words.ptr + 8, 0, 0, 1), Z, None),
        "a past its allocation": lambda: horner(0, 0, BlzVecArg(one_word.ptr, 0, 0, 2), Z, None),
    }
    for what, attempt in refused.items():
        assert attempt() == 4, what
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and _word(one_word) == 7 and bytes(out.download()) == mark
    # the op in flight: buffer 1 = buffer 0 divided by X - 7
    busy = (lambda: cl.start_process(1), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words),
            lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 1), lambda: cl.vec_scan(SSUM, 1, 1), lambda: cl.vec_horner(1, 1, one_word),
            lambda: cl.vec_divide(0, 0, one_word))
    sink = bytearray(32 * n)
    rem = DeviceBuffer(0, 32)
    cl.vec_divide(1, 0, one_word, rem)
    for buf in (0, 1):
        for attempt in (lambda: cl.set_data(NTTInput(buf, ab)), lambda: cl.exchange(buf, ab, sink)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam" and f"buffer {buf}" in str(ei.value)
    assert bytes(cl.result(0)) == ab          # the buffer it only reads can be read
    for attempt in busy + (lambda: cl.result(1),):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want, tot = _want([v % r for v in a], 7, r, True, True)
    want = _pack(want)
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab and _word(rem) == tot and cl.coset == 1
    assert _word(one_word) == 7
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with the op in flight: nothing is in flight afterwards, and the handle works
    cl.vec_horner(1, 0, one_word, reverse=True)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    assert _run(cl, 1, 0, one_word, True, True, rem) == want and _word(rem) == tot
    cl.close()
    for d in (words, one_word, out, rem):
        d.free()
