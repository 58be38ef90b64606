"""Gathers on resident buffers (blz_ntt_vec_gather) on the device: dst[p] = a[(offset + stride p) mod count] for p < len and 0
above, from a transform buffer or from device words that may be longer than the handle, out of place and in place - and what
the op is for: the rotation, the extension, the slice and the decimation of a PLONK-style quotient.  Every expected value is
Python integer arithmetic and every comparison is byte for byte: any 256-bit source word counts as its residue, every output
word is canonical.  The input recipe is the house one: the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random
256-bit words (more than half of them >= r) behind."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg, BlzVecView
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_vec_util import FIELDS, GENERATOR, TOP, _client, _dev, _pack, _transform, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
MUL, MULSUB, EVAL, SSUM = NTTClient.MUL, NTTClient.MULSUB, NTTClient.FOLD_EVAL, NTTClient.SCAN_SUM


def _inputs(field, count, seed):
    """The edge words first (as far as count reaches), random 256-bit words behind them."""
    r = pyref.CURVES[field]["r"]
    a = _words(seed, count)
    for i, e in enumerate([0, 1, r - 1, r, r + 1, TOP][:count]):
        a[i] = e
    return a


def _want(a, r, n, off, s, length):
    """The documented formula on Python integers, packed: a[(off + s p) % count] % r below length, 0 from there to n"""
    count = len(a)
    return _pack([a[(off + s * p) % count] % r if p < length else 0 for p in range(n)])


def _gather(cl, dst, a, off, s, length):
    cl.vec_gather(dst, a, offset=off, stride=s, length=length)
    cl.wait_result()
    return bytes(cl.result(dst))


def _buffer_views(n):
    """(offset, stride, len) on a source of n words: identity; rotations by 1, n - 1 and n / 2; the reversal; a broadcast; an
    odd stride (a permutation); stride 2 (wraps, reads every word it reads twice); len among 0, 1, n / 2 + 1, n - 1, n."""
    views = [(0, 1, n), (1, 1, n), (n - 1, 1, n), (n // 2, 1, n), (n - 1, n - 1, n), (n - 1, 0, n), (1, 3, n), (1, 2, n)]
    views += [(1, 1, ln) for ln in (0, 1, n // 2 + 1, n - 1)] + [(n - 1, n - 1, n // 2 + 1), (1, 3, n - 1)]
    return list(dict.fromkeys(views))


def test_the_quotient_identity_on_naive_transforms():
    """What test_quotient_round_trip runs on the device, at n = 8 with naive DFTs on Python integers (no device needed, but it is
    that test's reference): with z the default 4n-th root, w = z^4, F[p] = f(g z^p) and H[p] = h(g z^p), the rotation by 4 is
    f(w X) on the coset, 1 / Z_H has period 4 along the position, and the quotient's coefficients n - 1 .. 4n - 1 vanish."""
    n, logn = 8, 3
    for field in FIELDS:
        r = pyref.CURVES[field]["r"]
        gen = GENERATOR[field]
        g = 7 if gen == 5 else gen
        w, zt = pow(gen, (r - 1) >> logn, r), pow(gen, (r - 1) >> (logn + 2), r)
        assert pow(zt, 4, r) == w
        rng = random.Random(8)
        f = [rng.randrange(r) for _ in range(n)]
        h = [f[p] * f[(p + 1) % n] % r for p in range(n)]

        def idft(v, root, m):
            ri, mi = pow(root, r - 2, r), pow(m, r - 2, r)
            return [mi * sum(v[k] * pow(ri, i * k, r) for k in range(m)) % r for i in range(m)]

        fc, hc = idft(f, w, n), idft(h, w, n)
        ev = lambda c, x: sum(ci * pow(x, i, r) for i, ci in enumerate(c)) % r   # noqa: E731
        F = [ev(fc, g * pow(zt, p, r) % r) for p in range(4 * n)]
        H = [ev(hc, g * pow(zt, p, r) % r) for p in range(4 * n)]
        zh = [pow((pow(g, n, r) * pow(zt, n * p, r) - 1) % r, r - 2, r) for p in range(4)]
        T = [(F[p] * F[(p + 4) % (4 * n)] - H[p]) * zh[p & 3] % r for p in range(4 * n)]
        gi = pow(g, r - 2, r)
        t = [c * pow(gi, i, r) % r for i, c in enumerate(idft(T, zt, 4 * n))]
        assert not any(t[n - 1:]) and any(t[:n - 1])
        z = rng.randrange(r)
        assert (ev(fc, z) * ev(fc, w * z % r) - ev(hc, z)) % r == ev(t, z) * (pow(z, n, r) - 1) % r
        assert [ev(fc, pow(zt, 4 * p, r)) for p in range(n)] == f


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 8, 11])
def test_views_against_python_integers(gpu, field, logn):
    """Fewer positions than a wave, a wave, a block, several blocks.  Every view of _buffer_views on a transform-buffer source,
    buffer 0 -> buffer 1 (buffer 0 keeps its bytes), then in place with the same bytes out; then device words of every count
    the handle takes - 1 and 4 tiled, n / 2 with the upper half zeroed over a buffer that held non-zero words and then tiled
    twice, n, and 4n sliced and decimated."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(field, n, 900 * logn + len(field))
    ab = _pack(a)
    fill = _pack([v | 1 for v in _words(logn + 40, n)])   # no zero word: a position the op must zero shows
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    for off, s, ln in _buffer_views(n):
        what = f"{field} 2^{logn} offset {off} stride {s} len {ln}"
        want = _want(a, r, n, off, s, ln)
        cl.set_data(NTTInput(1, fill))
        assert _gather(cl, 1, 0, off, s, ln) == want, what + ": buffer 0 -> buffer 1"
        assert bytes(cl.result(0)) == ab, what
        cl.set_data(NTTInput(1, ab))
        assert _gather(cl, 1, 1, off, s, ln) == want, what + ": in place"
    assert bytes(cl.result(0)) == ab
    big = _inputs(field, 4 * n, 901 * logn + len(field))
    cases = [(1, 0, 1, n), (1, 0, 0, n), (4, 0, 1, n), (4, 3, 1, n), (n // 2, 0, 1, n // 2), (n // 2, 0, 1, n), (n, 0, 1, n), (n, n - 1, n - 1, n),
             (4 * n, n + 1, 1, n), (4 * n, 3, 4, n), (4 * n, 4 * n - 1, 4 * n - 1, n - 1)]
    for count, off, s, ln in dict.fromkeys(cases):
        src = big[:count]
        d = _dev(_pack(src))
        what = f"{field} 2^{logn}: {count} device words, offset {off} stride {s} len {ln}"
        cl.set_data(NTTInput(1, fill))
        assert _gather(cl, 1, d, off, s, ln) == _want(src, r, n, off, s, ln), what
        assert bytes(d.download()) == _pack(src), what
        d.free()
    assert bytes(cl.result(0)) == ab
    cl.close()


def test_second_turn_of_the_grid_stride_loop(gpu):
    """2^20 positions are two sweeps of the 2048 x 256 launch grid.  BLS12-381 only, both kernels, sources of n and of 4n
    words: a rotation (contiguous source), the reversal (strided), the rotation in place cut at len = n / 2 + 1 - the first
    position of the second sweep is the last that reads - and from 2^22 device words the slice and the decimation."""
    field, logn = "BLS381", 20
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a = _inputs(field, n, 2020)
    ar = [v % r for v in a]
    ab = _pack(a)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    assert _gather(cl, 1, 0, 1, 1, n) == _pack(ar[1:] + ar[:1])
    assert _gather(cl, 1, 0, n - 1, -1, n) == _pack(ar[::-1])
    assert bytes(cl.result(0)) == ab
    assert _gather(cl, 0, 0, 1, 1, n // 2 + 1) == _pack(ar[1:n // 2 + 2]) + bytes(32 * (n // 2 - 1))
    raw = random.Random(2021).randbytes(32 * 4 * n)
    d = _dev(raw)
    word = lambda i: int.from_bytes(raw[32 * i: 32 * i + 32], "little") % r   # noqa: E731
    assert _gather(cl, 1, d, n + 1, 1, n) == _pack([word(n + 1 + p) for p in range(n)])
    assert _gather(cl, 1, d, 3, 4, None) == _pack([word(3 + 4 * p) for p in range(n)])
    d.free()
    cl.close()


def test_protocol(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b = _inputs(field, n, 15), _inputs(field, n, 16)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    busy = (lambda: cl.start_process(1), lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(MUL, 1, 1, words),
            lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 1), lambda: cl.vec_scan(SSUM, 1, 1), lambda: cl.vec_horner(1, 1, one_word),
            lambda: cl.vec_gather(1, words), lambda: cl.vec_rotate(0, 0, 1), lambda: cl.vec_extend(1, one_word))
    sink = bytearray(32 * n)
    cl.vec_rotate(1, 0, -3)   # buffer 1 = buffer 0 rotated: enqueued, not waited for
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
    want = _want(a, r, n, n - 3, 1, n)
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab and cl.coset == 1
    with pytest.raises(DriverClientError):   # nothing is in flight any more
        cl.wait_result()
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with a gather in flight (in place: the kernel and the copy back): nothing is in flight afterwards, and the handle works
    cl.vec_gather(0, 0, offset=-1, stride=-1)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    assert _gather(cl, 1, 0, n - 3, 1, n) == want
    cl.vec_extend(1, one_word)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([7] + [0] * (n - 1))
    cl.close()
    for d in (words, one_word):
        d.free()


def test_refusals(gpu):
    field, logn = "BN254", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(field, n, 25), _inputs(field, n, 26)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def gather(dst, x, v):
        return L.blz_ntt_vec_gather(cl._h, dst, None if x is None else C.byref(x), None if v is None else C.byref(v))

    B0, W, ALL = BlzVecArg(None, 0, 0, 0), BlzVecArg(words.ptr, 0, 0, n), BlzVecView(0, 1, n)
    refused = {
        "no a": lambda: gather(1, None, ALL),
        "no view": lambda: gather(1, B0, None),
        "neither": lambda: gather(1, None, None),
        "buf_dst 2": lambda: gather(2, B0, ALL),
        "offset = count, a buffer": lambda: gather(1, B0, BlzVecView(n, 1, n)),
        "offset = count, device words": lambda: gather(1, BlzVecArg(words.ptr, 0, 0, 4), BlzVecView(4, 1, n)),
        "offset = count = 1": lambda: gather(1, BlzVecArg(one_word.ptr, 0, 0, 1), BlzVecView(1, 0, n)),
        "offset 2^64 - 1": lambda: gather(1, W, BlzVecView(TOP >> 192, 1, n)),
        "len = n + 1": lambda: gather(1, B0, BlzVecView(0, 1, n + 1)),
        "len 2^63": lambda: gather(1, W, BlzVecView(0, 1, 1 << 63)),
        "count 3": lambda: gather(1, BlzVecArg(words.ptr, 0, 0, 3), ALL),
        "count 0": lambda: gather(1, BlzVecArg(words.ptr, 0, 0, 0), ALL),
        "count 2^28": lambda: gather(1, BlzVecArg(words.ptr, 0, 0, 1 << 28), ALL),
        "count of a transform buffer": lambda: gather(1, BlzVecArg(None, 0, 0, 4 * n), ALL),
        "reserved = 1": lambda: gather(1, BlzVecArg(None, 0, 1, 0), ALL),
        "reserved = 1, device words": lambda: gather(1, BlzVecArg(words.ptr, 0, 1, n), ALL),
        "buf = 2": lambda: gather(1, BlzVecArg(None, 2, 0, 0), ALL),
        "d_ptr misaligned": lambda: gather(1, BlzVecArg(words.ptr + 8, 0, 0, 1), ALL),
        "a host pointer": lambda: gather(1, BlzVecArg(host_ptr, 0, 0, n), ALL),
        "4n words in an allocation of n": lambda: gather(1, BlzVecArg(words.ptr, 0, 0, 4 * n), ALL),
        "two words in an allocation of one": lambda: gather(1, BlzVecArg(one_word.ptr, 0, 0, 2), ALL),
    }
    for what, attempt in refused.items():
        assert attempt() == 4, what
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb and _word(one_word) == 7
    # the raised bound is the gather's alone: the other ops still stop at n
    big = _dev(bytes(32 * 2 * n))
    with pytest.raises(DriverClientError):
        cl.vec_op(MUL, 1, 0, big)
    # the handle is as usable as before
    assert _gather(cl, 1, big, 0, 1, None) == bytes(32 * n)
    assert _gather(cl, 1, 0, 0, 1, n) == _pack([v % r for v in a])
    assert gather(1, W, BlzVecView(n - 1, TOP >> 192, n)) == 0   # stride 2^64 - 1 is -1 modulo every count
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([v % r for v in b][::-1])
    cl.close()
    for d in (words, one_word, big):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_quotient_round_trip(gpu, field):
    """The four steps of a PLONK-style quotient that needed the host.  f random on H (n = 2^9); h[p] = f[p] f[p + 1] with the
    neighbour a vec_rotate by 1; both interpolated, extended into a 4n handle (vec_extend: zero from n up), evaluated on the
    coset g<zeta>; f(w X) on the coset is F rotated by 4 (zeta^4 = w with the default roots); T = (F F_rot - H) / Z_H with
    1 / Z_H four device words; interpolated back, t has degree n - 2.  Its low n coefficients return to an n handle as a slice
    of the 4n device words, and f(z) f(w z) - h(z) = t(z) (z^n - 1) at a random z, every evaluation an EVAL on the device.
    Between the first set_data and the downloads of the checks everything stays on the device."""
    logn = 9
    n, n4 = 1 << logn, 4 << logn
    r = pyref.CURVES[field]["r"]
    gen = GENERATOR[field]
    g = 7 if gen == 5 else gen
    w, zeta = pow(gen, (r - 1) >> logn, r), pow(gen, (r - 1) >> (logn + 2), r)
    rng = random.Random(len(field) + 9)
    f = [rng.randrange(r) for _ in range(n)]
    z = rng.randrange(r)
    inv_n, fwd_n = _client(field, logn, inverse=True), _client(field, logn)
    fwd_4n, inv_4n = _client(field, logn + 2), _client(field, logn + 2, inverse=True)
    fwd_4n.set_coset(g)
    inv_4n.set_coset(g)
    # h = f(X) f(w X) on H, then both interpolated
    inv_n.set_data(NTTInput(0, _pack(f)))
    inv_n.vec_rotate(1, 0, 1)
    inv_n.wait_result()
    assert bytes(inv_n.result(1)) == _pack(f[1:] + f[:1])
    inv_n.vec_op(MUL, 1, 0, 1)
    inv_n.wait_result()
    _transform(inv_n, 0)
    _transform(inv_n, 1)
    fc, hc = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
    inv_n.result_device(0, fc)
    inv_n.result_device(1, hc)
    # low-degree extension and evaluation on the coset
    for buf, d in ((0, fc), (1, hc)):
        fwd_4n.vec_extend(buf, d)
        fwd_4n.wait_result()
        ext = bytes(fwd_4n.result(buf))
        assert ext[:32 * n] == bytes(d.download()) and ext[32 * n:] == bytes(32 * (n4 - n))
        _transform(fwd_4n, buf)
    H = DeviceBuffer(0, 32 * n4)
    fwd_4n.result_device(1, H)
    fwd_4n.vec_rotate(1, 0, 4)
    fwd_4n.wait_result()
    zh = _dev(_pack([pow((pow(g, n, r) * pow(zeta, n * p, r) - 1) % r, r - 2, r) for p in range(4)]))
    fwd_4n.vec_op(MULSUB, 0, 0, 1, H)
    fwd_4n.wait_result()
    fwd_4n.vec_op(MUL, 0, 0, zh)
    fwd_4n.wait_result()
    T = DeviceBuffer(0, 32 * n4)
    fwd_4n.result_device(0, T)
    inv_4n.set_data(NTTInput(0, T))
    _transform(inv_4n, 0)
    t = _unpack(inv_4n.result(0))
    assert not any(t[n - 1:]) and any(t[:n - 1])
    # the low n coefficients back into an n handle: a slice of 4n device words
    inv_4n.result_device(0, T)
    fwd_n.vec_gather(0, T, offset=0, stride=1, length=n)
    fwd_n.wait_result()
    assert bytes(fwd_n.result(0)) == _pack(t[:n])
    dz, dwz = fwd_n.scalar(z), fwd_n.scalar(w * z % r)
    vals = []
    for src, point in ((0, dz), (fc, dz), (fc, dwz), (hc, dz)):
        y = fwd_n.vec_reduce(EVAL, src, point)
        fwd_n.wait_result()
        vals.append(_word(y))
        y.free()
    tz, fz, fwz, hz = vals
    assert (fz * fwz - hz) % r == tz * (pow(z, n, r) - 1) % r
    # the values on H out of the plain evaluation on the 4n domain: every 4th position
    fwd_4n.set_coset(None)
    fwd_4n.vec_extend(0, fc)
    fwd_4n.wait_result()
    _transform(fwd_4n, 0)
    fwd_4n.result_device(0, T)
    fwd_n.vec_gather(1, T, stride=4)
    fwd_n.wait_result()
    assert bytes(fwd_n.result(1)) == _pack(f)
    for c in (inv_n, fwd_n, fwd_4n, inv_4n):
        c.close()
    for d in (fc, hc, H, zh, T, dz, dwz):
        d.free()


def test_reversal_turns_a_forward_scan_into_the_division(gpu):
    """The reversal has a caller: reverse, a forward exclusive vec_horner, reverse again equals vec_divide of the same vector."""
    field, logn = "BLS377", 11
    n = 1 << logn
    a = _inputs(field, n, 1177)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(a)))
    dz = cl.scalar(_words(6, 1)[0])
    cl.vec_divide(1, 0, dz)
    cl.wait_result()
    q = bytes(cl.result(1))
    cl.vec_gather(1, 0, offset=n - 1, stride=n - 1)
    cl.wait_result()
    cl.vec_horner(1, 1, dz, exclusive=True)
    cl.wait_result()
    cl.vec_gather(1, 1, offset=-1, stride=-1)
    cl.wait_result()
    assert bytes(cl.result(1)) == q and any(q)
    cl.close()
    dz.free()
