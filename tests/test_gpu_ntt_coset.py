"""Coset transforms on the device (blz_ntt_set_coset): X[k] = sum_i x[i] g^i w^(i k) on a forward handle, its exact inverse
x[i] = g^-i n^-1 sum_k X[k] w^(-i k) on an inverse one, fused into the transform's passes.  The expected output is the oracle's
plain transform of the input pre-multiplied by g^i in Python integers (forward) / the oracle's inverse post-multiplied by g^-i."""
import os
import random
import statistics

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd.driver_client import DriverClient
from blaze_amd.ingo_ntt import NTT, NTTClient, NTTInput, NttInit
from oracle import pyref

pytestmark = pytest.mark.gpu
GENERATOR = {"BLS381": 7, "BLS377": 22, "BN254": 5}   # the fields' multiplicative generators
FIELDS = ["BLS381", "BLS377", "BN254"]
THREADS = 16


def _ntt(cl, data, buf=0):
    cl.set_data(NTTInput(buf, data))
    cl.initialize(NttInit())
    cl.start_process(buf)
    cl.wait_result()
    return bytes(cl.result(buf))


def _random_input(seed, n):
    import numpy as np
    x = np.random.default_rng(seed).integers(0, 256, size=32 * n, dtype=np.uint8).reshape(n, 32)
    x[:, 31] &= 0x0F   # < 2^252 < r of all three fields: canonical
    return x.tobytes()


def _column(r, g, n):
    col, p = [1] * n, 1
    for i in range(1, n):
        p = p * g % r
        col[i] = p
    return col


def _scaled(data, col, r):
    return b"".join((int.from_bytes(data[32 * i: 32 * i + 32], "little") * c % r).to_bytes(32, "little") for i, c in enumerate(col))


def _flags(inv, brin, brout):
    return (NTTClient.INVERSE if inv else 0) | (NTTClient.BITREV_INPUT if brin else 0) | (NTTClient.BITREV_OUTPUT if brout else 0)


def _random_shift(field, seed):
    r = pyref.CURVES[field]["r"]
    s = random.Random(seed).getrandbits(255) % r
    return s if s > 1 else 3


def _check_orders(orc, field, logn, shift, x, orders, directions, root=None):
    """One g^i column per (field, size, shift) and one oracle transform per direction; the bit-reversed orders' buffers and
    expectations are permutations of the natural ones (the power of g follows the element)."""
    r = pyref.CURVES[field]["r"]
    n = 1 << logn
    col = _column(r, shift, n)
    for inv in directions:
        if not inv:
            want = bytes(orc.ntt(field, _scaled(x, col, r), logn, threads=THREADS, root=root))
        else:
            icol = _column(r, pow(shift, -1, r), n)
            want = _scaled(bytes(orc.ntt(field, x, logn, inverse=True, threads=THREADS, root=root)), icol, r)
        for brin, brout in orders:
            cl = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, field=field, flags=_flags(inv, brin, brout), root=root)
            cl.set_coset(shift)
            assert cl.coset == shift
            src = bytes(orc.bitrev_permute(x, logn, THREADS)) if brin else x
            exp = bytes(orc.bitrev_permute(want, logn, THREADS)) if brout else want
            got = _ntt(cl, src, buf=int(inv))
            cl.close()
            assert got == exp, f"{field} 2^{logn} shift={shift:#x} inverse={inv} bitrev_in={brin} bitrev_out={brout}"


ALL_ORDERS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 4, 9, 10, 12])
def test_small_sizes_against_the_oracle(gpu, orc, field, logn):
    """One and two passes of the radix-2-in-LDS kernel (the wire pass is pass 3 up to 2^9, pass 2 from 2^10): the field's generator
    and a random 255-bit shift, forward and inverse, the four buffer orders."""
    x = _random_input(1000 + logn, 1 << logn)
    for shift in (GENERATOR[field], _random_shift(field, 31 * logn + len(field))):
        _check_orders(orc, field, logn, shift, x, ALL_ORDERS, (False, True))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [18, 19, 20])
def test_512_point_sizes_against_the_oracle(gpu, orc, field, logn):
    """2^18: pass 2 of the 512-point kernel is the wire pass; 2^19: three passes, the radix-2 kernel first and last; 2^20: pass 3
    of the 512-point kernel closes the inverse transform and pass 2 carries the rest of its shift.  BLS12-381 in all eight
    direction / order combinations, the other two fields forward and inverse in natural order."""
    x = _random_input(2000 + logn, 1 << logn)
    orders = ALL_ORDERS if field == "BLS381" else ALL_ORDERS[:1]
    _check_orders(orc, field, logn, GENERATOR[field], x, orders, (False, True))


@pytest.mark.parametrize("logn", [12, 18])
def test_non_canonical_words_and_callers_root(gpu, orc, logn):
    """Any 256-bit word is a residue (test_gpu_ntt.py test_non_canonical_words): x + k r must transform like x under a shift too -
    the product on the element as loaded sees the stray word.  And the shift composes with a caller's root."""
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    rng = random.Random(77 + logn)
    n = 1 << logn
    kmax = ((1 << 256) - 1) // r
    base = []
    for i in range(1024):
        v = rng.randrange(r)
        k = rng.randrange(kmax + 1)
        if v + k * r >= 1 << 256:
            k -= 1
        base.append((v, v + k * r))
    base.append(((1 << 256) - 1 - kmax * r, (1 << 256) - 1))
    base.append((0, kmax * r))
    canon = b"".join(base[(i * 5 + i // 1024) % len(base)][0].to_bytes(32, "little") for i in range(n))
    stray = b"".join(base[(i * 5 + i // 1024) % len(base)][1].to_bytes(32, "little") for i in range(n))
    shift = GENERATOR[field]
    col = _column(r, shift, n)
    want = bytes(orc.ntt(field, _scaled(canon, col, r), logn, threads=THREADS))
    cl = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, field=field)
    cl.set_coset(shift)
    assert _ntt(cl, canon) == want
    assert _ntt(cl, stray, buf=1) == want
    cl.close()
    root = pow(orc.omega(field, logn), 3, r)
    _check_orders(orc, field, logn, shift, _random_input(5 + logn, n), [(False, False), (True, True)], (False, True), root=root)


@pytest.mark.parametrize("logn", [12, 20])
def test_setter_semantics(gpu, orc, logn):
    """plain -> g -> plain gives today's bytes at both ends; g -> g' switches; get_coset reports each; shift 1 equals NULL;
    inverse(g) o forward(g) is the identity; refused values and a call while a transform is in flight are InvalidPrimitiveParam
    and change nothing; reset keeps g; both buffers hold their data across a set_coset."""
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    n = 1 << logn
    g, g2 = GENERATOR[field], _random_shift(field, 4242)
    x = _random_input(3000 + logn, n)
    x2 = _random_input(3001 + logn, n)
    fwd = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, field=field)
    inv = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, field=field, inverse=True)
    plain = bytes(orc.ntt(field, x, logn, threads=THREADS))
    plain_inv = bytes(orc.ntt(field, x, logn, inverse=True, threads=THREADS))
    want_g = bytes(orc.ntt(field, _scaled(x, _column(r, g, n), r), logn, threads=THREADS))
    want_g2 = bytes(orc.ntt(field, _scaled(x, _column(r, g2, n), r), logn, threads=THREADS))
    assert fwd.coset == 1 and inv.coset == 1
    assert _ntt(fwd, x) == plain and _ntt(inv, x) == plain_inv
    fwd.set_coset(g); inv.set_coset(g)
    assert fwd.coset == g and inv.coset == g
    y = _ntt(fwd, x)
    assert y == want_g
    assert _ntt(inv, y) == x, "inverse(g) o forward(g) is not the identity"
    # refused values change nothing
    for bad in (0, r, (1 << 256) - 1):
        for cl in (fwd, inv):
            with pytest.raises(DriverClientError) as ei:
                cl.set_coset(bad)
            assert ei.value.variant == "InvalidPrimitiveParam", bad
            assert cl.coset == g
    assert _ntt(fwd, x) == want_g and _ntt(inv, y) == x
    # a transform in flight: refused, and the transform still equals the oracle
    fwd.set_data(NTTInput(0, x))
    fwd.start_process(0)
    with pytest.raises(DriverClientError) as ei:
        fwd.set_coset(g2)
    assert ei.value.variant == "InvalidPrimitiveParam"
    fwd.wait_result()
    assert bytes(fwd.result(0)) == want_g and fwd.coset == g
    # reset keeps the shift
    fwd.reset()
    assert fwd.coset == g and _ntt(fwd, x) == want_g
    # both buffers hold their data across a set_coset
    fwd.set_data(NTTInput(0, x)); fwd.set_data(NTTInput(1, x2))
    fwd.set_coset(g2)
    assert fwd.coset == g2
    assert bytes(fwd.result(0)) == x and bytes(fwd.result(1)) == x2
    assert _ntt(fwd, x) == want_g2
    inv.set_coset(g2)
    assert _ntt(inv, want_g2) == x
    # shift 1 equals NULL equals the plain transform, byte for byte
    fwd.set_coset(1); inv.set_coset(1)
    assert fwd.coset == 1 and _ntt(fwd, x) == plain and _ntt(inv, x) == plain_inv
    fwd.set_coset(g); inv.set_coset(g)
    fwd.set_coset(None); inv.set_coset(None)
    assert inv.coset == 1 and _ntt(fwd, x, buf=1) == plain and _ntt(inv, x, buf=1) == plain_inv
    fwd.close(); inv.close()
    assert blaze_amd.lib().blz_ntt_set_coset(None, None) == 4


# ---- full size: 2^27 BLS12-381
_FULL = {}


def _full_input(orc):
    """The device-made input (kept on the host) and the ONE full-size oracle transform of this file: the plain natural-order one."""
    import numpy as np
    if "x" not in _FULL:
        n = 1 << 27
        d_in = DeviceBuffer(0, 32 * n)
        blaze_amd._lib.check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n, 2718))
        _FULL["x"] = np.frombuffer(d_in.download(), dtype=np.uint8)
        d_in.free()
        threads = max(1, min(64, (os.cpu_count() or 8)))
        _FULL["X"] = np.frombuffer(orc.ntt("BLS381", _FULL["x"], 27, threads=threads), dtype=np.uint8)
    return _FULL["x"], _FULL["X"]


def _run_dev(cl, src, buf=0):
    import numpy as np
    cl.set_data(NTTInput(buf, src)); cl.initialize(NttInit()); cl.start_process(buf); cl.wait_result()
    return np.frombuffer(cl.result(buf), dtype=np.uint8)


@pytest.mark.parametrize("pass2", ["factor_table", "stepped"])
def test_full_size_2e27(gpu, orc, pass2):
    """Both pass-2 kernels, forward and inverse handle.  Shift g = w^j (j with a non-zero digit in each of its three 9-bit
    fields): the coset output is the plain output rotated, Y[k] = X[(k + j) mod n] - all 2^27 outputs against the oracle's plain
    transform; once more with both bit-reversed orders.  The field's generator: inverse-coset(coset(x)) = x on
    all 2^27 elements, and 16 non-zero inputs whose indices exercise all three index digits against the closed form
    X[k] = sum_p x[p] g^p w^(p k) on 2^16 sampled outputs."""
    import numpy as np
    field, logn = "BLS381", 27
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    w = orc.omega(field, logn)
    fl = NTTClient.NO_FACTOR_TABLE if pass2 == "stepped" else 0
    x, X = _full_input(orc)
    j = 5 + (3 << 9) + (2 << 18)
    fwd = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, flags=fl)
    before = fwd.info()
    assert before["pass2_factor_table"] == (pass2 == "factor_table")
    fwd.set_coset(pow(w, j, r))
    assert fwd.info()["device_bytes"] - before["device_bytes"] < 32 << 20   # tG (20 MiB) and the small tables
    d_x = DeviceBuffer(0, 32 * n)
    d_x.upload(x)
    y = _run_dev(fwd, d_x)
    rolled = np.roll(X.reshape(n, 32), -j, axis=0).reshape(-1)
    assert np.array_equal(y, rolled), "2^27 coset transform with g = w^j is not the rotated plain transform"
    del y
    # once more with both bit-reversed orders: the buffers are permuted, the power of g follows the element
    threads = max(1, min(64, (os.cpu_count() or 8)))
    bb = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, flags=fl | NTTClient.BITREV_INPUT | NTTClient.BITREV_OUTPUT)
    bb.set_coset(pow(w, j, r))
    y = _run_dev(bb, orc.bitrev_permute(x, logn, threads))
    bb.close()
    assert np.array_equal(y, np.frombuffer(orc.bitrev_permute(rolled, logn, threads), dtype=np.uint8)), "... with both bit-reversed orders"
    del y, rolled
    # a general shift: the round trip through the inverse handle, on the device
    g = GENERATOR[field]
    inv = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, flags=fl | NTTClient.INVERSE)
    assert inv.info()["pass2_factor_table"] == (pass2 == "factor_table")
    fwd.set_coset(g); inv.set_coset(g)
    fwd.set_data(NTTInput(0, d_x)); fwd.start_process(0); fwd.wait_result()
    fwd.result_device(0, d_x)
    z = _run_dev(inv, d_x)
    d_x.free()
    assert np.array_equal(z, x), "inverse-coset(coset(x)) != x at 2^27"
    del z
    # back to plain: the tables that carried the shift (pass 2's factors among them) are today's again
    inv.set_coset(None)
    assert np.array_equal(_run_dev(inv, X, buf=1), x), "a handle set back to plain differs from the plain inverse"
    inv.close()
    fwd.set_coset(None)
    assert np.array_equal(_run_dev(fwd, x), X), "a handle set back to plain differs from the plain transform"
    fwd.set_coset(g)
    # 16 non-zero inputs, closed form on 2^16 sampled outputs
    rng = random.Random(27)
    ps = [1, 511, 512, 513, 1 << 18, (1 << 18) + 1, (300 << 18) + (200 << 9) + 100, n - 1] + [rng.randrange(n) for _ in range(8)]
    vals = [rng.randrange(1, r) for _ in ps]
    sparse = np.zeros(32 * n, dtype=np.uint8)
    for p, v in zip(ps, vals):
        sparse[32 * p: 32 * p + 32] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    y = _run_dev(fwd, sparse, buf=1).reshape(n, 32)
    fwd.close()
    k0, stride, cnt = 5, 2039, 1 << 16
    ks = [(k0 + stride * t) % n for t in range(cnt)]
    acc = [0] * cnt
    for p, v in zip(ps, vals):
        term = v * pow(g, p, r) * pow(w, p * k0 % n, r) % r
        step = pow(w, p * stride % n, r)
        for t in range(cnt):
            acc[t] += term
            term = term * step % r
    for t, k in enumerate(ks):
        assert int.from_bytes(y[k].tobytes(), "little") == acc[t] % r, k


def test_timing_2e27(gpu, orc):
    """One forward and one inverse handle, each toggled between plain and coset with set_coset, alternating, 5 transforms each,
    medians of blz_ntt_last_kernel_ms.  Bounds (derived, not measured): forward coset <= 1.15 x plain - the additional product is
    8 x 143 of 14 935 multiply-adds per lane = 7.7 %, doubled for the table reads and register pressure (an unfused scaling pass
    would cost >= 25 %); inverse coset <= 1.05 x plain inverse - no additional product, box noise within a process is 1-2 %."""
    logn = 27
    n = 1 << logn
    g = GENERATOR["BLS381"]
    d_in = DeviceBuffer(0, 32 * n)
    blaze_amd._lib.check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n, 7))
    med = {}
    for name, inverse in (("forward", False), ("inverse", True)):
        cl = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, inverse=inverse)
        cl.set_data(NTTInput(0, d_in))
        ms = {"plain": [], "coset": []}
        for it in range(6):
            for kind in ("plain", "coset"):
                cl.set_coset(g if kind == "coset" else None)
                cl.start_process(0)
                cl.wait_result()
                if it:   # (the first round warms up)
                    ms[kind].append(cl.last_kernel_ms())
        cl.close()
        med[name] = {k: statistics.median(v) for k, v in ms.items()}
    d_in.free()
    print("[2^27 kernel ms, medians of 5] forward plain %.3f coset %.3f (x %.3f)  inverse plain %.3f coset %.3f (x %.3f)" % (
        med["forward"]["plain"], med["forward"]["coset"], med["forward"]["coset"] / med["forward"]["plain"],
        med["inverse"]["plain"], med["inverse"]["coset"], med["inverse"]["coset"] / med["inverse"]["plain"]))
    assert med["forward"]["coset"] <= 1.15 * med["forward"]["plain"], med
    assert med["inverse"]["coset"] <= 1.05 * med["inverse"]["plain"], med
