"""Sparse matrix-vector products on resident buffers (blz_ntt_vec_spmv) on the device: dst[p] = the sum over the nonzeros k of
row p of val[k] x[col[k] mod count], from CSR arrays in device memory, with and without coefficients, and the index mode
dst[p] = val[p] x[col[p] mod count] - and what the op is for: the three vectors A w, B w, C w of an R1CS instance and the wire
columns of PLONK.  Every expected value is Python integer arithmetic (tests/ntt_spmv_util.py) and every comparison is byte for
byte: any 256-bit word of x or val counts as its residue, every output word is canonical.  The input recipe is the house one:
the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 first, unmasked random 256-bit words behind."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DriverClientError
from blaze_amd._lib import BlzVecArg, BlzVecCsr
from blaze_amd.ingo_ntt import NTTClient, NTTInput, NttInit
from ntt_spmv_util import (TILE, _inputs, _u32, random_cols, random_vals, row_ptr_of, shaped_lengths, sparse_rows, split_rows,
                           spmv_ref, spmv_want)
from ntt_vec_util import FIELDS, _client, _dev, _pack, _transform, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
MUL, MULSUB, SSUM = NTTClient.MUL, NTTClient.MULSUB, NTTClient.SCAN_SUM


def _fill(n, seed):   # not ntt_mle_util.fill (random bytes): n words none of which is zero, so that a position the op must zero shows
    return _pack([v | 1 for v in _words(seed, n)])


def _run(cl, dst, x, col, row_ptr=None, val=None, **kw):
    """One vec_spmv from host lists: the arrays are uploaded, the op runs, the destination comes back."""
    bufs = [_dev(_u32(col) if col else bytes(4)), None if row_ptr is None else _dev(_u32(row_ptr)),
            None if val is None else _dev(_pack(val) if val else bytes(32))]
    kw.setdefault("nnz", len(col))
    cl.vec_spmv(dst, x, bufs[0], row_ptr=bufs[1], val=bufs[2], **kw)
    cl.wait_result()
    out = bytes(cl.result(dst))
    for b in bufs:
        if b is not None:
            b.free()
    return out


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [3, 12])
def test_csr_against_python_integers(gpu, field, logn):
    """x is transform buffer 0 (n words, the edge words among them), the destination buffer 1 - filled with non-zero words
    before every call, so that an empty row and the positions above `rows` show.  Every nnz that changes the number of tiles
    or fills one exactly, split at random over rows with empty ones among them; with coefficients (edge words first) and
    without; nnz = len(col) throughout, so the bound 2048 at n = 8 is met exactly."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    x = _inputs(r, n, 700 * logn + len(field))
    xb, fill = _pack(x), _fill(n, logn + 70)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, xb))
    rng = random.Random(31 * logn + len(field))
    sizes = [0, 1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE] + ([5 * TILE + 37] if logn == 12 else [])
    for nnz in sizes:
        for rows in sorted({1, min(n, 7), n}):
            lengths = split_rows(rng, nnz, rows)
            rp = row_ptr_of(lengths)
            col, val = random_cols(rng, nnz, n), random_vals(r, nnz, nnz + rows)
            for v in (val, None):
                what = f"{field} 2^{logn} nnz {nnz} rows {rows} {'with' if v else 'without'} val"
                cl.set_data(NTTInput(1, fill))
                assert _run(cl, 1, 0, col, rp, v) == spmv_want(x, r, n, col, rp, v), what
    assert bytes(cl.result(0)) == xb
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
def test_csr_shapes_a_tile_can_get_wrong(gpu, field):
    """n = 2^12 and the row lengths of shaped_lengths: empty rows at the start, between two tiles and at the end, a row ending
    exactly on a tile boundary, one crossing a boundary, one covering three whole tiles and parts of two more, 2500 rows of
    length 1 (four rows inside a lane), a row whose two terms cancel, rows < n.  The same arrays then with junk nonzeros
    ahead of row_ptr[0] and behind row_ptr[rows], as a slab (d_row_ptr + r0, once starting inside the long row's tiles), and
    with x as the other transform buffer and as 1, 4 and 4n device words."""
    logn = 12
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    lengths, marks = shaped_lengths(n)
    rows = len(lengths)
    rng = random.Random(len(field) + 12)
    x = _inputs(r, n, 1200 + len(field))   # x[1] = 1, x[2] = r - 1
    xb, fill = _pack(x), _fill(n, 71)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, xb))
    for first, extra in ((0, 0), (7, 9)):
        rp = row_ptr_of(lengths, first)
        nnz = rp[-1] + extra
        col, val = random_cols(rng, nnz, n), random_vals(r, nnz, 1201 + first)
        k = rp[marks["cancels"]]
        col[k], col[k + 1], val[k + 1] = 1, 2 + n, val[k]    # v * 1 + v * (r - 1), and 1 + (r - 1) without val
        for v in (val, None):
            what = f"{field} row_ptr[0] = {first}, {extra} nonzeros behind the last row, {'with' if v else 'without'} val"
            want = spmv_ref(x, r, n, col, rp, v)
            assert want[marks["cancels"]] == 0 and any(want[rows:]) is False and any(want[:rows])
            cl.set_data(NTTInput(1, fill))
            assert _run(cl, 1, 0, col, rp, v, nnz=nnz) == _pack(want), what
            # a slab of rows: row_ptr + r0, the full col / val arrays
            for r0, cnt in ((marks["covers_three"], None), (marks["covers_three"] + 1, 1000), (marks["crosses_one"], 3), (rows - 3, 2)):
                cl.set_data(NTTInput(1, fill))
                got = _run(cl, 1, 0, col, rp, v, nnz=nnz, row0=r0, rows=cnt)
                assert got == spmv_want(x, r, n, col, rp[r0:], v, rows=cnt), what + f", slab from row {r0}"
    assert bytes(cl.result(0)) == xb
    # x as device words of other lengths than n: the destination is buffer 0 now, buffer 1 keeps its bytes
    rp = row_ptr_of(lengths)
    col, val = random_cols(rng, rp[-1], 4 * n), random_vals(r, rp[-1], 1203)
    big = _inputs(r, 4 * n, 1204)
    keep = bytes(cl.result(1))
    for count in (1, 4, 4 * n):
        src = big[:count]
        d = _dev(_pack(src))
        for v in (val, None):
            cl.set_data(NTTInput(0, fill))
            assert _run(cl, 0, d, col, rp, v) == spmv_want(src, r, n, col, rp, v), f"{field}: x of {count} device words"
        assert bytes(d.download()) == _pack(src)
        d.free()
    assert bytes(cl.result(1)) == keep
    # ... and the other way round: x is buffer 1, the destination buffer 0
    x1 = [int.from_bytes(keep[32 * i: 32 * i + 32], "little") for i in range(n)]
    assert _run(cl, 0, 1, col, rp, val) == spmv_want(x1, r, n, col, rp, val)
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 6, 11])
def test_index_mode_against_python_integers(gpu, field, logn):
    """col as the identity, a reversal, a random permutation, a constant and random 32-bit values (masked by the op); with and
    without val; the source a transform buffer and 1, 4 and 4n device words; fewer entries than n (zeros above) and none."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(17 * logn + len(field))
    x = _inputs(r, n, 1700 * logn + len(field))
    xb, fill = _pack(x), _fill(n, logn + 72)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, xb))
    perm = list(range(n))
    rng.shuffle(perm)
    tables = {"identity": list(range(n)), "reversal": list(range(n))[::-1], "permutation": perm, "constant": [n - 1] * n,
              "wild": random_cols(rng, n, n), "short": perm[:n // 2 + 1], "empty": []}
    val = random_vals(r, n, 1701 + logn)
    for name, col in tables.items():
        for v in (val[:len(col)], None):
            what = f"{field} 2^{logn} {name} {'with' if v is not None else 'without'} val"
            cl.set_data(NTTInput(1, fill))
            assert _run(cl, 1, 0, col, None, v, nnz=len(col)) == spmv_want(x, r, n, col, None, v), what
    assert bytes(cl.result(0)) == xb
    big = _inputs(r, 4 * n, 1702 + logn)
    for count in (1, 4, 4 * n):
        src = big[:count]
        d = _dev(_pack(src))
        col = random_cols(rng, n, count)
        for v in (val, None):
            cl.set_data(NTTInput(1, fill))
            assert _run(cl, 1, d, col, None, v) == spmv_want(src, r, n, col, None, v), f"{field} 2^{logn}: x of {count} device words"
        d.free()
    cl.close()


def test_second_turn_of_the_grid_stride_loop(gpu):
    """2^20 positions are two sweeps of the 2048 x 256 launch grid of k_spmv_index (k_spmv_tile launches one block per tile and
    has no such loop).  BLS12-381, a random permutation with coefficients and without, cut at n / 2 + 1 entries - the first
    position of the second sweep is the last that reads.  Every position is checked."""
    field, logn = "BLS381", 20
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    raw = random.Random(2030).randbytes(32 * n)
    x = [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]
    vraw = random.Random(2031).randbytes(32 * n)
    val = [int.from_bytes(vraw[32 * i: 32 * i + 32], "little") for i in range(n)]
    perm = list(range(n))
    random.Random(2032).shuffle(perm)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, raw))
    col, dval = _dev(_u32(perm)), _dev(vraw)
    cl.vec_index(1, 0, col)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([x[c] % r for c in perm])
    cl.vec_index(1, 0, col, val=dval)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([x[c] * v % r for c, v in zip(perm, val)])
    m = n // 2 + 1
    cl.vec_spmv(1, 0, col, val=dval, rows=m, nnz=m)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([x[c] * v % r for c, v in zip(perm[:m], val)]) + bytes(32 * (n - m))
    assert bytes(cl.result(0)) == raw
    cl.close()
    for d in (col, dval):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_r1cs_instance_end_to_end(gpu, field):
    """n = 2^10 constraints over a witness of 2n words.  A, B and the free part of C are random sparse over the first n
    columns, with one row of A 300 nonzeros long; C's row p also holds a 1 in column n + p, and w[n + p] is chosen as
    (A w)[p] (B w)[p] - (C_free w)[p]: the instance is satisfied by the construction of that column.  Three vec_spmv calls
    into two handles, C w handed over as device words, then MULSUB leaves zeros in every position - and with one coefficient
    of A flipped it does not."""
    logn = 10
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 10)
    w = [rng.randrange(r) for _ in range(n)]
    A, B, Cf = (sparse_rows(rng, r, n, n) for _ in range(3))
    # a long row in A: row 5 takes 300 nonzeros
    rpA, colA, valA = A
    k = rpA[5]
    colA[k:k] = [rng.randrange(n) for _ in range(300)]
    valA[k:k] = [rng.randrange(r) for _ in range(300)]
    rpA = rpA[:6] + [v + 300 for v in rpA[6:]]
    aw, bw, cw = (spmv_ref(w, r, n, m[1], m[0], m[2]) for m in ((rpA, colA, valA), B, Cf))
    w += [(aw[p] * bw[p] - cw[p]) % r for p in range(n)]
    rpC, colC, valC = [], [], []
    for p in range(n):   # C = C_free plus the identity on the fresh column
        rpC.append(len(colC))
        colC += Cf[1][Cf[0][p]:Cf[0][p + 1]] + [n + p]
        valC += Cf[2][Cf[0][p]:Cf[0][p + 1]] + [1]
    rpC.append(len(colC))
    dw = _dev(_pack(w))
    h1, h2 = _client(field, logn), _client(field, logn)
    out_c = _dev(bytes(32 * n))

    def residual(vals_a):
        arrays = [_dev(b) for b in (_u32(rpA), _u32(colA), _pack(vals_a), _u32(B[0]), _u32(B[1]), _pack(B[2]), _u32(rpC), _u32(colC), _pack(valC))]
        h1.vec_spmv(0, dw, arrays[1], row_ptr=arrays[0], val=arrays[2])
        h2.vec_spmv(0, dw, arrays[7], row_ptr=arrays[6], val=arrays[8])
        h1.wait_result()
        h1.vec_spmv(1, dw, arrays[4], row_ptr=arrays[3], val=arrays[5])
        h2.wait_result()
        h2.result_device(0, out_c)
        h1.wait_result()
        h1.vec_op(MULSUB, 0, 0, 1, out_c)
        h1.wait_result()
        for d in arrays:
            d.free()
        return bytes(h1.result(0))

    assert residual(valA) == bytes(32 * n)
    flipped = list(valA)
    flipped[rpA[5] + 150] = (flipped[rpA[5] + 150] + 1) % r
    bad = residual(flipped)
    assert bad != bytes(32 * n) and bad[:32 * 5] == bytes(32 * 5) and bad[32 * 6:] == bytes(32 * (n - 6))
    for cl in (h1, h2):
        cl.close()
    for d in (dw, out_c):
        d.free()


def test_plonk_wire_assembly(gpu):
    """a[p] = w[ia[p]], b[p] = w[ib[p]], c[p] = w[ic[p]] through vec_index into three buffers of two handles."""
    field, logn = "BN254", 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(99)
    w = _inputs(r, 256, 98)
    dw = _dev(_pack(w))
    tables = [[rng.randrange(256) for _ in range(n)] for _ in range(3)]
    h1, h2 = _client(field, logn), _client(field, logn)
    cols = [_dev(_u32(t)) for t in tables]
    for cl, dst, d in ((h1, 0, cols[0]), (h1, 1, cols[1]), (h2, 0, cols[2])):
        cl.vec_index(dst, dw, d)
        cl.wait_result()
    got = [bytes(h1.result(0)), bytes(h1.result(1)), bytes(h2.result(0))]
    assert got == [_pack([w[i] % r for i in t]) for t in tables]
    for cl in (h1, h2):
        cl.close()
    for d in cols + [dw]:
        d.free()


def test_protocol(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b = _inputs(r, n, 15), _inputs(r, n, 16)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    rng = random.Random(8)
    lengths = split_rows(rng, 3 * TILE + 5, n)
    rp = row_ptr_of(lengths)
    col, val = random_cols(rng, rp[-1], n), random_vals(r, rp[-1], 17)
    d_rp, d_col, d_val = _dev(_u32(rp)), _dev(_u32(col)), _dev(_pack(val))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    spmv = lambda: cl.vec_spmv(1, 0, d_col, row_ptr=d_rp, val=d_val)   # noqa: E731
    busy = (lambda: cl.start_process(1), lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(MUL, 1, 1, words),
            lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 1), lambda: cl.vec_scan(SSUM, 1, 1), lambda: cl.vec_horner(1, 1, one_word),
            lambda: cl.vec_gather(1, words), spmv, lambda: cl.vec_index(0, words, d_col))
    # refused while a transform or an op is in flight; the destination of the refused call keeps its bytes
    cl.initialize(NttInit())
    cl.start_process(0)
    with pytest.raises(DriverClientError) as ei:
        spmv()
    assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    cl.vec_op(MUL, 0, 0, words)
    with pytest.raises(DriverClientError) as ei:
        spmv()
    assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(0, ab))
    sink = bytearray(32 * n)
    spmv()   # enqueued, not waited for
    for attempt in (lambda: cl.set_data(NTTInput(1, bb)), lambda: cl.exchange(1, bb, sink)):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 1" in str(ei.value)
    assert bytes(cl.result(0)) == ab          # the buffer it only reads can be read
    for attempt in busy + (lambda: cl.result(1),):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want = spmv_want(a, r, n, col, rp, val)
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab
    with pytest.raises(DriverClientError):   # nothing is in flight any more
        cl.wait_result()
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with a product in flight: nothing is in flight afterwards, and the handle works
    spmv()
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    spmv()
    cl.wait_result()
    assert bytes(cl.result(1)) == want
    cl.close()
    for d in (d_rp, d_col, d_val, words, one_word):
        d.free()


def test_refusals(gpu):
    field, logn = "BN254", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 25), _inputs(r, n, 26)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    nnz = 2 * n
    d_rp = _dev(_u32(list(range(0, nnz + 1, 2))))
    d_col = _dev(_u32([i % n for i in range(nnz)]))
    d_val = _dev(_pack([i + 1 for i in range(nnz)]))
    huge = 256 * n + 1
    d_huge = _dev(bytes(4 * huge))
    host = C.create_string_buffer(32 * nnz + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def spmv(dst, x, m):
        return L.blz_ntt_vec_spmv(cl._h, dst, None if x is None else C.byref(x), None if m is None else C.byref(m))

    def csr(rp=d_rp.ptr, col=d_col.ptr, val=d_val.ptr, rows=n, nz=nnz):
        return BlzVecCsr(rp, col, val, rows, nz)

    B0, B1, W = BlzVecArg(None, 0, 0, 0), BlzVecArg(None, 1, 0, 0), BlzVecArg(words.ptr, 0, 0, n)
    refused = {   # what: (call, what the message names)
        "no x": (lambda: spmv(1, None, csr()), "operand x and a matrix m"),
        "no m": (lambda: spmv(1, B0, None), "operand x and a matrix m"),
        "buf_dst 2": (lambda: spmv(2, B0, csr()), "buf_dst must be"),
        "rows = n + 1": (lambda: spmv(1, B0, csr(rows=n + 1)), "matrix m: rows"),
        "nnz = max(1024, 256 n) + 1": (lambda: spmv(1, B0, csr(rp=None, col=d_huge.ptr, val=None, rows=n, nz=huge)), "matrix m: nnz"),
        "nnz 2^40": (lambda: spmv(1, B0, csr(nz=1 << 40)), "matrix m: nnz"),
        "no d_col": (lambda: spmv(1, B0, csr(col=None)), "matrix m: d_col"),
        "index mode, rows != nnz": (lambda: spmv(1, B0, csr(rp=None, rows=n, nz=n - 1)), "matrix m: without d_row_ptr"),
        "d_col 2 bytes off": (lambda: spmv(1, B0, csr(col=d_col.ptr + 2, nz=nnz - 1)), "matrix m: d_col"),
        "d_row_ptr 1 byte off": (lambda: spmv(1, B0, csr(rp=d_rp.ptr + 1, rows=n - 1)), "matrix m: d_row_ptr"),
        "d_val 8 bytes off": (lambda: spmv(1, B0, csr(val=d_val.ptr + 8, nz=nnz - 1)), "matrix m: d_val"),
        "d_val runs past its allocation": (lambda: spmv(1, B0, csr(val=d_val.ptr + 32)), "the allocation d_val points into"),
        "d_col runs past its allocation": (lambda: spmv(1, B0, csr(col=d_col.ptr + 4)), "the allocation d_col points into"),
        "d_row_ptr runs past its allocation": (lambda: spmv(1, B0, csr(rp=d_rp.ptr + 4)), "the allocation d_row_ptr points into"),
        "a host pointer as d_col": (lambda: spmv(1, B0, csr(col=host_ptr)), "matrix m: d_col"),
        "a host pointer as d_val": (lambda: spmv(1, B0, csr(val=host_ptr)), "matrix m: d_val"),
        "a host pointer as d_row_ptr": (lambda: spmv(1, B0, csr(rp=host_ptr)), "matrix m: d_row_ptr"),
        "x names buf_dst": (lambda: spmv(1, B1, csr()), "operand x"),
        "x names buf_dst 0": (lambda: spmv(0, B0, csr()), "operand x"),
        # the operand errors of blz_ntt_vec_op
        "count 3": (lambda: spmv(1, BlzVecArg(words.ptr, 0, 0, 3), csr()), "operand x"),
        "count 0": (lambda: spmv(1, BlzVecArg(words.ptr, 0, 0, 0), csr()), "operand x"),
        "count 2^28": (lambda: spmv(1, BlzVecArg(words.ptr, 0, 0, 1 << 28), csr()), "operand x"),
        "count of a transform buffer": (lambda: spmv(1, BlzVecArg(None, 0, 0, 4 * n), csr()), "operand x"),
        "reserved = 1": (lambda: spmv(1, BlzVecArg(None, 0, 1, 0), csr()), "operand x"),
        "buf = 2": (lambda: spmv(1, BlzVecArg(None, 2, 0, 0), csr()), "operand x"),
        "x misaligned": (lambda: spmv(1, BlzVecArg(words.ptr + 8, 0, 0, 1), csr()), "operand x"),
        "x a host pointer": (lambda: spmv(1, BlzVecArg(host_ptr, 0, 0, n), csr()), "operand x"),
        "x of 4n words in an allocation of n": (lambda: spmv(1, BlzVecArg(words.ptr, 0, 0, 4 * n), csr()), "operand x"),
    }
    L.blz_last_error_message.restype = C.c_char_p
    for what, (attempt, names) in refused.items():
        assert attempt() == 4, what
        msg = L.blz_last_error_message().decode()
        assert names in msg, (what, msg)   # the argument by its full name: "operand x", "matrix m: d_col" ...
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb
    # the handle is as usable as before, and the bound itself is accepted
    assert spmv(1, B0, csr()) == 0
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([((2 * p + 1) * a[(2 * p) % n] + (2 * p + 2) * a[(2 * p + 1) % n]) % r for p in range(n)])
    assert spmv(1, W, csr(rp=None, col=d_huge.ptr, val=None, rows=n, nz=n)) == 0
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([b[0] % r] * n)
    # nnz = 256 n: 64 tiles, all but the first without a row (row_ptr[rows] = 2n); every column is 0
    assert spmv(1, B0, csr(col=d_huge.ptr, val=None, nz=huge - 1)) == 0
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack([2 * a[0] % r] * n)
    cl.close()
    for d in (words, d_rp, d_col, d_val, d_huge):
        d.free()
