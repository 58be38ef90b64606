"""Scatter-add on resident buffers (blz_ntt_vec_scatter) on the device: dst[t] = the sum over the nonzeros k with
idx[k] mod n == t of val[k] x[src(k) mod count] - the histogram without x and val - and what the op is for: the multiplicity
column of a lookup argument and the transposed sparse product.  Every expected value is Python integer arithmetic, a dict of
sums modulo r, and every comparison is byte for byte over every position, the zeros included: any 256-bit word of x or val
counts as its residue, every output word is canonical.  The destination is filled with non-zero words before a call, so that a
position no nonzero names shows.  The sizes straddle the two LDS thresholds of ntt_scatter.hip.hpp (add mode n <= 2^10, count
mode n <= 2^14): the path depends on n and the mode alone."""
import ctypes as C
import random
import re

import pytest

import blaze_amd
from blaze_amd import DriverClientError
from blaze_amd._lib import BlzVecArg, BlzVecScatter
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from isa_util import _read
from ntt_mle_util import check_order_of_checks
from ntt_spmv_util import _inputs, _u32, sparse_rows, spmv_ref
from ntt_vec_util import FIELDS, TOP, _client, _dev, _edges, _pack, _transform, _unpack, _word, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
SUB, MUL, INV = NTTClient.SUB, NTTClient.MUL, NTTClient.INV
SUM, DOT = NTTClient.FOLD_SUM, NTTClient.FOLD_DOT


def scatter_ref(r, n, idx, x=None, val=None, src=None):
    """dst as a list of n integers, from a dict of sums modulo r: the documented formula."""
    sums = {}
    for k, i in enumerate(idx):
        term = 1 if val is None else val[k]
        if x is not None:
            term *= x[(k if src is None else src[k]) % len(x)]
        t = i % n
        sums[t] = (sums.get(t, 0) + term) % r
    return [sums.get(t, 0) for t in range(n)]


def _fill(n, seed):
    return _pack([v | 1 for v in _words(seed, n)])


def _values(r, count, seed):
    """The house recipe with 2^255 added: 0, 1, r - 1, r, r + 1, 2^256 - 1, 2^255 first, unmasked random 256-bit words behind."""
    a = _words(seed, count)
    for i, e in enumerate((_edges(r) + [1 << 255])[:count]):
        a[i] = e
    return a


def _indices(rng, nnz, n):
    """Index words the op has to mask: 0, n - 1, n, 0xffffffff first, then random 32-bit values."""
    return ([0, n - 1, n, 0xffffffff] + [rng.randrange(1 << 32) for _ in range(nnz)])[:nnz]


def _run(cl, dst, idx, x=None, val=None, src=None):
    """One vec_scatter from host lists: the arrays are uploaded, the op runs, the destination comes back."""
    bufs = [_dev(_u32(idx) if idx else bytes(4)), None if val is None else _dev(_pack(val) if val else bytes(32)),
            None if src is None else _dev(_u32(src) if src else bytes(4))]
    cl.vec_scatter(dst, bufs[0], x=x, val=bufs[1], src=bufs[2], nnz=len(idx))
    cl.wait_result()
    out = bytes(cl.result(dst))
    for b in bufs:
        if b is not None:
            b.free()
    return out


@pytest.mark.parametrize("field,logn", [("BLS381", 1), ("BLS381", 3), ("BLS381", 9), ("BLS381", 14), ("BLS381", 15), ("BLS377", 9), ("BN254", 9)])
def test_counts_against_python_integers(gpu, field, logn):
    """The histogram.  2^14 is the largest destination counted in LDS, 2^15 the smallest counted in memory.  64 n + 1 nonzeros
    (up to 2^9) put more than one block on the LDS path."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    fill = _fill(n, logn + 80)
    cl = _client(field, logn)
    rng = random.Random(41 * logn + len(field))
    for nnz in [0, 1, 7, 63, 64, 65, 4 * n + 3] + ([64 * n + 1] if logn <= 9 else []):
        idx = _indices(rng, nnz, n)
        cl.set_data(NTTInput(1, fill))
        got = _run(cl, 1, idx)
        want = scatter_ref(r, n, idx)
        assert sum(want) == nnz
        assert got == _pack(want), f"{field} 2^{logn} nnz {nnz}"
    # through the mirror's own name, the whole index buffer
    idx = _indices(rng, 100, n)
    d = _dev(_u32(idx))
    cl.vec_count(0, d)
    cl.wait_result()
    assert bytes(cl.result(0)) == _pack(scatter_ref(r, n, idx))
    d.free()
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [1, 3, 10, 11, 12])
def test_add_against_python_integers(gpu, field, logn):
    """2^10 is the largest destination accumulated in LDS, 2^11 the smallest accumulated in memory.  The modes {val}, {x},
    {x, val}, {x, val, src}; x the other transform buffer and 1, 4 and 2n device words; words of x and val at and above r and
    0 and r - 1 among them; src words with high bits set; no nnz a multiple of the eight lanes of a group."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(43 * logn + len(field))
    fill = _fill(n, logn + 81)
    big = _values(r, 2 * n + 2, 4300 + logn)[2:]   # from r - 1 on: the one-word x is r - 1, the four words r - 1, r, r + 1, 2^256 - 1
    xbuf = _values(r, n, 4400 + logn)
    xb = _pack(xbuf)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, xb))
    sources = [(0, xbuf, None)]
    for count in (1, 4, 2 * n):
        d = _dev(_pack(big[:count]))
        sources.append((d, big[:count], d))
    for nnz in (1, 9, 8 * 64 - 1, 8 * 64 + 1, 1000):
        idx = _indices(rng, nnz, n)
        val = _values(r, nnz, 4500 + nnz)
        val.reverse()   # the edge words at the end too: in the last, partly filled group of eight
        src = [rng.randrange(1 << 32) | (0x80000000 if k & 1 else 0) for k in range(nnz)]
        cl.set_data(NTTInput(1, fill))
        assert _run(cl, 1, idx, val=val) == _pack(scatter_ref(r, n, idx, val=val)), f"{field} 2^{logn} nnz {nnz} val"
        for x, xs, _ in sources:
            for mode, kw in (("x", {}), ("x, val", {"val": val}), ("x, val, src", {"val": val, "src": src})):
                cl.set_data(NTTInput(1, fill))
                got = _run(cl, 1, idx, x=x, **kw)
                assert got == _pack(scatter_ref(r, n, idx, x=xs, **kw)), f"{field} 2^{logn} nnz {nnz} {mode}, x of {len(xs)} words"
    assert bytes(cl.result(0)) == xb   # the buffer x names is only read
    for _, xs, d in sources[1:]:
        assert bytes(d.download()) == _pack(xs)
        d.free()
    cl.close()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn", [3, 12])
def test_carries_of_every_limb_accumulator(gpu, field, logn):
    """2^16 nonzeros of value r - 1 into ONE position: r - 2^16.  2^16 words of all-ones limbs into a second: each of the eight
    64-bit accumulators holds 2^16 (2^32 - 1) and carries into the next, the top one into the ninth limb the finish folds in.
    The positions around them are zero.  2^12 accumulates in memory, 2^3 in LDS, in 512 blocks."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    m = 1 << 16
    p1, p2 = 5, 2
    idx = [p1, p2] * m
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _fill(n, 82)))
    d_idx, d_val = _dev(_u32(idx)), _dev((_pack([r - 1]) + _pack([TOP])) * m)
    cl.vec_scatter(0, d_idx, val=d_val)
    cl.wait_result()
    got = _unpack(cl.result(0))
    want = [0] * n
    want[p1], want[p2] = r - m, m * TOP % r
    assert got == want
    cl.close()
    for d in (d_idx, d_val):
        d.free()


def test_second_turn_of_the_grid_stride_loops(gpu):
    """A turn of the grid-stride loops of k_scatter_add and k_scatter_count is SCATTER_MAX_BLOCKS x SCATTER_THREADS = 1024 x 256 =
    2^18 = 2^16 x 4 nonzeros (read from ntt_scatter.hip.hpp below): nnz = 2^16 x 4 + 8 x 3 + 5 leaves the second turn three full
    groups of eight lanes and five lanes of a fourth.  Uniform indices, x the other buffer and val at 2^12; the histogram at
    2^15, where it counts in memory."""
    src = _read("blaze_amd", "csrc", "ntt_scatter.hip.hpp")
    blocks = int(re.search(r"constexpr uint32_t SCATTER_MAX_BLOCKS = (\d+);", src).group(1))
    assert "SCATTER_THREADS = VEC_THREADS;" in src and "constexpr int VEC_THREADS = 256;" in _read("blaze_amd", "csrc", "ntt_vec.hip.hpp")
    turn = blocks * 256
    assert turn == (1 << 16) * 4
    nnz = turn + 8 * 3 + 5
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    rng = random.Random(2040)
    logn = 12
    n = 1 << logn
    x = _inputs(r, n, 2041)
    vraw = random.Random(2042).randbytes(32 * nnz)
    val = _unpack(vraw)
    idx = [rng.randrange(1 << 32) for _ in range(nnz)]
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(x)))
    d_idx, d_val = _dev(_u32(idx)), _dev(vraw)
    cl.vec_scatter(1, d_idx, x=0, val=d_val)
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(scatter_ref(r, n, idx, x=x, val=val))
    cl.close()
    d_val.free()
    logn = 15
    n = 1 << logn
    cl = _client(field, logn)
    cl.vec_count(0, d_idx)
    cl.wait_result()
    assert bytes(cl.result(0)) == _pack(scatter_ref(r, n, idx))
    cl.close()
    d_idx.free()


def test_two_runs_and_both_paths_give_the_same_bytes(gpu):
    """Half of 20001 nonzeros go to one position, the rest below 2^10.  The same call twice: the same bytes.  The same input at
    2^10 (LDS) and at 2^12 (memory): the same first 2^10 words, zeros above, both equal to Python's."""
    field = "BN254"
    r = pyref.CURVES[field]["r"]
    rng = random.Random(2050)
    nnz = 20001
    idx = [37 if rng.random() < 0.5 else rng.randrange(1 << 10) for _ in range(nnz)]
    src = [rng.randrange(1 << 32) for _ in range(nnz)]
    xs, val = _values(r, 1 << 10, 2051), _values(r, nnz, 2052)
    d_x, d_idx, d_src, d_val = _dev(_pack(xs)), _dev(_u32(idx)), _dev(_u32(src)), _dev(_pack(val))
    want = _pack(scatter_ref(r, 1 << 10, idx, x=xs, val=val, src=src))
    got = {}
    for logn in (10, 12):
        cl = _client(field, logn)
        runs = []
        for turn in range(2):
            cl.set_data(NTTInput(0, _fill(1 << logn, 83 + turn)))
            cl.vec_scatter(0, d_idx, x=d_x, val=d_val, src=d_src)
            cl.wait_result()
            runs.append(bytes(cl.result(0)))
        assert runs[0] == runs[1]
        got[logn] = runs[0]
        cl.close()
    assert got[10] == want
    assert got[12] == want + bytes(32 * ((1 << 12) - (1 << 10)))
    for d in (d_x, d_idx, d_src, d_val):
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_transposed_product_against_spmv(gpu, field):
    """<A x, y> from vec_spmv + FOLD_DOT and <x, A^T y> from vec_scatter (idx = col, src = the row of each nonzero, val) +
    FOLD_DOT on a 2^10 handle: equal to each other and to Python."""
    logn = 10
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 2060)
    rp, col, val = sparse_rows(rng, r, n, n)
    row_of = [p for p in range(n) for _ in range(rp[p], rp[p + 1])]
    x, y = _inputs(r, n, 2061), _inputs(r, n, 2062)
    d_x, d_y = _dev(_pack(x)), _dev(_pack(y))
    d_rp, d_col, d_row, d_val = _dev(_u32(rp)), _dev(_u32(col)), _dev(_u32(row_of)), _dev(_pack(val))
    cl = _client(field, logn)
    cl.vec_spmv(1, d_x, d_col, row_ptr=d_rp, val=d_val)
    cl.wait_result()
    left = cl.vec_reduce(DOT, 1, d_y)
    cl.wait_result()
    cl.vec_scatter(0, d_col, x=d_y, val=d_val, src=d_row)
    cl.wait_result()
    aty = scatter_ref(r, n, col, x=y, val=val, src=row_of)
    assert bytes(cl.result(0)) == _pack(aty)
    right = cl.vec_reduce(DOT, 0, d_x)
    cl.wait_result()
    ax = spmv_ref(x, r, n, col, rp, val)
    want = sum(a * b for a, b in zip(ax, y)) % r
    assert want == sum(a * b for a, b in zip(x, aty)) % r
    assert _word(left) == want and _word(right) == want
    cl.close()
    for d in (d_x, d_y, d_rp, d_col, d_row, d_val, left, right):
        d.free()


def test_logup_identity_on_one_handle(gpu):
    """The lookup argument's identity at 2^12: sum_p 1 / (alpha - f[p]) = sum_t m[t] / (alpha - t[t]) with f = vec_index(t, idx) and
    m = vec_count(idx).  The table holds 2^10 distinct nonzero words and a repeat of one of them above; a repeated entry needs
    no care - the multiplicity goes to the index actually used, and both sides sum over the same pairs.  Existing ops do the
    rest; two words are downloaded."""
    field, logn = "BLS381", 12
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    rng = random.Random(2070)
    distinct = set()
    while len(distinct) < 1 << 10:
        distinct.add(rng.randrange(1, r))
    table = sorted(distinct)
    rng.shuffle(table)
    table += [table[7]] * (n - len(table))
    idx = [rng.randrange(16) if rng.random() < 0.3 else rng.randrange(n) for _ in range(n)]   # skewed: 30 % in sixteen entries
    alpha = rng.randrange(r)
    assert alpha not in distinct
    cl = _client(field, logn)
    d_t, d_idx, d_alpha = _dev(_pack(table)), _dev(_u32(idx)), cl.scalar(alpha)
    cl.vec_index(0, d_t, d_idx)            # f
    cl.wait_result()
    cl.vec_op(SUB, 0, d_alpha, 0)
    cl.wait_result()
    cl.vec_op(INV, 0, 0)
    cl.wait_result()
    left = cl.vec_reduce(SUM, 0)
    cl.wait_result()
    cl.vec_count(1, d_idx)                 # m
    cl.wait_result()
    cl.vec_op(SUB, 0, d_alpha, d_t)
    cl.wait_result()
    cl.vec_op(INV, 0, 0)
    cl.wait_result()
    right = cl.vec_reduce(DOT, 0, 1)
    cl.wait_result()
    want = sum(pow(alpha - table[i], -1, r) for i in idx) % r
    assert _word(left) == want and _word(right) == want
    cl.close()
    for d in (d_t, d_idx, d_alpha, left, right):
        d.free()


def test_protocol(gpu, orc):
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b = _inputs(r, n, 35), _inputs(r, n, 36)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    rng = random.Random(9)
    nnz = 3000
    idx, src, val = _indices(rng, nnz, n), [rng.randrange(1 << 32) for _ in range(nnz)], _values(r, nnz, 37)
    d_idx, d_src, d_val = _dev(_u32(idx)), _dev(_u32(src)), _dev(_pack(val))
    words = _dev(bb)
    one_word = _dev((7).to_bytes(32, "little"))
    scatter = lambda: cl.vec_scatter(1, d_idx, x=0, val=d_val, src=d_src)   # noqa: E731
    busy = (lambda: cl.start_process(1), lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(MUL, 1, 1, words),
            lambda: cl.vec_reduce(SUM, 1), lambda: cl.vec_horner(1, 1, one_word), lambda: cl.vec_gather(1, words),
            lambda: cl.vec_index(0, words, d_idx), scatter, lambda: cl.vec_count(0, d_idx))
    # refused while an op is in flight; the destination of the refused call keeps its bytes
    cl.vec_op(MUL, 0, 0, words)
    with pytest.raises(DriverClientError) as ei:
        scatter()
    assert ei.value.variant == "InvalidPrimitiveParam"
    cl.wait_result()
    assert bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(0, ab))
    sink = bytearray(32 * n)
    scatter()   # enqueued, not waited for
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
    want = _pack(scatter_ref(r, n, idx, x=a, val=val, src=src))
    assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab
    with pytest.raises(DriverClientError):   # nothing is in flight any more
        cl.wait_result()
    # the handle still transforms
    _transform(cl, 1)
    assert bytes(cl.result(1)) == bytes(orc.ntt(field, want, logn))
    # reset with a scatter in flight: nothing is in flight afterwards, and the handle works
    scatter()
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.set_data(NTTInput(0, ab))
    scatter()
    cl.wait_result()
    assert bytes(cl.result(1)) == want
    cl.close()
    for d in (d_idx, d_src, d_val, words, one_word):
        d.free()


def test_refusals(gpu):
    field, logn = "BN254", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 45), _inputs(r, n, 46)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words = _dev(bb)
    nnz = 2 * n
    idx = [(3 * i) % n for i in range(nnz)]
    val = [i + 1 for i in range(nnz)]
    d_idx, d_src, d_val = _dev(_u32(idx)), _dev(_u32(list(range(nnz)))), _dev(_pack(val))
    host = C.create_string_buffer(32 * nnz + 64)
    host_ptr = (C.addressof(host) + 63) & ~63

    def scatter(dst, x, s):
        return L.blz_ntt_vec_scatter(cl._h, dst, None if x is None else C.byref(x), None if s is None else C.byref(s))

    def sc(idx=d_idx.ptr, src=d_src.ptr, val=d_val.ptr, nz=nnz, reserved=0):
        return BlzVecScatter(idx, src, val, nz, reserved)

    B0, B1, W = BlzVecArg(None, 0, 0, 0), BlzVecArg(None, 1, 0, 0), BlzVecArg(words.ptr, 0, 0, n)
    refused = {   # what: (call, what the message names)
        "no s": (lambda: scatter(1, B0, None), "a scatter s"),
        "buf_dst 2": (lambda: scatter(2, B0, sc()), "buf_dst must be"),
        "reserved = 1": (lambda: scatter(1, B0, sc(reserved=1)), "scatter s: reserved"),
        "nnz 2^31 + 1": (lambda: scatter(1, B0, sc(nz=(1 << 31) + 1)), "scatter s: nnz"),
        "nnz 2^40": (lambda: scatter(1, B0, sc(nz=1 << 40)), "scatter s: nnz"),
        "no d_idx": (lambda: scatter(1, B0, sc(idx=None)), "scatter s: d_idx"),
        "d_src without x": (lambda: scatter(1, None, sc()), "scatter s: d_src"),
        "d_idx 2 bytes off": (lambda: scatter(1, B0, sc(idx=d_idx.ptr + 2, nz=nnz - 1)), "scatter s: d_idx"),
        "d_src 1 byte off": (lambda: scatter(1, B0, sc(src=d_src.ptr + 1, nz=nnz - 1)), "scatter s: d_src"),
        "d_val 8 bytes off": (lambda: scatter(1, B0, sc(val=d_val.ptr + 8, nz=nnz - 1)), "scatter s: d_val"),
        "d_idx runs past its allocation": (lambda: scatter(1, B0, sc(idx=d_idx.ptr + 4)), "the allocation d_idx points into"),
        "d_src runs past its allocation": (lambda: scatter(1, B0, sc(src=d_src.ptr + 4)), "the allocation d_src points into"),
        "d_val runs past its allocation": (lambda: scatter(1, B0, sc(val=d_val.ptr + 32)), "the allocation d_val points into"),
        "a host pointer as d_idx": (lambda: scatter(1, B0, sc(idx=host_ptr)), "scatter s: d_idx"),
        "a host pointer as d_src": (lambda: scatter(1, B0, sc(src=host_ptr)), "scatter s: d_src"),
        "a host pointer as d_val": (lambda: scatter(1, B0, sc(val=host_ptr)), "scatter s: d_val"),
        "x names buf_dst": (lambda: scatter(1, B1, sc()), "operand x names or overlaps buffer 1"),
        "x names buf_dst 0": (lambda: scatter(0, B0, sc()), "operand x names or overlaps buffer 0"),
        # the operand errors of blz_ntt_vec_op
        "count 3": (lambda: scatter(1, BlzVecArg(words.ptr, 0, 0, 3), sc()), "operand x"),
        "count 0": (lambda: scatter(1, BlzVecArg(words.ptr, 0, 0, 0), sc()), "operand x"),
        "count 2^28": (lambda: scatter(1, BlzVecArg(words.ptr, 0, 0, 1 << 28), sc()), "operand x"),
        "count of a transform buffer": (lambda: scatter(1, BlzVecArg(None, 0, 0, 4 * n), sc()), "operand x"),
        "x reserved = 1": (lambda: scatter(1, BlzVecArg(None, 0, 1, 0), sc()), "operand x"),
        "buf = 2": (lambda: scatter(1, BlzVecArg(None, 2, 0, 0), sc()), "operand x"),
        "x misaligned": (lambda: scatter(1, BlzVecArg(words.ptr + 8, 0, 0, 1), sc()), "operand x"),
        "x a host pointer": (lambda: scatter(1, BlzVecArg(host_ptr, 0, 0, n), sc()), "operand x"),
        "x of 4n words in an allocation of n": (lambda: scatter(1, BlzVecArg(words.ptr, 0, 0, 4 * n), sc()), "operand x"),
    }
    L.blz_last_error_message.restype = C.c_char_p
    for what, (attempt, names) in refused.items():
        assert attempt() == 4, what
        msg = L.blz_last_error_message().decode()
        assert names in msg, (what, msg)
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    assert bytes(words.download()) == bb

    # the order of the checks, and an op in flight: a call wrong in two ways reports the earlier check
    want = _pack(scatter_ref(r, n, idx, x=a, val=val))

    def good():
        assert scatter(1, B0, sc(src=None)) == 0
        cl.wait_result()
        assert bytes(cl.result(1)) == want and bytes(cl.result(0)) == ab
        cl.set_data(NTTInput(1, bb))

    running = "already running"
    cases = [
        ("reserved, and an op in flight", (lambda: scatter(1, B0, sc(reserved=1)), "scatter s: reserved", True), (lambda: scatter(1, B0, sc()), running, True)),
        ("an op in flight, and a bad d_idx", (lambda: scatter(1, B0, sc(idx=d_idx.ptr + 2, nz=nnz - 1)), running, True),
         (lambda: scatter(1, B0, sc(idx=d_idx.ptr + 2, nz=nnz - 1)), "scatter s: d_idx", False)),
        ("buf_dst, and nnz", (lambda: scatter(2, B0, sc(nz=1 << 40)), "buf_dst must be", False), (lambda: scatter(1, B0, sc(nz=1 << 40)), "scatter s: nnz", False)),
        ("a bad x, and x on the destination", (lambda: scatter(1, BlzVecArg(None, 1, 1, 0), sc()), "operand x: reserved", False),
         (lambda: scatter(1, B1, sc()), "names or overlaps", False)),
        ("x on the destination, and a bad d_val", (lambda: scatter(1, B1, sc(val=host_ptr)), "names or overlaps", False),
         (lambda: scatter(1, B0, sc(val=host_ptr)), "scatter s: d_val", False)),
    ]
    total = _dev(bytes(32))
    check_order_of_checks(cl, cases, lambda: cl.vec_reduce(SUM, 0, out=total), good)   # in flight, and writes no buffer
    # the bounds themselves are accepted: nnz 0 writes zeros (d_idx is not looked at), x of device words, no x
    assert scatter(1, B0, sc(idx=None, src=None, val=None, nz=0)) == 0
    cl.wait_result()
    assert bytes(cl.result(1)) == bytes(32 * n)
    assert scatter(1, W, sc(src=None, val=None)) == 0
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(scatter_ref(r, n, idx, x=b))
    assert scatter(0, None, sc(src=None)) == 0
    cl.wait_result()
    assert bytes(cl.result(0)) == _pack(scatter_ref(r, n, idx, val=val))
    cl.close()
    for d in (words, d_idx, d_src, d_val, total):
        d.free()

