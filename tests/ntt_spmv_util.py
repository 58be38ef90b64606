"""What the tests of blz_ntt_vec_spmv share: the reference - the documented formula on Python integers modulo r - and the
builders of the CSR arrays.  The wire format, the edge words and the handle's plumbing are tests/ntt_vec_util.py's."""
import struct

from ntt_vec_util import _edges, _pack, _words

TILE = 1024   # nonzeros per block of k_spmv_tile (ntt_spmv.hip.hpp)


def _u32(vals):
    return struct.pack(f"<{len(vals)}I", *vals)


def _inputs(field_r, count, seed):
    """The edge words first (as far as count reaches), unmasked random 256-bit words behind them."""
    a = _words(seed, count)
    for i, e in enumerate(_edges(field_r)[:count]):
        a[i] = e
    return a


def row_ptr_of(lengths, first=0):
    rp = [first]
    for ln in lengths:
        rp.append(rp[-1] + ln)
    return rp


def sparse_rows(rng, r, rows, width, per_row=(1, 4)):
    """Random sparse rows over the columns [0, width): (row_ptr, col, val)"""
    lengths = [rng.randint(*per_row) for _ in range(rows)]
    rp = row_ptr_of(lengths)
    return rp, [rng.randrange(width) for _ in range(rp[-1])], [rng.randrange(r) for _ in range(rp[-1])]


def spmv_ref(x, r, n, col, row_ptr=None, val=None, rows=None):
    """dst as a list of n integers: dst[p] = sum val[k] x[col[k] % count] % r over row_ptr[p] <= k < row_ptr[p + 1] for
    p < rows, 0 above.  row_ptr None: row p is nonzero p.  val None: coefficients 1.  rows None: all the rows there are."""
    count = len(x)
    if row_ptr is None:
        row_ptr = list(range(len(col) + 1))
    if rows is None:
        rows = len(row_ptr) - 1
    out = [0] * n
    for p in range(rows):
        s = 0
        for k in range(row_ptr[p], row_ptr[p + 1]):
            s += (1 if val is None else val[k]) * x[col[k] % count]
        out[p] = s % r
    return out


def spmv_want(*a, **kw):
    return _pack(spmv_ref(*a, **kw))


def split_rows(rng, nnz, rows):
    """`rows` row lengths that add up to nnz, with empty rows among them (cuts drawn with repetition)."""
    cuts = sorted(rng.randrange(nnz + 1) for _ in range(rows - 1))
    edges = [0] + cuts + [nnz]
    return [edges[i + 1] - edges[i] for i in range(rows)]


def shaped_lengths(n):
    """Row lengths that hit what a tile of 1024 nonzeros split four to a lane can get wrong (n >= 4096 rows available).
    Returns (lengths, marks): marks names the rows the tests speak of."""
    ln, marks = [], {}
    ln += [0, 0, 0]                      # empty rows at the start
    ln += [1000, 24]                     # ... the second ends exactly on the boundary at 1024
    marks["ends_on_boundary"] = len(ln) - 1
    ln += [1500]                         # 1024 .. 2524: crosses the boundary at 2048
    marks["crosses_one"] = len(ln) - 1
    ln += [548]                          # 2524 .. 3072: ends on a boundary again
    ln += [0] * 7                        # empty rows exactly between two tiles
    ln += [300]                          # 3072 .. 3372
    ln += [724 + 3 * TILE + 500]         # 3372 .. 7668: parts of tiles 3 and 7, the whole of tiles 4, 5, 6
    marks["covers_three"] = len(ln) - 1
    ln += [2]                            # two terms that cancel (the tests choose col / val)
    marks["cancels"] = len(ln) - 1
    ln += [1] * 2500                     # four rows inside one lane, over several tiles
    ln += [2, 3, 0, 5, 0, 0, 4, 1, 0, 7, 9, 0, 1, 1, 2]
    ln += [0] * 11                       # empty rows at the end
    assert len(ln) < n
    return ln, marks


def random_cols(rng, nnz, count, wild=True):
    """Column values: below count, and (wild) at and above it - the op masks them."""
    return [rng.randrange(1 << 32) if wild and rng.random() < 0.5 else rng.randrange(count) for _ in range(nnz)]


def random_vals(r, nnz, seed):
    """Coefficients: the edge words first, unmasked random 256-bit words behind."""
    return _inputs(r, nnz, seed)

