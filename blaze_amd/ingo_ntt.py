"""Host-side mirror of src/ingo_ntt (ntt_api.rs): same names and call sequence over the C ABI."""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Optional

from ._lib import GATE_MAX_FACTORS, GATE_MAX_TABLES, GATE_MAX_TERMS, LIN_FORM, LIN_MAX_FORMS, LIN_MAX_SUMMANDS, LIN_MAX_TABLES, LIN_NO_COEF, BlzLinGate, BlzSumGate, BlzVecArg, BlzVecCsr, BlzVecScatter, BlzVecView, DeviceBuffer, buf_ptr, check, lib
from .driver_client import DriverClient, DriverPrimitive

NTT_LOG_SIZE = 27  # ntt_data.rs:65: NTT_SIZE = 2^27
NTT_WORD_SIZE = 32  # ntt_data.rs:66
FORM = LIN_FORM  # BLZ_LIN_FORM: FORM + k as a factor or as common of NTTClient.gate_eval_lin names forms[k]
VEC_INV_TILE = 1024  # csrc/ntt_engine.hpp NTT_VEC_INV_TILE: elements per block of NTTClient.vec_op(NTTClient.INV, ...)


class NTT(enum.Enum):  # ntt_api.rs:8-10
    Ntt = 0


@dataclass
class NttInit:  # ntt_api.rs:17
    pass


@dataclass
class NTTInput:  # ntt_api.rs:19-23
    buf_host: int
    data: object  # bytes-like of 2^log_size * 32 bytes, or a DeviceBuffer


class NTTClient(DriverPrimitive[NTT, NttInit, NTTInput, bytes]):
    """ntt_api.rs:12-15, 25-125.  `log_size` defaults to the reference's fixed 2^27; smaller
    transforms exist for tests (the reference has no such knob).  `field` names the curve whose
    scalar field the transform is over ("BLS381" by default, "BLS377", "BN254")."""

    _FIELDS = {"BLS377": 0, "BLS381": 1, "BN254": 2}  # enum blz_curve

    NO_FACTOR_TABLE = 1  # include/blaze_hip.h BLZ_NTT_NO_FACTOR_TABLE
    INVERSE = 2          # BLZ_NTT_INVERSE
    BITREV_INPUT = 4     # BLZ_NTT_BITREV_INPUT
    BITREV_OUTPUT = 8    # BLZ_NTT_BITREV_OUTPUT
    ADD, SUB, MUL, MULADD, MULSUB, INV = range(6)   # enum blz_vec_op
    FOLD_SUM, FOLD_DOT, FOLD_EVAL = range(3)        # enum blz_fold_op
    SCAN_SUM, SCAN_PROD = range(2)                  # enum blz_scan_op
    SCAN_EXCLUSIVE = 1                              # BLZ_SCAN_EXCLUSIVE
    HORNER_EXCLUSIVE, HORNER_REVERSE = 1, 2         # BLZ_HORNER_*
    MLE_LOW = 1                                     # BLZ_MLE_LOW
    GATE_PRODUCT, GATE_R1CS = 0, 1                  # BLZ_GATE_*
    TREE_PROD, TREE_FRAC = 0, 1                     # enum blz_tree_op
    GKR_UNFUSED = 1                                 # BLZ_GKR_UNFUSED

    def __init__(self, _ptype: NTT, dclient: DriverClient, log_size: int = NTT_LOG_SIZE, inverse: bool = False,
                 field: str = "BLS381", flags: int = 0, root: Optional[int] = None):
        """root / BITREV_* flags: the transform's convention, which the reference leaves unstated (NttInit {} is empty,
        ntt_api.rs:8-23) - any primitive 2^log_size-th root of unity (an int, checked on the device) instead of this
        build's g^((r - 1) / 2^log_size), input and / or output in bit-reversed order (include/blaze_hip.h blz_ntt_new_ex3)."""
        self.driver_client = dclient
        self.log_size = log_size
        self.inverse = inverse or bool(flags & self.INVERSE)
        self.field = field
        self.nbytes = NTT_WORD_SIZE << log_size
        h = C.c_void_p()
        rb = None if root is None else int(root).to_bytes(32, "little")
        check(lib().blz_ntt_new_ex3(dclient.id, self._FIELDS[field], log_size, int(flags) | (self.INVERSE if inverse else 0), rb, C.byref(h)))
        self._h = h
        self._vec_keep = None   # the operands of a vec_op in flight: their device memory must outlive it

    def close(self):
        if getattr(self, "_h", None):
            lib().blz_ntt_free(self._h)
            self._h = None
            self._vec_keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def loaded_binary_parameters(self) -> list[int]:
        raise NotImplementedError("todo!() in the reference too (ntt_api.rs:33-35)")

    def initialize(self, _param: NttInit = NttInit()) -> None:  # ntt_api.rs:37-56
        check(lib().blz_ntt_initialize(self._h))

    def start_process(self, buf_kernel: Optional[int] = None) -> None:  # ntt_api.rs:58-70
        if buf_kernel is None:
            raise TypeError("buf_kernel is required (the reference unwraps it: ntt_api.rs:62)")
        check(lib().blz_ntt_start_process(self._h, buf_kernel))

    def set_data(self, input: NTTInput) -> None:  # ntt_api.rs:72-87
        if isinstance(input.data, DeviceBuffer):
            check(lib().blz_ntt_set_data_device(self._h, input.buf_host, input.data.ptr, input.data.nbytes))
            return
        p, n, _k = buf_ptr(input.data)
        check(lib().blz_ntt_set_data(self._h, input.buf_host, p, n))

    def wait_result(self) -> None:  # ntt_api.rs:89-108
        check(lib().blz_ntt_wait_result(self._h))
        self._vec_keep = None

    def result(self, buf_num: Optional[int] = None) -> Optional[bytes]:  # ntt_api.rs:110-124
        if buf_num is None:
            raise TypeError("buf_num is required (the reference unwraps it: ntt_api.rs:113)")
        out = bytearray(self.nbytes)
        p, _, _k = buf_ptr(out)
        check(lib().blz_ntt_result(self._h, buf_num, p, self.nbytes))
        return out

    def result_into(self, buf_num: int, out) -> None:
        """result() into a caller-owned writable buffer (bytearray, numpy array ...) of 32 * n bytes: a host that
        keeps its output vector between transforms does not pay the first-touch page faults of a fresh 4 GiB
        allocation on every call (the C ABI takes the caller's pointer anyway)."""
        p, nb, _k = buf_ptr(out)
        if nb != self.nbytes:
            raise ValueError(f"result buffer holds {nb} bytes, the transform has {self.nbytes}")
        check(lib().blz_ntt_result(self._h, buf_num, p, self.nbytes))

    def exchange(self, buf_host: int, next_input, out) -> None:
        """result(buf_host) into `out` and set_data(NTTInput(buf_host, next_input)) as one full-duplex call
        (include/blaze_hip.h blz_ntt_exchange): what a cycle of ntt_parallel_test_correctness does on the buffer the
        kernel is not using (tests/integration_ntt.rs:102-136), with both directions of the link busy at once."""
        pi, ni, _k1 = buf_ptr(next_input)
        po, no, _k2 = buf_ptr(out)
        if no < self.nbytes:
            raise ValueError(f"result buffer holds {no} bytes, the transform has {self.nbytes}")
        check(lib().blz_ntt_exchange(self._h, buf_host, pi, ni, po, no))

    def info(self) -> dict:
        """Device bytes this client holds and which pass-2 kernel it runs (include/blaze_hip.h blz_ntt_info)."""
        v = (C.c_uint64 * 4)()
        check(lib().blz_ntt_info(self._h, v))
        return {"device_bytes": int(v[0]), "pass2_factor_table": bool(v[1]), "pass1_boundary_table": bool(v[2]), "log_size": int(v[3])}

    def result_device(self, buf_num: int, dst: DeviceBuffer) -> None:
        check(lib().blz_ntt_result_device(self._h, buf_num, dst.ptr, dst.nbytes))

    def reset(self) -> None:
        check(lib().blz_ntt_reset(self._h))
        self._vec_keep = None

    @staticmethod
    def _vec_arg(x):
        if x is None:
            return None
        if isinstance(x, DeviceBuffer):
            return BlzVecArg(x.ptr, 0, 0, x.nbytes // NTT_WORD_SIZE)
        return BlzVecArg(None, int(x), 0, 0)

    def vec_op(self, op: int, dst: int, a, b=None, c=None) -> None:
        """Element-wise op over the client's n positions (include/blaze_hip.h blz_ntt_vec_op): transform buffer `dst` =
        a + b (ADD), a - b (SUB), a * b (MUL), a * b + c (MULADD), a * b - c (MULSUB), 1 / a with 0 -> 0 (INV).  An int operand
        names a transform buffer (0 | 1, `dst` included: in place); a DeviceBuffer is device words, nbytes / 32 of them - a
        power of two up to n - read periodically along the buffer position (one word: a scalar).  Enqueued like a transform:
        wait_result() finishes it, last_kernel_ms() then reports it; the DeviceBuffers are kept alive until then and must not be
        written."""
        args = [self._vec_arg(x) for x in (a, b, c)]
        check(lib().blz_ntt_vec_op(self._h, int(op), dst, *[None if v is None else C.byref(v) for v in args]))
        self._vec_keep = (a, b, c)

    def vec_reduce(self, op: int, a, b=None, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """One value out of a vector (include/blaze_hip.h blz_ntt_vec_reduce): FOLD_SUM sum a[p], FOLD_DOT sum a[p] b[p],
        FOLD_EVAL sum a[p] z^p with z the one-word DeviceBuffer `b` (0^0 = 1).  Operands as for vec_op.  Returns the 32-byte
        DeviceBuffer the canonical result lands in (`out`, or a fresh one) once wait_result() has finished the op; the
        transform buffers named are only read."""
        if out is None:
            out = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE)
        args = [self._vec_arg(x) for x in (a, b)]
        check(lib().blz_ntt_vec_reduce(self._h, int(op), *[None if v is None else C.byref(v) for v in args], out.ptr))
        self._vec_keep = (a, b, out)
        return out

    def vec_scan(self, op: int, dst: int, a, exclusive: bool = False, total: Optional[DeviceBuffer] = None) -> None:
        """Prefix scan along the buffer (blz_ntt_vec_scan): transform buffer `dst`[p] = a[0] o .. o a[p] (SCAN_SUM, SCAN_PROD),
        or with exclusive=True the identity at p = 0 and a[0] o .. o a[p - 1] after it - an exclusive SCAN_PROD of a one-word
        DeviceBuffer z writes the powers z^p.  `a` may name `dst` (in place).  `total` (a 32-byte DeviceBuffer) receives the
        fold of all n elements.  Finished by wait_result()."""
        va = self._vec_arg(a)
        check(lib().blz_ntt_vec_scan(self._h, int(op), self.SCAN_EXCLUSIVE if exclusive else 0, dst,
                                     None if va is None else C.byref(va), None if total is None else total.ptr))
        self._vec_keep = (a, total)

    def vec_horner(self, dst: int, a, z: DeviceBuffer, exclusive: bool = False, reverse: bool = False,
                   total: Optional[DeviceBuffer] = None) -> None:
        """Weighted (Horner) scan along the buffer (blz_ntt_vec_horner): transform buffer `dst`[p] = a[p] + z dst[p - 1], with
        reverse=True a[p] + z dst[p + 1]; exclusive=True shifts the result by one position and puts 0 at the open end.  z is a
        one-word DeviceBuffer (scalar()); `a` may name `dst` (in place).  `total` (a 32-byte DeviceBuffer) receives the last
        inclusive value - with reverse=True that is a(z).  Finished by wait_result()."""
        va, vz = self._vec_arg(a), self._vec_arg(z)
        flags = (self.HORNER_EXCLUSIVE if exclusive else 0) | (self.HORNER_REVERSE if reverse else 0)
        check(lib().blz_ntt_vec_horner(self._h, flags, dst, None if va is None else C.byref(va), None if vz is None else C.byref(vz),
                                       None if total is None else total.ptr))
        self._vec_keep = (a, z, total)

    def vec_divide(self, dst: int, a, z: DeviceBuffer, rem: Optional[DeviceBuffer] = None) -> None:
        """Division by X - z: transform buffer `dst` = the n coefficients of the quotient of a(X) = sum a[p] X^p by X - z (the top
        one is 0), `rem` (a 32-byte DeviceBuffer) = the remainder a(z).  A reverse, exclusive vec_horner."""
        self.vec_horner(dst, a, z, exclusive=True, reverse=True, total=rem)
        self._vec_keep = (a, z, rem)

    def vec_gather(self, dst: int, a, offset: int = 0, stride: int = 1, length: Optional[int] = None) -> None:
        """Gather along the buffer (blz_ntt_vec_gather): transform buffer `dst`[p] = a[(offset + stride p) mod count] for
        p < length and 0 for length <= p < n.  `a` is a transform buffer (count = n; `dst` itself: in place, through the
        client's scratch at twice the traffic) or a DeviceBuffer of count = nbytes / 32 words, a power of two that may exceed n
        (up to 2^27).  A negative offset or stride is taken modulo count (stride -1 walks backwards); length=None means
        min(count, n).  Every output word is canonical.  Finished by wait_result()."""
        va = self._vec_arg(a)
        n = 1 << self.log_size
        count = n if va is None or not va.d_ptr else int(va.count)
        m = count or 1   # (a count of 0 is the library's to refuse)
        offset, stride = int(offset), int(stride)
        view = BlzVecView(offset % m if offset < 0 else offset, stride % m if stride < 0 else stride,
                          min(count, n) if length is None else int(length))
        check(lib().blz_ntt_vec_gather(self._h, dst, None if va is None else C.byref(va), C.byref(view)))
        self._vec_keep = (a,)

    def vec_rotate(self, dst: int, a, k: int) -> None:
        """Rotation: transform buffer `dst`[p] = a[(p + k) mod n], k of either sign - on the domain, rotating the values of
        Z(X) by 1 gives those of Z(wX); on a 4n coset, by 4.  `a` is a transform buffer or a DeviceBuffer of n words.  A
        vec_gather with stride 1."""
        n = 1 << self.log_size
        if isinstance(a, DeviceBuffer) and a.nbytes != self.nbytes:
            raise ValueError(f"a rotation takes n = {n} words, the DeviceBuffer holds {a.nbytes // NTT_WORD_SIZE}")
        self.vec_gather(dst, a, offset=int(k) % n, stride=1, length=n)
        self._vec_keep = (a,)

    def vec_extend(self, dst: int, a: DeviceBuffer) -> None:
        """Low-degree extension: transform buffer `dst` = the m <= n words of the DeviceBuffer `a` (m a power of two) with
        zeros above them - n coefficients into a 4n client.  A vec_gather with length = m."""
        self.vec_gather(dst, a, offset=0, stride=1, length=a.nbytes // NTT_WORD_SIZE)
        self._vec_keep = (a,)

    def vec_scatter(self, dst: int, idx: DeviceBuffer, x=None, val: Optional[DeviceBuffer] = None, src: Optional[DeviceBuffer] = None,
                    nnz: Optional[int] = None) -> None:
        """Scatter-add (blz_ntt_vec_scatter): transform buffer `dst`[t] = sum over k < nnz with idx[k] mod n == t of
        val[k] x[src(k) mod count], src(k) = src[k] or, without `src`, k; a position no nonzero names becomes 0.  `idx` and `src`
        are uint32 DeviceBuffers (nnz = idx.nbytes / 4 entries unless `nnz` says less), `val` 32-byte words (None: every
        coefficient is 1).  `x` is the other transform buffer or a DeviceBuffer of count = nbytes / 32 words (a power of two up
        to 2^27; one word: a scalar), None: every x word is 1 - and then `src` must be None; it may not name `dst`.  Without x
        and val it is the histogram of idx (vec_count).  With idx = col, src = the row of each nonzero and x = y it is the
        transposed sparse product A^T y.  Exact in the field: two runs give the same bytes.  Finished by wait_result()."""
        vx = self._vec_arg(x)
        if nnz is None:
            nnz = idx.nbytes // 4 if idx is not None else 0
        s = BlzVecScatter(None if idx is None else idx.ptr, None if src is None else src.ptr, None if val is None else val.ptr, int(nnz), 0)
        check(lib().blz_ntt_vec_scatter(self._h, dst, None if vx is None else C.byref(vx), C.byref(s)))
        self._vec_keep = (x, idx, src, val)

    def vec_count(self, dst: int, idx: DeviceBuffer, nnz: Optional[int] = None) -> None:
        """Multiplicities: transform buffer `dst`[t] = the number of entries k < nnz of the uint32 DeviceBuffer `idx` with
        idx[k] mod n == t, as a field element - the column m of a lookup argument beside the looked-up column vec_index makes
        from the same indices.  A vec_scatter without x and val."""
        self.vec_scatter(dst, idx, nnz=nnz)
        self._vec_keep = (idx,)

    def vec_spmv(self, dst: int, x, col: DeviceBuffer, row_ptr: Optional[DeviceBuffer] = None, val: Optional[DeviceBuffer] = None,
                 rows: Optional[int] = None, nnz: Optional[int] = None, row0: int = 0) -> None:
        """Sparse matrix times vector (blz_ntt_vec_spmv): transform buffer `dst`[p] = sum over row_ptr[p] <= k < row_ptr[p + 1] of
        val[k] x[col[k] mod count] for p < rows, 0 for an empty row and for rows <= p < n.  `x` is the other transform buffer or a
        DeviceBuffer of count = nbytes / 32 words (a power of two up to 2^27); it may not name `dst`.  `col` (uint32, nnz =
        nbytes / 4 entries unless `nnz` says less), `row_ptr` (uint32, rows + 1 entries; rows = nbytes / 4 - 1 - row0 unless
        `rows` says less) and `val` (32-byte words, None: every coefficient is 1) are DeviceBuffers.  row0 = r0 passes the slab
        of rows from r0 on (row_ptr + r0 with the full col / val arrays).  row_ptr=None is index mode: row p is nonzero p
        (vec_index).  Every output word is canonical.  Finished by wait_result()."""
        vx = self._vec_arg(x)
        if nnz is None:
            nnz = col.nbytes // 4 if col is not None else 0
        if row_ptr is None:
            rows = nnz if rows is None else rows
            rp = None
        else:
            rows = row_ptr.nbytes // 4 - 1 - int(row0) if rows is None else rows
            if int(row0) < 0 or int(row0) + int(rows) + 1 > row_ptr.nbytes // 4:
                raise ValueError(f"rows {rows} from row {row0} on need {int(row0) + int(rows) + 1} row pointers, the DeviceBuffer holds {row_ptr.nbytes // 4}")
            rp = row_ptr.ptr + 4 * int(row0)
        m = BlzVecCsr(rp, None if col is None else col.ptr, None if val is None else val.ptr, int(rows), int(nnz))
        check(lib().blz_ntt_vec_spmv(self._h, dst, None if vx is None else C.byref(vx), C.byref(m)))
        self._vec_keep = (x, col, row_ptr, val)

    def vec_index(self, dst: int, x, col: DeviceBuffer, val: Optional[DeviceBuffer] = None) -> None:
        """Data-dependent gather: transform buffer `dst`[p] = x[col[p] mod count] (times val[p] with `val`) for p < nbytes / 4
        entries of the uint32 DeviceBuffer `col`, 0 above - a PLONK wire column w[ia[p]], a looked-up column t[idx[p]], a
        permutation held as an index table.  A vec_spmv without row_ptr."""
        self.vec_spmv(dst, x, col, val=val)
        self._vec_keep = (x, col, val)

    def _mle_len(self, length, *tables) -> int:
        """The live length of a multilinear op: `length`, or the shortest table named (a transform buffer holds n words)."""
        if length is not None:
            return int(length)
        n = 1 << self.log_size
        return min(x.nbytes // NTT_WORD_SIZE if isinstance(x, DeviceBuffer) else n for x in tables)

    def vec_mle_fold(self, dst, a, r: DeviceBuffer, length: Optional[int] = None, low: bool = False) -> None:
        """Bind one variable of a multilinear table (blz_ntt_vec_mle_fold): dst[p] = lo + r (hi - lo) for p < length / 2, with
        (lo, hi) = (a[p], a[p + length / 2]) - the top variable - or, low=True, (a[2p], a[2p + 1]) - variable 0.  `dst` is an int
        (a transform buffer) or a DeviceBuffer (device words); exactly length / 2 words of it are written, every other byte keeps
        its value.  `dst` may be `a` itself (in place).  `r` is a one-word DeviceBuffer (scalar()) the host never reads;
        length=None means all of `a`.  Finished by wait_result()."""
        vd, va, vr = self._vec_arg(dst), self._vec_arg(a), self._vec_arg(r)
        check(lib().blz_ntt_vec_mle_fold(self._h, self.MLE_LOW if low else 0, *[None if v is None else C.byref(v) for v in (vd, va, vr)],
                                         self._mle_len(length, a)))
        self._vec_keep = (dst, a, r)

    def vec_mle_round(self, a, b=None, c=None, points: Optional[int] = None, length: Optional[int] = None, low: bool = False,
                      out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """One round polynomial of a sumcheck (blz_ntt_vec_mle_round): out[t] = sum over p < length / 2 of the product over the k
        tables given (a, then b, then c) of lo + t (hi - lo), for t = 0 .. points - 1, pairing as in vec_mle_fold.  points (1 .. 4)
        defaults to k + 1, the number of values that determines the polynomial.  Returns the DeviceBuffer of points x 32 bytes the
        canonical values land in (`out`, or a fresh one) once wait_result() has finished the op; nothing else is written."""
        k = 1 + (b is not None) + (c is not None)
        points = k + 1 if points is None else int(points)
        if out is None:
            out = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * max(points, 1))
        args = [self._vec_arg(x) for x in (a, b, c)]
        check(lib().blz_ntt_vec_mle_round(self._h, self.MLE_LOW if low else 0, *[None if v is None else C.byref(v) for v in args], points,
                                          self._mle_len(length, *[x for x in (a, b, c) if x is not None]), out.ptr))
        self._vec_keep = (a, b, c, out)
        return out

    def vec_mle_eq(self, dst, point: Optional[DeviceBuffer], m: Optional[int] = None) -> None:
        """The equality table (blz_ntt_vec_mle_eq): dst[p] = prod over i < m of (x_i tau_i + (1 - x_i)(1 - tau_i)) for p < 2^m, x_i
        bit i of p and tau_i word i of the DeviceBuffer `point` (m = nbytes / 32 unless `m` says less; m = 0, for which point may
        be None, writes the single word 1).  `dst` is an int (a transform buffer) or a DeviceBuffer; exactly 2^m words of it are
        written.  The host never reads the point.  Finished by wait_result()."""
        vd = self._vec_arg(dst)
        if m is None:
            m = 0 if point is None else point.nbytes // NTT_WORD_SIZE
        check(lib().blz_ntt_vec_mle_eq(self._h, None if vd is None else C.byref(vd), None if point is None else point.ptr, int(m)))
        self._vec_keep = (dst, point)

    def sumcheck_step(self, tables, r: Optional[DeviceBuffer] = None, gate: int = GATE_PRODUCT, points: Optional[int] = None,
                      length: Optional[int] = None, out: Optional[DeviceBuffer] = None) -> Optional[DeviceBuffer]:
        """One step of a sumcheck in one pass (blz_ntt_sumcheck_step).  `tables` are the gate's operands in order - ints
        (transform buffers) or DeviceBuffers -: GATE_PRODUCT takes 1 to 3 (G = a, a b, a b c), GATE_R1CS four (G = a (b c - d)).
        With `r` (a one-word DeviceBuffer the host never reads) every table is folded IN PLACE, T[p] = T[p] + r (T[p + length / 2]
        - T[p]) for p < length / 2 - exactly length / 2 words of each are written - and out[t], t < points, is the round
        polynomial of the folded tables: what vec_mle_round at length / 2 would return.  Without `r` it is the round polynomial
        of the tables as they are (a sumcheck's first round; nothing is written to a table).  points defaults to the gate's degree
        + 1 (4 for GATE_R1CS); points=0 (with r) binds only and returns None - a sumcheck's last variable.  Otherwise returns the
        DeviceBuffer of points x 32 bytes the canonical values land in (`out`, or a fresh one).  Both transform buffers may be
        tables; with `r` neither can then be read or written until wait_result() has finished the op."""
        tables = list(tables)
        if len(tables) > 4:
            raise ValueError(f"a gate takes at most four tables, {len(tables)} given")
        if points is None:
            points = 4 if gate == self.GATE_R1CS else len(tables) + 1
        points = int(points)
        if out is None and points > 0:
            out = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * points)
        args = [self._vec_arg(x) for x in tables + [None] * (4 - len(tables)) + [r]]
        check(lib().blz_ntt_sumcheck_step(self._h, int(gate), *[None if v is None else C.byref(v) for v in args], points,
                                          self._mle_len(length, *(tables or [0])), None if out is None else out.ptr))
        self._vec_keep = (*tables, r, out)
        return out if points > 0 else None

    @staticmethod
    def _sum_gate(tables, terms, common, max_tables=GATE_MAX_TABLES):
        """The blz_sum_gate of (tables, terms, common) - sumcheck_gate's conventions, gate_eval's too, and the terms of
        gate_eval_lin, which allows more tables - and its longest term's length"""
        terms = list(terms)
        if len(tables) > max_tables or len(terms) > GATE_MAX_TERMS:
            raise ValueError(f"a gate takes at most {max_tables} tables and {GATE_MAX_TERMS} terms, {len(tables)} and {len(terms)} given")
        gate = BlzSumGate(len(tables), len(terms), -1 if common is None else int(common), 0)
        degree = 0
        for m, (sign, factors) in enumerate(terms):
            factors = [int(f) for f in factors]
            if sign not in (1, -1) or len(factors) > 255 or any(f < 0 or f > 255 for f in factors):
                raise ValueError(f"term {m}: a term is (+1 | -1, [table indices])")
            gate.term[m].nfactors, gate.term[m].negate = len(factors), int(sign < 0)
            for j, f in enumerate(factors[:GATE_MAX_FACTORS]):   # (a longer term is the library's to refuse: nfactors says so)
                gate.term[m].factor[j] = f
            degree = max(degree, len(factors))
        return gate, degree

    def sumcheck_gate(self, tables, terms, common: Optional[int] = None, r: Optional[DeviceBuffer] = None, points: Optional[int] = None,
                      length: Optional[int] = None, out: Optional[DeviceBuffer] = None) -> Optional[DeviceBuffer]:
        """sumcheck_step for a caller-defined gate (blz_ntt_sumcheck_gate): G = tables[common] x sum of the signed products
        `terms`, a list of (sign, [table indices]) - sign +1 / -1, 1 to 4 indices into `tables` (at most 12 ints / DeviceBuffers),
        an index may repeat, `common` (None: no common factor) may also be a factor.  A vanilla PLONK zerocheck over
        [eq, qL, qR, qM, qO, qC, a, b, c] is common=0, terms=[(1, [1, 6]), (1, [2, 7]), (1, [3, 6, 7]), (-1, [4, 8]), (1, [5])].
        With `r` EVERY table is folded in place - named by a term or not - and out[t], t < points, is the round polynomial of
        the folded tables; without `r` the round alone (nothing is written; periodic tables allowed, a constant selector is a
        one-word DeviceBuffer).  points defaults to the gate's degree + 1 and is at most 6; points=0 (with r) binds only and
        returns None.  length=None means the longest table named."""
        tables = list(tables)
        gate, degree = self._sum_gate(tables, terms, common)
        if points is None:
            points = degree + (common is not None) + 1
        points = int(points)
        if out is None and points > 0:
            out = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * points)
        args = (BlzVecArg * max(len(tables), 1))(*[self._vec_arg(x) for x in tables])
        vr = self._vec_arg(r)
        if length is None:
            n = 1 << self.log_size
            length = max([x.nbytes // NTT_WORD_SIZE if isinstance(x, DeviceBuffer) else n for x in tables] or [0])
        check(lib().blz_ntt_sumcheck_gate(self._h, C.byref(gate), args, None if vr is None else C.byref(vr), points, int(length),
                                          None if out is None else out.ptr))
        self._vec_keep = (*tables, r, out)
        return out if points > 0 else None

    def zerocheck_gate(self, tables, terms, weight: DeviceBuffer, common: Optional[int] = None, r: Optional[DeviceBuffer] = None,
                       points: Optional[int] = None, length: Optional[int] = None, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """The gate step of a zerocheck sum_p eq(tau, p) G(p) (blz_ntt_zerocheck_gate): sumcheck_gate with the equality table out
        of the gate and the summed weight table `weight` in its place.  `tables`, `terms`, `common` follow sumcheck_gate's
        conventions and describe G alone.  `weight` is a DeviceBuffer of a power of two of words - for round 0 what
        vec_mle_eq(weight, point, m - 1) writes, half the tables' length.  Without `r` out[t] = sum_p weight[p] G(pair p at t),
        p < length / 2 (the weight may be periodic), and nothing else is written.  With `r` every table is folded in place, the
        weight's first length / 4 words become weight[q] + weight[q + length / 4] - the next round's weight, no product - and
        out[t] is the weighted round polynomial of the folded tables; the weight holds at least length / 2 words.  out is u_i of
        s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X): the caller multiplies the linear factor back in.  points defaults to the gate's
        degree + 1 - nothing is added for the weight - and is 1 to 6; a zerocheck's last op, the bind alone, is
        sumcheck_gate(points=0).  length=None means the longest table named."""
        tables = list(tables)
        gate, degree = self._sum_gate(tables, terms, common)
        if points is None:
            points = degree + (common is not None) + 1
        points = int(points)
        if out is None:
            out = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * max(points, 1))
        args = (BlzVecArg * max(len(tables), 1))(*[self._vec_arg(x) for x in tables])
        vw, vr = self._vec_arg(weight), self._vec_arg(r)
        if length is None:
            n = 1 << self.log_size
            length = max([x.nbytes // NTT_WORD_SIZE if isinstance(x, DeviceBuffer) else n for x in tables] or [0])
        check(lib().blz_ntt_zerocheck_gate(self._h, C.byref(gate), args, None if vw is None else C.byref(vw), None if vr is None else C.byref(vr),
                                           points, int(length), out.ptr))
        self._vec_keep = (*tables, weight, r, out)
        return out

    @staticmethod
    def _rotations(rot, ntables):
        """`rot` of gate_eval / gate_eval_lin as the C array: one integer per table, taken modulo 2^64; None stays None (all zero)"""
        if rot is None:
            return None
        rot = [int(k) for k in rot]
        if len(rot) != ntables:
            raise ValueError(f"rot holds one rotation per table: {len(rot)} for {ntables} tables")
        return (C.c_uint64 * max(len(rot), 1))(*[k & 0xFFFFFFFFFFFFFFFF for k in rot])

    def gate_eval(self, dst, tables, terms, common: Optional[int] = None, rot=None, length: Optional[int] = None) -> None:
        """A caller-defined gate evaluated position by position (blz_ntt_gate_eval): dst[p] = tables[common][p_c] x sum of the
        signed products `terms`, for p < length, with table i read at p_i = (p + rot[i]) mod its count.  `tables` and `terms`
        follow sumcheck_gate's conventions - ints (transform buffers) or DeviceBuffers of a power of two of words up to n, read
        periodically (one word: a scalar); terms a list of (sign, [table indices]).  The PLONK quotient numerator over
        [qL, qR, qM, qO, qC, a, b, c] is terms=[(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (-1, [3, 7]), (1, [4])].  `rot` is one
        integer per table (None: all zero), taken modulo 2^64: -1 reads the previous row.  `dst` is an int or a DeviceBuffer;
        exactly `length` words of it (None: n) are written, every other byte keeps its value.  `dst` may be one of the tables -
        dst <- dst + alpha a b is one op - if that table is not rotated.  Finished by wait_result()."""
        tables = list(tables)
        gate, _ = self._sum_gate(tables, terms, common)
        args = (BlzVecArg * max(len(tables), 1))(*[self._vec_arg(x) for x in tables])
        vd = self._vec_arg(dst)
        rots = self._rotations(rot, len(tables))
        if length is None:
            length = 1 << self.log_size
        check(lib().blz_ntt_gate_eval(self._h, C.byref(gate), None if vd is None else C.byref(vd), args, rots, int(length)))
        self._vec_keep = (dst, *tables)

    def gate_eval_lin(self, dst, tables, forms, terms, common: Optional[int] = None, rot=None, length: Optional[int] = None) -> None:
        """gate_eval with linear-form factors (blz_ntt_gate_eval_lin) - products of sums: dst[p] = C(p) x sum of the signed
        products `terms`, where a factor, and `common`, is a table index or FORM + k, the value of forms[k].  `forms` is a list
        of at most 8 forms; a form is a list of 1 to 4 summands (sign, coef, table): sign +1 / -1, `table` an index into
        `tables`, `coef` the index of the table whose word multiplies it or None for 1.  `tables` holds at most 16 ints
        (transform buffers) / DeviceBuffers, read periodically, with one rotation each in `rot` (None: all zero) whatever names
        the index; a one-word coefficient (beta, gamma) costs one product per position, a longer one two; a constant is a
        one-word table with coef None.  The numerator column prod_j (w_j + beta id_j + gamma) over [a, b, c, id1, id2, id3, beta,
        gamma] is forms=[[(1, None, j), (1, 6, 3 + j), (1, None, 7)] for j in range(3)], terms=[(1, [FORM, FORM + 1, FORM + 2])].
        `dst`, `length` and in place as for gate_eval: exactly `length` words (None: n) are written, and `dst` may be an
        unrotated table that a factor, a summand or a coefficient names.  Finished by wait_result()."""
        tables, forms = list(tables), [list(f) for f in forms]
        if len(forms) > LIN_MAX_FORMS:
            raise ValueError(f"a gate takes at most {LIN_MAX_FORMS} forms, {len(forms)} given")
        sums, _ = self._sum_gate(tables, terms, common, LIN_MAX_TABLES)   # a factor FORM + k is a byte like any other
        gate = BlzLinGate(sums.ntables, sums.nterms, sums.common, len(forms), sums.term)
        for k, form in enumerate(forms):
            gate.form[k].nsummands = min(len(form), 255)   # (a longer form is the library's to refuse)
            for s, (sign, coef, table) in enumerate(form[:LIN_MAX_SUMMANDS]):
                if sign not in (1, -1) or not 0 <= int(table) < 256 or not (coef is None or 0 <= int(coef) < LIN_NO_COEF):
                    raise ValueError(f"form {k}, summand {s}: (sign, coef, table) with sign +1 or -1, coef None or a table index, table a table index")
                x = gate.form[k].summand[s]
                x.coef, x.table, x.negate = LIN_NO_COEF if coef is None else int(coef), int(table), int(sign < 0)
        args = (BlzVecArg * max(len(tables), 1))(*[self._vec_arg(x) for x in tables])
        vd = self._vec_arg(dst)
        rots = self._rotations(rot, len(tables))
        if length is None:
            length = 1 << self.log_size
        check(lib().blz_ntt_gate_eval_lin(self._h, C.byref(gate), None if vd is None else C.byref(vd), args, rots, int(length)))
        self._vec_keep = (dst, *tables)

    @staticmethod
    def tree_layer(length: int, k: int):
        """(word offset, words) of layer k, 1 <= k <= log2(length), in a destination of mle_tree: layer 1 at 0, layer 2 at
        length / 2, the root at length - 2"""
        length, k = int(length), int(k)
        if length < 2 or length & (length - 1) or not 1 <= k < length.bit_length():
            raise ValueError(f"layer {k} of a tree over {length} words: length is 2^m >= 2 and 1 <= k <= m")
        return length - (length >> (k - 1)), length >> k

    def mle_tree(self, dst, a, op: int = TREE_PROD, length: Optional[int] = None, low: bool = False, dst_q=None, a_q=None) -> None:
        """Every layer of the product or fraction tree under a multilinear table (blz_ntt_mle_tree).  Layer 0 is `a`, `length`
        = 2^m words of it (None: all of it), read periodically; layer k holds length / 2^k words and lands at tree_layer(length,
        k) of `dst`: length - 1 words are written, every other byte keeps its value.  (lo, hi) = (L[p], L[p + size / 2]) - the
        top variable, so the halves of a layer are views (DeviceBuffer.view) the step ops take as tables - or, low=True,
        (L[2p], L[2p + 1]).  TREE_PROD: L'[p] = lo hi, a grand product.  TREE_FRAC: numerators `a` -> `dst` and denominators
        `a_q` -> `dst_q`, (P, Q)' = (P_lo Q_hi + P_hi Q_lo, Q_lo Q_hi) - logUp's sum of fractions, never inverted; a one-word `a`
        holding 1 is the numerator of sum 1 / (beta + f).  Operands are ints (transform buffers) or DeviceBuffers; a destination
        may not overlap a source or the other destination.  Finished by wait_result()."""
        args = [self._vec_arg(x) for x in (dst, dst_q, a, a_q)]
        check(lib().blz_ntt_mle_tree(self._h, int(op), self.MLE_LOW if low else 0, *[None if v is None else C.byref(v) for v in args],
                                     self._mle_len(length, *[x for x in (a, a_q) if x is not None] or [0])))
        self._vec_keep = (dst, dst_q, a, a_q)

    def fs_challenge(self, state: DeviceBuffer, words=None, count: Optional[int] = None, r: Optional[DeviceBuffer] = None) -> Optional[DeviceBuffer]:
        """One step of the on-device Fiat-Shamir transcript (blz_ntt_fs_challenge): SHA3-256 of `state` (a one-word DeviceBuffer,
        read and written) followed by the first `count` words of `words` (an int - a transform buffer - or a DeviceBuffer; count=None
        means all of a DeviceBuffer, at most 32) exactly as stored.  The digest becomes the new state; with every bit from
        bitlen(modulus) - 1 upward cleared it is the challenge written to `r`, a one-word DeviceBuffer that a step op takes as its
        r without the host ever reading it.  r=None absorbs only.  blaze_amd.fiat_shamir.absorb is the host's mirror.  Returns
        `r`; finished by wait_result()."""
        if count is None:
            count = 0 if words is None else (words.nbytes // NTT_WORD_SIZE if isinstance(words, DeviceBuffer) else 1 << self.log_size)
        vw = self._vec_arg(words)
        check(lib().blz_ntt_fs_challenge(self._h, state.ptr, None if vw is None else C.byref(vw), int(count), None if r is None else r.ptr))
        self._vec_keep = (state, words, r)
        return r

    def sumcheck_prove(self, tables, terms, state: DeviceBuffer, weight: Optional[DeviceBuffer] = None, common: Optional[int] = None,
                       points: Optional[int] = None, length: Optional[int] = None, rounds: Optional[DeviceBuffer] = None,
                       challenges: Optional[DeviceBuffer] = None):
        """A whole sumcheck in ONE call (blz_ntt_sumcheck_prove): the round alone, then per variable fs_challenge over the round
        just written and the step with that challenge, then the bind alone - m = log2(length) rounds enqueued back to back, no
        host wait in between.  `tables`, `terms`, `common` describe the gate as for sumcheck_gate; weight=None proves the sum of
        G, a `weight` (DeviceBuffer, length / 2 words, as for zerocheck_gate) the sum of weight x G with zerocheck_gate's steps.
        `state` is the transcript, one word, read and left at the state after the last round.  points defaults to the gate's
        degree + 1 (+ 1 for a common factor), 1 to 6.  Returns (rounds, challenges): DeviceBuffers of m x points and m words
        (the ones passed, or fresh ones).  After wait_result() word 0 of every table is the table at the challenges, top
        variable first, and a verifier re-derives the challenges with blaze_amd.fiat_shamir.challenges."""
        tables = list(tables)
        gate, degree = self._sum_gate(tables, terms, common)
        if points is None:
            points = degree + (common is not None) + 1
        points = int(points)
        if length is None:
            n = 1 << self.log_size
            length = max([x.nbytes // NTT_WORD_SIZE if isinstance(x, DeviceBuffer) else n for x in tables] or [0])
        m = max(int(length).bit_length() - 1, 1)
        if rounds is None:
            rounds = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * m * max(points, 1))
        if challenges is None:
            challenges = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE * m)
        args = (BlzVecArg * max(len(tables), 1))(*[self._vec_arg(x) for x in tables])
        vw = self._vec_arg(weight)
        check(lib().blz_ntt_sumcheck_prove(self._h, C.byref(gate), args, None if vw is None else C.byref(vw), points, int(length),
                                           state.ptr, rounds.ptr, challenges.ptr))
        self._vec_keep = (*tables, weight, state, rounds, challenges)
        return rounds, challenges

    def gkr_prove(self, tree, a, state: DeviceBuffer, length: Optional[int] = None, weight: Optional[DeviceBuffer] = None,
                  rounds: Optional[DeviceBuffer] = None, points: Optional[DeviceBuffer] = None, claims: Optional[DeviceBuffer] = None,
                  fused: bool = True):
        """The GKR grand product over a product tree in ONE call (blz_ntt_gkr_prove).  `tree` is what mle_tree(tree, a) left
        (TREE_PROD, default pairing) over the `length` = 2^m leaves `a` (None: all of `a`); both are ints (transform buffers) or
        DeviceBuffers and both are consumed: the first half of each half-layer is scratch afterwards.  From the root down, layer
        j's claim is proven by a sumcheck under the weight eq(point of the layer above) with every challenge made on the device,
        then the two final words go to `claims` and through one more transcript step.  `state` is the transcript, one word, read
        and left at the state after the last step; the root is not absorbed.  `weight` is the scratch for the weight, max(length
        / 4, 1) words.  Returns (rounds, points, claims): DeviceBuffers of 3 m (m - 1) / 2, m (m + 1) / 2 and 2 m words (the
        ones passed, or fresh ones) laid out as blaze_amd.gkr.layout(m) says; blaze_amd.gkr.verify_product checks them and returns
        the leaves' claim and point.  fused=False takes the chain of single launches only (GKR_UNFUSED): the same bytes, slower.
        Finished by wait_result()."""
        from . import gkr
        length = self._mle_len(length, a)
        lay = gkr.layout(max(int(length).bit_length() - 1, 1))
        dev = self.driver_client.id
        if weight is None:
            weight = DeviceBuffer(dev, NTT_WORD_SIZE * lay.weight_words)
        if rounds is None:
            rounds = DeviceBuffer(dev, NTT_WORD_SIZE * max(lay.rounds_words, 1))
        if points is None:
            points = DeviceBuffer(dev, NTT_WORD_SIZE * lay.points_words)
        if claims is None:
            claims = DeviceBuffer(dev, NTT_WORD_SIZE * lay.claims_words)
        vt, va = self._vec_arg(tree), self._vec_arg(a)
        check(lib().blz_ntt_gkr_prove(self._h, self.TREE_PROD, 0 if fused else self.GKR_UNFUSED, C.byref(vt), C.byref(va), int(length), weight.ptr,
                                      state.ptr, rounds.ptr, points.ptr, claims.ptr))
        self._vec_keep = (tree, a, weight, state, rounds, points, claims)
        return rounds, points, claims

    def gkr_prove_frac(self, tree_p, tree_q, a_p, a_q, state: DeviceBuffer, length: Optional[int] = None, weight: Optional[DeviceBuffer] = None,
                       rounds: Optional[DeviceBuffer] = None, points: Optional[DeviceBuffer] = None, claims: Optional[DeviceBuffer] = None,
                       lambdas: Optional[DeviceBuffer] = None, fused: bool = True):
        """The GKR argument over a fraction tree (logUp-GKR) in ONE call (blz_ntt_gkr_prove_frac).  `tree_p`, `tree_q` are what
        mle_tree(tree_p, a_p, TREE_FRAC, dst_q=tree_q, a_q=a_q) left (default pairing) over the `length` = 2^m numerators `a_p`
        and denominators `a_q` (None: all of `a_p`); the four are ints (transform buffers) or DeviceBuffers, none periodic - a
        one-word numerator is expanded with vec_gather first - and all are consumed.  From the root down, layer j >= 1 draws a
        batching challenge lambda_j from the transcript, writes T = P_hi + lambda_j Q_hi over P_hi and proves
        P(tau) + lambda_j Q(tau) = sum eq(tau, p) (P_lo Q_hi + Q_lo T) by a sumcheck under the weight eq(point of the layer above)
        with every challenge made on the device; then the four final words (P_lo, P_hi, Q_lo, Q_hi at the challenges) go to
        `claims` and through one more transcript step.  `state` is the transcript, one word, read and left at the state after
        the last step; the roots are not absorbed.  `weight` is the scratch for the weight, max(length / 4, 1) words.  Returns
        (rounds, points, claims, lambdas): DeviceBuffers of 3 m (m - 1) / 2, m (m + 1) / 2, 4 m and m words (the ones passed,
        or fresh ones; word 0 of lambdas is never written) laid out as blaze_amd.gkr.layout_frac(m) says;
        blaze_amd.gkr.verify_fraction checks them and returns the leaves' claims and point.  fused=False takes the chain of
        single launches only (GKR_UNFUSED): the same bytes, slower.  Finished by wait_result()."""
        from . import gkr
        length = self._mle_len(length, a_p)
        lay = gkr.layout_frac(max(int(length).bit_length() - 1, 1))
        dev = self.driver_client.id
        if weight is None:
            weight = DeviceBuffer(dev, NTT_WORD_SIZE * lay.weight_words)
        if rounds is None:
            rounds = DeviceBuffer(dev, NTT_WORD_SIZE * max(lay.rounds_words, 1))
        if points is None:
            points = DeviceBuffer(dev, NTT_WORD_SIZE * lay.points_words)
        if claims is None:
            claims = DeviceBuffer(dev, NTT_WORD_SIZE * lay.claims_words)
        if lambdas is None:
            lambdas = DeviceBuffer(dev, NTT_WORD_SIZE * lay.lambdas_words)
        args = [self._vec_arg(x) for x in (tree_p, tree_q, a_p, a_q)]
        check(lib().blz_ntt_gkr_prove_frac(self._h, 0 if fused else self.GKR_UNFUSED, *[C.byref(v) for v in args], int(length), weight.ptr, state.ptr,
                                           rounds.ptr, points.ptr, claims.ptr, lambdas.ptr))
        self._vec_keep = (tree_p, tree_q, a_p, a_q, weight, state, rounds, points, claims, lambdas)
        return rounds, points, claims, lambdas

    def scalar(self, value: int) -> DeviceBuffer:
        """A one-element operand for vec_op: `value` (any 256-bit integer, taken as its residue) in device memory."""
        v = int(value)
        if v < 0 or v >> 256:
            raise ValueError("a vec_op operand word is a 256-bit unsigned integer")
        d = DeviceBuffer(self.driver_client.id, NTT_WORD_SIZE)
        d.upload(v.to_bytes(NTT_WORD_SIZE, "little"))
        return d

    def set_coset(self, shift: Optional[int]) -> None:
        """Transforms started from now on run on the coset shift * <w> (include/blaze_hip.h blz_ntt_set_coset): a forward client
        computes X[k] = sum_i x[i] shift^i w^(i k), an inverse one its exact inverse; None or 1: the plain transform again.
        0 < shift < r, checked on the device."""
        if shift is None:
            check(lib().blz_ntt_set_coset(self._h, None))
            return
        s = int(shift)
        if s < 0 or s >> 256:
            raise ValueError("the coset shift is a field element: 0 < shift < r")
        check(lib().blz_ntt_set_coset(self._h, s.to_bytes(32, "little")))

    @property
    def coset(self) -> int:
        """The shift in force; 1 when the client runs the plain transform."""
        out = bytearray(32)
        p, _, _k = buf_ptr(out)
        check(lib().blz_ntt_get_coset(self._h, p))
        return int.from_bytes(out, "little")

    # NTTBanks::preprocess / postprocess (ntt_data.rs:80-156) on device buffers
    def banks_preprocess(self, d_in: DeviceBuffer, d_banks: DeviceBuffer) -> None:
        check(lib().blz_ntt_banks_preprocess_device(self._h, d_in.ptr, d_banks.ptr))

    def banks_postprocess(self, d_banks: DeviceBuffer, d_out: DeviceBuffer) -> None:
        check(lib().blz_ntt_banks_postprocess_device(self._h, d_banks.ptr, d_out.ptr))

    def last_kernel_ms(self) -> float:
        v = C.c_float()
        check(lib().blz_ntt_last_kernel_ms(self._h, C.byref(v)))
        return float(v.value)
