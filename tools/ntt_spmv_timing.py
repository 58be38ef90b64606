#!/usr/bin/env python3
"""What a sparse matrix-vector product on resident buffers costs over the BLS12-381 scalar field (blz_ntt_vec_spmv; DESIGN.md
section 4, "Sparse products"): medians of blz_ntt_last_kernel_ms, each case beside ONE yardstick taken in the same process,
alternating with it inside every round - a device-to-device hipMemcpyAsync on the handle's stream, HIP-event timed, of the bytes
that case moves if every 32-byte word it uses were all it fetched (a copy of B bytes reads B and writes B).
    index mode on a 2^26 handle, buffer 0 -> buffer 1, no coefficients (k_spmv_index):
        index_identity      col[p] = p: reads 2 GiB of x and 256 MiB of col, writes 2 GiB
        index_permutation   col a random permutation: the same bytes USED; every 32-byte read lands in a line of its own
    CSR on a 2^24 handle, x = buffer 0, with coefficients (memset, k_spmv_tile, k_spmv_carry):
        csr_1_to_4          2^24 rows of 1 .. 4 nonzeros, random columns
        csr_one_long_row    the same nnz, col and val, half of the nonzeros in ONE row (row 0), the rest spread evenly
      per nonzero 4 bytes of col, 32 of val and 32 of x; per row 4 bytes of row_ptr; the destination is written twice (the
      memset's zeros, then the rows)
The last pair is the design's claim: the work is split by nonzeros, so the time does not follow the row lengths.
The outputs are checked on the device before anything is written, by code other than the op's own.  The sources are canonical
words, so an index-mode destination must equal torch's index_select of the source at col, all n positions compared as
4 x int64.  A CSR destination y = M x is checked against a random vector u through the identity
    sum_p u[p] y[p] = sum_k val[k] u[row of k] x[col[k]]:
the left side is a DOT on the 2^24 handle; for the right side torch gathers u[row of k] and x[col[k]] (the row of k by
searchsorted in row_ptr) into the buffers of a 2^26 handle, whose MUL and DOT do the arithmetic.
Writes profiles/ntt_spmv_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_spmv_timing.py [--out profiles/ntt_spmv_ops.json] [--rounds 9] [--log-size 26] [--timeout 540]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 1 << 20   # rows per piece of a torch gather


def child(rounds: int, logn: int) -> dict:
    import torch

    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import check, lib
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_ntt import NTT, NTTClient

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def hip_ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")

    N, n = 1 << logn, 1 << (logn - 2)      # the index handle's and the CSR handle's positions
    dc = DriverClient(0)
    big = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
    small = NTTClient(NTT.Ntt, dc, log_size=logn - 2, flags=NTTClient.NO_FACTOR_TABLE)
    stream, dev = C.c_void_p(), C.c_int()
    check(lib().blz_ntt_stream(big._h, C.byref(stream), C.byref(dev)))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def to_buffer(t):
        """a torch tensor's bytes in a DeviceBuffer of their own"""
        t = t.contiguous()
        d = DeviceBuffer(0, t.numel() * t.element_size())
        torch.cuda.synchronize()
        hip_ok(hip.hipMemcpyAsync(d.ptr, t.data_ptr(), d.nbytes, 3, stream), "hipMemcpyAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        return d

    def words_tensor(d, count):
        t = torch.empty((count, 4), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        hip_ok(hip.hipMemcpyAsync(t.data_ptr(), d.ptr, 32 * count, 3, stream), "hipMemcpyAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        return t

    def gather_rows(src, idx, out):
        for p0 in range(0, idx.numel(), PIECE):   # in pieces: torch refuses the launch of one index_select over 2^27 rows
            out[p0:p0 + PIECE] = src.index_select(0, idx[p0:p0 + PIECE])

    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(26)
    # ---- sources: canonical field elements
    words = DeviceBuffer(0, 32 * N)
    check(blaze_amd.aux().blz_synth_field_elements(0, words.ptr, N, 11))
    check(lib().blz_ntt_set_data_device(big._h, 0, words.ptr, words.nbytes))
    check(lib().blz_ntt_set_data_device(small._h, 0, words.ptr, 32 * n))   # x of the CSR cases: the first n words
    # ---- index mode
    ident = torch.arange(N, dtype=torch.int64, device="cuda:0")
    perm = torch.randperm(N, generator=gen, device="cuda:0")
    index_cols = {"index_identity": ident, "index_permutation": perm}
    index_bufs = {k: to_buffer(v.to(torch.int32)) for k, v in index_cols.items()}
    # ---- CSR: 1 .. 4 nonzeros per row, and the same nonzeros with half of them in row 0
    lengths = torch.randint(1, 5, (n,), generator=gen, device="cuda:0", dtype=torch.int64)
    rp_even = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(lengths, 0)])
    nnz = int(rp_even[-1])
    half = nnz // 2
    rp_skew = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"),
                         half + ((nnz - half) * torch.arange(0, n, dtype=torch.int64, device="cuda:0")) // (n - 1)])
    assert int(rp_skew[-1]) == nnz and int(rp_skew[1]) == half
    col = torch.randint(0, n, (nnz,), generator=gen, device="cuda:0", dtype=torch.int64)
    d_col = to_buffer(col.to(torch.int32))
    d_val = DeviceBuffer(0, 32 * N)          # N words: the check multiplies by them as a d_ptr operand of the 2^logn handle
    hip_ok(hip.hipMemsetAsync(d_val.ptr, 0, d_val.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    check(blaze_amd.aux().blz_synth_field_elements(0, d_val.ptr, nnz, 12))
    if nnz > N:
        raise RuntimeError("the check holds one word per nonzero in the larger handle")
    csr_rp = {"csr_1_to_4": rp_even, "csr_one_long_row": rp_skew}
    csr_bufs = {k: to_buffer(v.to(torch.int32)) for k, v in csr_rp.items()}

    def traffic(name):
        """(bytes read that the result uses, bytes written)"""
        if name in index_cols:
            return 32 * N + 4 * N, 32 * N
        return nnz * (4 + 32 + 32) + 4 * (n + 1), 2 * 32 * n

    names = list(index_cols) + list(csr_rp)
    most = max(sum(traffic(k)) // 2 for k in names)
    d_src, d_dst = DeviceBuffer(0, most), DeviceBuffer(0, most)
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def run_op(name):
        if name in index_cols:
            big.vec_index(1, 0, index_bufs[name])
            big.wait_result()
            return big.last_kernel_ms()
        small.vec_spmv(1, 0, d_col, row_ptr=csr_bufs[name], val=d_val, rows=n, nnz=nnz)
        small.wait_result()
        return small.last_kernel_ms()

    def run_copy(nbytes):
        ms = C.c_float()
        hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        hip_ok(hip.hipMemcpyAsync(d_dst.ptr, d_src.ptr, nbytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
        hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    op_ms = {k: [] for k in names}
    cp_ms = {k: [] for k in names}
    for it in range(rounds + 2):          # two warm-up rounds
        for k in names:
            a, b = run_op(k), run_copy(sum(traffic(k)) // 2)
            if it >= 2:
                op_ms[k].append(a)
                cp_ms[k].append(b)
    d_src.free()
    d_dst.free()

    # ---- the outputs, checked
    t_words = words_tensor(words, N)
    for k, idx in index_cols.items():
        run_op(k)
        got = torch.empty((N, 4), dtype=torch.int64, device="cuda:0")
        check(lib().blz_ntt_result_device(big._h, 1, got.data_ptr(), 32 * N))
        for p0 in range(0, N, PIECE):
            if not torch.equal(got[p0:p0 + PIECE], t_words.index_select(0, idx[p0:p0 + PIECE])):
                raise RuntimeError(f"{k}: the destination is not the source at col in positions {p0} .. {p0 + PIECE - 1}")
        del got
    u = DeviceBuffer(0, 32 * n)
    check(blaze_amd.aux().blz_synth_field_elements(0, u.ptr, n, 13))
    t_u = words_tensor(u, n)
    ks = torch.arange(nnz, dtype=torch.int64, device="cuda:0")
    sums = {}
    for k, rp in csr_rp.items():
        run_op(k)
        left = small.vec_reduce(NTTClient.FOLD_DOT, 1, u)
        small.wait_result()
        row_of = torch.searchsorted(rp, ks, right=True) - 1
        pad = torch.zeros((N, 4), dtype=torch.int64, device="cuda:0")
        gather_rows(t_words[:n], col, pad)            # x[col[k]]
        torch.cuda.synchronize()
        check(lib().blz_ntt_set_data_device(big._h, 0, pad.data_ptr(), 32 * N))
        gather_rows(t_u, row_of, pad)                 # u[row of k]
        torch.cuda.synchronize()
        check(lib().blz_ntt_set_data_device(big._h, 1, pad.data_ptr(), 32 * N))
        del pad, row_of
        big.vec_op(NTTClient.MUL, 1, 1, d_val)
        big.wait_result()
        right = big.vec_reduce(NTTClient.FOLD_DOT, 0, 1)
        big.wait_result()
        lw, rw = bytes(left.download(32)), bytes(right.download(32))
        if lw != rw or not any(lw):
            raise RuntimeError(f"{k}: sum u[p] (M x)[p] = {lw.hex()} but sum val[k] u[row k] x[col k] = {rw.hex()}")
        sums[k] = lw.hex()
    if len(set(sums.values())) != 2:
        raise RuntimeError("the two matrices gave the same product: the check would not tell them apart")
    for cl in (big, small):
        cl.close()

    res = {"log_size_index": logn, "log_size_csr": logn - 2, "field": "BLS381", "rounds": rounds, "checked": True,
           "csr": {"rows": n, "nnz": nnz, "longest_row_1_to_4": 4, "longest_row_skewed": half}, "cases": {}}
    for k in names:
        om, cm = statistics.median(op_ms[k]), statistics.median(cp_ms[k])
        rd, wr = traffic(k)
        res["cases"][k] = {
            "kernels": "k_spmv_index<false>" if k in index_cols else "hipMemsetAsync, k_spmv_tile<true>, k_spmv_carry",
            "bytes_read_used": rd, "bytes_written": wr, "yardstick_copy_bytes": (rd + wr) // 2,
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "achieved_tb_per_s": round((rd + wr) / om / 1e9, 3),
            "yardstick_copy_ms": round(cm, 4), "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_copy": round(om / cm, 4),
        }
    c = res["cases"]
    res["one_long_row_over_1_to_4"] = round(c["csr_one_long_row"]["kernel_ms"] / c["csr_1_to_4"]["kernel_ms"], 4)
    res["permutation_over_identity"] = round(c["index_permutation"]["kernel_ms"] / c["index_identity"]["kernel_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_spmv_ops.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log-size", type=int, default=26)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.rounds, a.log_size)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds),
                        "--log-size", str(a.log_size)], capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"the measuring process ended with status {r.returncode}: nothing written")
        return r.returncode
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
