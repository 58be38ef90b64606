#!/usr/bin/env python3
"""What a scatter-add on resident buffers costs over the BLS12-381 scalar field (blz_ntt_vec_scatter; DESIGN.md section 4,
"Scatter-add"): medians of blz_ntt_last_kernel_ms, each case beside TWO yardsticks taken in the same process, alternating with
it inside every round - blz_ntt_vec_index over the same nnz indices (the gather that reads what the scatter writes; on the 2^24
handle, 2^24 indices a call, from a table of the case's n words), and a device-to-device hipMemcpyAsync on the handle's stream,
HIP-event timed, of the bytes the case moves if every word it uses were all it fetched and every add were a plain store (a copy
of B bytes reads B and writes B).
    count_2e24            n = 2^24, nnz = 2^24 uniform indices              memset, k_scatter_count, k_scatter_count_fin
    add_val_2e24          n = 2^24, nnz = 2^24 uniform, with val            2 memsets, k_scatter_add<0,1>, k_scatter_fin
    add_transpose_2e25    n = 2^24, nnz = 2^25 uniform, x, val and src      2 memsets, k_scatter_add<1,1>, k_scatter_fin: A^T y
    count_lds_2e12        n = 2^12, nnz = 2^24 uniform                      k_scatter_count_lds
    add_lds_2e10          n = 2^10, nnz = 2^24 uniform, with val            k_scatter_add_lds<0,1>
    add_contended_2e24    n = 2^24, nnz = 2^24, every index equal, val      the contended worst case of k_scatter_add
The outputs are checked before anything is timed, by code other than the op's own.  A histogram must equal torch.bincount of
the masked indices, all n positions compared as 4 x int64.  An add is checked against a random vector u through the identity
    sum_t u[t] dst[t] = sum_k val[k] x[src(k)] u[idx[k]]:
the left side is a DOT of the destination with u; the right side, 2^24 nonzeros at a time, is vec_index of u at idx into one
buffer of the 2^24 handle, vec_index of x at src with the coefficients val into the other (val alone: the words themselves),
and their DOT, the pieces added as Python integers modulo r.  The small handles take u periodically, n words of it.
Writes profiles/ntt_scatter_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_scatter_timing.py [--out profiles/ntt_scatter_ops.json] [--rounds 9] [--log-size 24] [--timeout 540]
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

R_BLS381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


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

    N = 1 << logn
    dc = DriverClient(0)
    handles = {lg: NTTClient(NTT.Ntt, dc, log_size=lg, flags=NTTClient.NO_FACTOR_TABLE) for lg in (logn, 12, 10)}
    big = handles[logn]
    stream, dev = C.c_void_p(), C.c_int()
    check(lib().blz_ntt_stream(big._h, C.byref(stream), C.byref(dev)))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def copy_bytes(dst, src, nbytes):
        torch.cuda.synchronize()
        hip_ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, stream), "hipMemcpyAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def to_buffer(t):
        """a torch tensor's bytes in a DeviceBuffer of their own"""
        t = t.contiguous()
        d = DeviceBuffer(0, t.numel() * t.element_size())
        copy_bytes(d.ptr, t.data_ptr(), d.nbytes)
        return d

    def synth(count, seed):
        d = DeviceBuffer(0, 32 * count)
        check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, count, seed))
        return d

    def piece(d, first, count, unit):
        """`count` entries of `unit` bytes of d from entry `first` on, in a DeviceBuffer of their own"""
        out = DeviceBuffer(0, count * unit)
        copy_bytes(out.ptr, d.ptr + first * unit, out.nbytes)
        return out

    def word(d):
        return int.from_bytes(bytes(d.download(32)), "little")

    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(27)
    uniform = torch.randint(0, 1 << 32, (2 * N,), generator=gen, device="cuda:0", dtype=torch.int64)   # masked by the op
    rows = torch.randint(0, 1 << 32, (2 * N,), generator=gen, device="cuda:0", dtype=torch.int64)
    d_uniform, d_rows = to_buffer(uniform.to(torch.int32)), to_buffer(rows.to(torch.int32))
    equal = torch.full((N,), 12345, dtype=torch.int64, device="cuda:0")
    d_equal = to_buffer(equal.to(torch.int32))
    d_val, d_x, d_u = synth(2 * N, 21), synth(N, 22), synth(N, 23)
    # name: (log n, nnz, indices, their tensor, x, val, src)
    cases = {
        "count_2e24": (logn, N, d_uniform, uniform, None, None, None),
        "add_val_2e24": (logn, N, d_uniform, uniform, None, d_val, None),
        "add_transpose_2e25": (logn, 2 * N, d_uniform, uniform, d_x, d_val, d_rows),
        "count_lds_2e12": (12, N, d_uniform, uniform, None, None, None),
        "add_lds_2e10": (10, N, d_uniform, uniform, None, d_val, None),
        "add_contended_2e24": (logn, N, d_equal, equal, None, d_val, None),
    }
    kernels = {
        "count_2e24": "hipMemsetAsync, k_scatter_count, k_scatter_count_fin", "add_val_2e24": "2 x hipMemsetAsync, k_scatter_add<0,1>, k_scatter_fin",
        "add_transpose_2e25": "2 x hipMemsetAsync, k_scatter_add<1,1>, k_scatter_fin", "count_lds_2e12": "hipMemsetAsync, k_scatter_count_lds, k_scatter_count_fin",
        "add_lds_2e10": "2 x hipMemsetAsync, k_scatter_add_lds<0,1>, k_scatter_fin", "add_contended_2e24": "2 x hipMemsetAsync, k_scatter_add<0,1>, k_scatter_fin",
    }

    def traffic(name):
        """(bytes read that the result uses, bytes written with every add counted as a store of its accumulator)"""
        lg, nnz, _, _, x, val, src = cases[name]
        n = 1 << lg
        rd = nnz * (4 + (32 if x else 0) + (32 if val else 0) + (4 if src else 0))
        if x is None and val is None:
            return rd + 4 * n, 4 * n + 4 * nnz + 32 * n          # the memset, the adds, the finish
        return rd + 64 * n, 64 * n + 64 * nnz + 32 * n

    def run_op(name):
        lg, nnz, idx, _, x, val, src = cases[name]
        cl = handles[lg]
        cl.vec_scatter(0, idx, x=x, val=val, src=src, nnz=nnz)
        cl.wait_result()
        return cl.last_kernel_ms()

    tables = {lg: piece(d_u, 0, 1 << lg, 32) for lg in (12, 10)}
    tables[logn] = d_u
    halves = {id(d): [piece(d, h * N, N, 4) for h in range(2)] for d in (d_uniform, d_rows)}
    halves[id(d_equal)] = [d_equal]
    val_halves = [piece(d_val, h * N, N, 32) for h in range(2)]

    def run_index(name):
        """vec_index over the same indices, on the 2^logn handle, from a table of the case's n words"""
        lg, nnz, idx, _, _, _, _ = cases[name]
        ms = 0.0
        for h in range(nnz // N):
            big.vec_index(1, tables[lg], halves[id(idx)][h])
            big.wait_result()
            ms += big.last_kernel_ms()
        return ms

    most = max(sum(traffic(k)) // 2 for k in cases)
    d_from, d_to = DeviceBuffer(0, most), DeviceBuffer(0, most)
    hip_ok(hip.hipMemsetAsync(d_from.ptr, 1, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_to.ptr, 2, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def run_copy(nbytes):
        ms = C.c_float()
        hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        hip_ok(hip.hipMemcpyAsync(d_to.ptr, d_from.ptr, nbytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
        hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    # ---- the outputs, checked before anything is timed
    sums = {}
    for name, (lg, nnz, idx, t_idx, x, val, src) in cases.items():
        n, cl = 1 << lg, handles[lg]
        run_op(name)
        if x is None and val is None:
            got = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
            check(lib().blz_ntt_result_device(cl._h, 0, got.data_ptr(), 32 * n))
            want = torch.bincount(t_idx[:nnz] & (n - 1), minlength=n)
            if not torch.equal(got[:, 0], want) or bool(got[:, 1:].any()) or int(got[:, 0].sum()) != nnz:
                raise RuntimeError(f"{name}: the destination is not the histogram of the indices")
            continue
        left = cl.vec_reduce(NTTClient.FOLD_DOT, 0, tables[lg])
        cl.wait_result()
        right = 0
        for h in range(nnz // N):
            big.vec_index(0, tables[lg], halves[id(idx)][h])       # u[idx[k]]
            big.wait_result()
            if x is None:
                operand = val_halves[h]
            else:
                big.vec_index(1, x, halves[id(src)][h], val=val_halves[h])   # val[k] x[src[k]]
                big.wait_result()
                operand = 1
            w = big.vec_reduce(NTTClient.FOLD_DOT, 0, operand)
            big.wait_result()
            right = (right + word(w)) % R_BLS381
            w.free()
        if word(left) != right or right == 0:
            raise RuntimeError(f"{name}: sum u[t] dst[t] = {word(left):x} but sum val[k] x[src k] u[idx k] = {right:x}")
        sums[name] = right
        left.free()
    if len(set(sums.values())) != len(sums):
        raise RuntimeError("two cases gave the same sum: the check would not tell them apart")

    op_ms = {k: [] for k in cases}
    ix_ms = {k: [] for k in cases}
    cp_ms = {k: [] for k in cases}
    for it in range(rounds + 2):          # two warm-up rounds
        for k in cases:
            a, b, c = run_op(k), run_index(k), run_copy(sum(traffic(k)) // 2)
            if it >= 2:
                op_ms[k].append(a)
                ix_ms[k].append(b)
                cp_ms[k].append(c)
    for cl in handles.values():
        cl.close()

    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "checked": True, "cases": {}}
    for k, (lg, nnz, *_rest) in cases.items():
        om, im, cm = (statistics.median(v[k]) for v in (op_ms, ix_ms, cp_ms))
        rd, wr = traffic(k)
        res["cases"][k] = {
            "log_n": lg, "nnz": nnz, "kernels": kernels[k],
            "bytes_read_used": rd, "bytes_written_adds_as_stores": wr, "yardstick_copy_bytes": (rd + wr) // 2,
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "nonzeros_per_us": round(nnz / om / 1e3, 1),
            "vec_index_ms": round(im, 4), "vec_index_ms_min_max": [round(min(ix_ms[k]), 4), round(max(ix_ms[k]), 4)],
            "yardstick_copy_ms": round(cm, 4), "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_vec_index": round(om / im, 4), "ratio_to_copy": round(om / cm, 4),
        }
    c = res["cases"]
    res["contended_over_uniform"] = round(c["add_contended_2e24"]["kernel_ms"] / c["add_val_2e24"]["kernel_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_scatter_ops.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log-size", type=int, default=24)
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
