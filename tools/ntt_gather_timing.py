#!/usr/bin/env python3
"""What a gather on resident buffers costs over the BLS12-381 scalar field (blz_ntt_vec_gather; DESIGN.md section 4,
"Gathers"): medians of blz_ntt_last_kernel_ms, each case beside ONE yardstick taken in the same process, alternating with it
inside every round - a device-to-device hipMemcpyAsync on the handle's stream, HIP-event timed, of the bytes that case moves (a
copy of B bytes reads B and writes B).
    on the 2^27 handle (n = 2^27, 4 GiB per vector), from buffer 0 into buffer 1:
        identity, rotate by 1, rotate by n / 2   k_gather_contig; reads 4 GiB, writes 4 GiB: a copy of 4 GiB
        reversal                                 k_gather_strided, descending addresses; the same bytes
        in-place rotate by 1                     k_gather_contig into the scratch, then the copy back: a copy of 8 GiB
        extension from 2^25 device words         reads 1 GiB, writes 4 GiB (3 GiB of zeros): a copy of 2.5 GiB
    on a 2^25 handle, from 2^27 device words:
        slice (offset n + 1)                     reads 1 GiB, writes 1 GiB: a copy of 1 GiB
        decimation (stride 4, offset 3)          USES 1 GiB of the 4 GiB it touches, writes 1 GiB: beside a copy of 1 GiB, and
                                                 beside one of 2.5 GiB - what it moves if every touched line is fetched whole
The outputs are checked on the device before anything is written, by code other than the op's own: the source words are
canonical, so every case's destination must equal torch's index_select of the source at (offset + stride p) & (count - 1),
with zeros from len up - all n positions, compared as 4 x int64.
Writes profiles/ntt_gather_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_gather_timing.py [--out profiles/ntt_gather_ops.json] [--rounds 9] [--log-size 27] [--timeout 420]
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

CHECK_ROWS = 1 << 20   # positions per piece of the output check


def cases(logn: int):
    """name -> (handle, source, offset, stride, len, dst): handle "big" (2^logn) or "small" (2^(logn - 2)); source a transform
    buffer (an int) or "quarter" / "words" (2^(logn - 2) / 2^logn device words)"""
    n, m = 1 << logn, 1 << (logn - 2)
    return {
        "identity": ("big", 0, 0, 1, n, 1),
        "rotate_1": ("big", 0, 1, 1, n, 1),
        "rotate_half": ("big", 0, n // 2, 1, n, 1),
        "reversal": ("big", 0, n - 1, n - 1, n, 1),
        "rotate_1_in_place": ("big", 1, 1, 1, n, 1),
        "extend_from_quarter": ("big", "quarter", 0, 1, m, 1),
        "slice_of_4n": ("small", "words", m + 1, 1, m, 1),
        "decimate_4n_stride_4": ("small", "words", 3, 4, m, 1),
    }


def traffic(logn: int, name: str):
    """(bytes read that the result uses, bytes written, bytes of the yardstick copy) from the shapes"""
    big, quarter = 32 << logn, 32 << (logn - 2)
    if name == "rotate_1_in_place":
        return 2 * big, 2 * big, 2 * big
    if name == "extend_from_quarter":
        return quarter, big, (quarter + big) // 2
    if name in ("slice_of_4n", "decimate_4n_stride_4"):
        return quarter, quarter, quarter
    return big, big, big


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

    n, m = 1 << logn, 1 << (logn - 2)
    dc = DriverClient(0)
    handles = {"big": NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE),
               "small": NTTClient(NTT.Ntt, dc, log_size=logn - 2, flags=NTTClient.NO_FACTOR_TABLE)}
    stream, dev = C.c_void_p(), C.c_int()
    check(lib().blz_ntt_stream(handles["big"]._h, C.byref(stream), C.byref(dev)))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    # the source: 2^logn canonical field elements as device words, their first quarter again as a buffer of its own, and the
    # same words in both transform buffers of the big handle
    words, quarter = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * m)
    check(blaze_amd.aux().blz_synth_field_elements(0, words.ptr, n, 11))
    hip_ok(hip.hipMemcpyAsync(quarter.ptr, words.ptr, quarter.nbytes, 3, stream), "hipMemcpyAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    for buf in (0, 1):
        check(lib().blz_ntt_set_data_device(handles["big"]._h, buf, words.ptr, words.nbytes))
    sources = {"words": words, "quarter": quarter}
    table = cases(logn)
    most = max(traffic(logn, k)[2] for k in table)
    d_src, d_dst = DeviceBuffer(0, most), DeviceBuffer(0, most)
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def run_op(name):
        handle, src, off, s, ln, dst = table[name]
        cl = handles[handle]
        cl.vec_gather(dst, sources.get(src, src), offset=off, stride=s, length=ln)
        cl.wait_result()
        return cl.last_kernel_ms()

    def run_copy(nbytes):
        ms = C.c_float()
        hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        hip_ok(hip.hipMemcpyAsync(d_dst.ptr, d_src.ptr, nbytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
        hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    touched = (32 * n + 32 * m) // 2   # the decimation, if every line it touches is fetched whole: reads 4 x, writes 1 x
    op_ms = {k: [] for k in table}
    cp_ms = {k: [] for k in table}
    touched_ms = []
    for it in range(rounds + 2):          # two warm-up rounds
        for k in table:
            a, b = run_op(k), run_copy(traffic(logn, k)[2])
            c = run_copy(touched) if k == "decimate_4n_stride_4" else None
            if it >= 2:
                op_ms[k].append(a)
                cp_ms[k].append(b)
                if c is not None:
                    touched_ms.append(c)
    d_src.free()
    d_dst.free()

    # ---- the outputs, checked: every position of every case against torch's gather of the source
    t_words = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    hip_ok(hip.hipMemcpyAsync(t_words.data_ptr(), words.ptr, words.nbytes, 3, stream), "hipMemcpyAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    if not bool((t_words != 0).any(dim=1).all()):
        raise RuntimeError("the synthetic source holds zero words: the check of the zeroed tail would prove nothing")
    for k, (handle, src, off, s, ln, dst) in table.items():
        cl = handles[handle]
        if not isinstance(src, str):   # the in-place case rotated its buffer once per round: put the words back
            check(lib().blz_ntt_set_data_device(cl._h, src, words.ptr, words.nbytes))
        count = m if src == "quarter" else n
        size = 1 << cl.log_size
        run_op(k)
        got = torch.empty((size, 4), dtype=torch.int64, device="cuda:0")
        check(lib().blz_ntt_result_device(cl._h, dst, got.data_ptr(), 32 * size))
        for p0 in range(0, size, CHECK_ROWS):   # in pieces: torch refuses the launch of one index_select over 2^27 rows
            p1 = min(p0 + CHECK_ROWS, size)
            reads = max(p0, min(ln, p1))     # positions p0 .. reads - 1 read the source, reads .. p1 - 1 are zero
            ok = True
            if reads > p0:
                idx = (off + s * torch.arange(p0, reads, dtype=torch.int64, device="cuda:0")) & (count - 1)
                ok = torch.equal(got[p0:reads], t_words.index_select(0, idx))
            if p1 > reads:
                ok = ok and not bool((got[reads:p1] != 0).any())
            if not ok:
                raise RuntimeError(f"{k}: the destination is not the gather of the source in positions {p0} .. {p1 - 1}")
        del got
    for cl in handles.values():
        cl.close()

    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "checked": True, "cases": {}}
    for k, (handle, src, off, s, ln, dst) in table.items():
        om, cm = statistics.median(op_ms[k]), statistics.median(cp_ms[k])
        rd, wr, cp = traffic(logn, k)
        res["cases"][k] = {
            "handle_log_size": logn if handle == "big" else logn - 2,
            "source": f"transform buffer {src}" if not isinstance(src, str) else f"{m if src == 'quarter' else n} device words",
            "offset": off, "stride": s, "len": ln,
            "kernel": "k_gather_contig" if s == 1 else "k_gather_strided",
            "bytes_read_used": rd, "bytes_written": wr, "yardstick_copy_bytes": cp,
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "achieved_tb_per_s": round((rd + wr) / om / 1e9, 3),
            "yardstick_copy_ms": round(cm, 4), "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_copy": round(om / cm, 4),
        }
    tm = statistics.median(touched_ms)
    res["cases"]["decimate_4n_stride_4"].update({
        "bytes_touched": 32 * n, "touched_copy_bytes": touched, "touched_copy_ms": round(tm, 4),
        "ratio_to_touched_copy": round(statistics.median(op_ms["decimate_4n_stride_4"]) / tm, 4)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_gather_ops.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log-size", type=int, default=27)
    ap.add_argument("--timeout", type=int, default=420)
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
