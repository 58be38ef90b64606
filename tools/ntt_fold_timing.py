#!/usr/bin/env python3
"""What the folds along a resident buffer cost at 2^27 over the BLS12-381 scalar field (blz_ntt_vec_reduce, blz_ntt_vec_scan;
DESIGN.md section 4, "Reductions and scans"): medians of blz_ntt_last_kernel_ms for SUM, DOT, EVAL, SCAN_SUM and SCAN_PROD, each
beside a yardstick that is none of the code under test - a device-to-device hipMemcpyAsync on the handle's stream, timed with HIP
events in the same process, that moves the same number of HBM bytes as the op (a copy of B bytes reads B and writes B):
    SUM, EVAL   read 4 GiB, write 32 bytes                                    ->  a copy of 2 GiB
    DOT         reads 2 x 4 GiB                                               ->  a copy of 4 GiB
    SCAN_*      read the vector twice (k_fold_scan_up, k_fold_scan_down), write it once  ->  a copy of 6 GiB
Ops and copies alternate inside every round; blz_calib_mad_rate is taken right behind the timed rounds, and each op's multiply-adds
per element (from the kernels' code, ntt_fold.hip.hpp) give the issue time they imply at that rate.  The timed outputs are checked
before anything is written: the three reductions against each other and against Python integers through the scans (the last
word of an inclusive scan is the fold; sampled adjacent positions of a scan differ / divide by the input word at that position;
DOT of the vector with the one-word 1 is SUM; EVAL at 1 is SUM; EVAL at z equals DOT with the powers column an exclusive product
scan of z wrote).  Writes profiles/ntt_fold_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_fold_timing.py [--out profiles/ntt_fold_ops.json] [--rounds 9] [--log-size 27] [--timeout 420]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_BLS381 = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PRODUCT = 128          # v_mad_u64_u32 of one 8 x 32-bit Montgomery product (fp_mul: 64 for a b, 64 for q m)
CANON = 4              # vec_canon of one word in this field (the quotient estimate is at most 2: four limbs' products survive)


def multiply_adds():
    """Per element, from the code.  `lane`: the arithmetic's own count; `issued`: what the SIMDs issue - a tree level with fewer
    nodes than lanes still occupies whole waves (a 256-leaf tree: 9 wave-products of 64 lanes each, per 1024 elements).  The
    reductions' trees, the powers of z and the scans of the tiles' totals are below 0.01 products per element and left out."""
    tile = 1024
    up = (4 + 3) / 4                      # to Montgomery form, the lane's 3 combines
    down = (4 + 3 + 8 + 1 + 1 + 4) / 4    # the same, 8 Kogge-Stone steps, carry x lanes below, its way back, carry x element
    return {
        "SUM": {"lane": CANON, "issued": CANON},
        "DOT": {"lane": PRODUCT + CANON, "issued": PRODUCT + CANON},
        "EVAL": {"lane": PRODUCT + CANON, "issued": PRODUCT + CANON},
        "SCAN_SUM": {"lane": 2 * CANON, "issued": 2 * CANON},
        "SCAN_PROD": {"lane": round((up + down + 255 / tile) * PRODUCT, 2), "issued": round((up + down + 9 * 64 / tile) * PRODUCT, 2),
                      "products_per_element": {"k_fold_scan_up": round(up + 255 / tile, 3), "k_fold_scan_down": down}},
    }


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

    n = 1 << logn
    nbytes = 32 * n
    r = R_BLS381
    cl = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
    stream, dev = C.c_void_p(), C.c_int()
    check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    # buffer 0: the vector under the ops (synthetic non-zero field elements); d_y: DOT's second vector
    d_y = DeviceBuffer(0, nbytes)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_y.ptr, n, 7))
    check(lib().blz_ntt_set_data_device(cl._h, 0, d_y.ptr, nbytes))
    check(blaze_amd.aux().blz_synth_field_elements(0, d_y.ptr, n, 8))
    z = random.Random(27).randrange(2, r)
    d_z, d_one = cl.scalar(z), cl.scalar(1)
    out, total = DeviceBuffer(0, 32), DeviceBuffer(0, 32)

    copy_bytes = {"SUM": nbytes // 2, "DOT": nbytes, "EVAL": nbytes // 2, "SCAN_SUM": 6 * nbytes // 4, "SCAN_PROD": 6 * nbytes // 4}
    d_src, d_dst = DeviceBuffer(0, max(copy_bytes.values())), DeviceBuffer(0, max(copy_bytes.values()))
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, d_src.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, d_dst.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def word(d):
        return int.from_bytes(bytes(d.download(32)), "little")

    def run_op(name, b=None):
        if name == "SUM":
            cl.vec_reduce(NTTClient.FOLD_SUM, 0, None, out)
        elif name == "DOT":
            cl.vec_reduce(NTTClient.FOLD_DOT, 0, d_y if b is None else b, out)
        elif name == "EVAL":
            cl.vec_reduce(NTTClient.FOLD_EVAL, 0, d_z if b is None else b, out)
        elif name == "SCAN_SUM":
            cl.vec_scan(NTTClient.SCAN_SUM, 1, 0, total=total)
        else:
            cl.vec_scan(NTTClient.SCAN_PROD, 1, 0, total=total)
        cl.wait_result()
        return cl.last_kernel_ms()

    def run_copy(size):
        ms = C.c_float()
        hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        hip_ok(hip.hipMemcpyAsync(d_dst.ptr, d_src.ptr, size, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
        hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    names = ("SUM", "DOT", "EVAL", "SCAN_SUM", "SCAN_PROD")
    op_ms = {k: [] for k in names}
    cp_ms = {k: [] for k in names}
    for it in range(rounds + 2):          # two warm-up rounds
        for k in names:
            a, b = run_op(k), run_copy(copy_bytes[k])
            if it >= 2:
                op_ms[k].append(a)
                cp_ms[k].append(b)
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))

    # ---- the timed outputs, checked
    t_a = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    t_s = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    check(lib().blz_ntt_result_device(cl._h, 0, t_a.data_ptr(), nbytes))

    def rows(t, idx):
        v = t[torch.tensor(idx, device="cuda:0")].cpu().tolist()
        return [sum((w & 0xFFFFFFFFFFFFFFFF) << (64 * k) for k, w in enumerate(row)) for row in v]

    rng = random.Random(1)
    sample = sorted(set([1, 2, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, n // 2, n - 1] + [rng.randrange(1, n) for _ in range(4096)]))
    sample = [p for p in sample if 0 < p < n]
    prev = [p - 1 for p in sample]
    va = rows(t_a, sample)
    run_op("SUM")
    s_sum = word(out)
    run_op("SCAN_SUM")
    check(lib().blz_ntt_result_device(cl._h, 1, t_s.data_ptr(), nbytes))
    hi, lo = rows(t_s, sample), rows(t_s, prev)
    if any((q + x) % r != p for p, q, x in zip(hi, lo, va)) or rows(t_s, [0]) != rows(t_a, [0]):
        raise RuntimeError("SCAN_SUM: adjacent sampled positions do not differ by the input word")
    if rows(t_s, [n - 1])[0] != s_sum or word(total) != s_sum:
        raise RuntimeError("SUM, the last word of SCAN_SUM and its d_total disagree")
    run_op("SCAN_PROD")
    check(lib().blz_ntt_result_device(cl._h, 1, t_s.data_ptr(), nbytes))
    hi, lo = rows(t_s, sample), rows(t_s, prev)
    if any(q * x % r != p or p == 0 for p, q, x in zip(hi, lo, va)) or rows(t_s, [0]) != rows(t_a, [0]):
        raise RuntimeError("SCAN_PROD: adjacent sampled positions do not differ by the factor of the input word")
    if rows(t_s, [n - 1])[0] != word(total):
        raise RuntimeError("the last word of SCAN_PROD and its d_total disagree")
    run_op("DOT", d_one)
    if word(out) != s_sum:
        raise RuntimeError("DOT with the one-word 1 is not SUM")
    run_op("EVAL", d_one)
    if word(out) != s_sum:
        raise RuntimeError("EVAL at 1 is not SUM")
    run_op("EVAL")
    s_eval = word(out)
    cl.vec_scan(NTTClient.SCAN_PROD, 1, d_z, exclusive=True)      # buffer 1 = the powers of z
    cl.wait_result()
    check(lib().blz_ntt_result_device(cl._h, 1, t_s.data_ptr(), nbytes))
    if rows(t_s, sample[:512]) != [pow(z, p, r) for p in sample[:512]]:
        raise RuntimeError("the exclusive product scan of z is not its powers on the sampled positions")
    cl.vec_reduce(NTTClient.FOLD_DOT, 0, 1, out)
    cl.wait_result()
    if word(out) != s_eval:
        raise RuntimeError("EVAL at z differs from DOT with the powers of z")
    cl.close()

    mads = multiply_adds()
    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "tile": 1024,
           "calib_mad_rate": cal[0], "calib_clock_mhz": cal[2], "checked": True, "ops": {}}
    for k in names:
        om, cm = statistics.median(op_ms[k]), statistics.median(cp_ms[k])
        hbm = 2 * copy_bytes[k]
        res["ops"][k] = {
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "hbm_bytes": hbm, "achieved_tb_per_s": round(hbm / om / 1e9, 3),
            "yardstick_copy_bytes": copy_bytes[k], "yardstick_copy_ms": round(cm, 4),
            "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_copy": round(om / cm, 4),
            "multiply_adds_per_element": mads[k],
            "issue_ms_implied": round(mads[k]["issued"] * n / cal[0] * 1e3, 4),
        }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_fold_ops.json"))
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
