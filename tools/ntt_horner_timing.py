#!/usr/bin/env python3
"""What the weighted scan along a resident buffer costs at 2^27 over the BLS12-381 scalar field (blz_ntt_vec_horner; DESIGN.md
section 4, "Weighted scans"): medians of blz_ntt_last_kernel_ms for the four flag combinations, each beside two yardsticks taken
in the same process, alternating with it inside every round:
    a device-to-device hipMemcpyAsync on the handle's stream, HIP-event timed, that moves the op's HBM traffic - the vector read
    twice (k_horner_up, k_horner_down) and written once, 12 GiB, is a copy of 6 GiB (a copy of B bytes reads B and writes B);
    SCAN_PROD (blz_ntt_vec_scan) on the same handle and the same vector - the scan with the same traffic and 7.25 products per
    element, which the weighted scan's 4.75 are meant to undercut.
blz_calib_mad_rate is taken right behind the timed rounds, and the op's multiply-adds per element (from the kernels' code,
ntt_horner.hip.hpp) give the issue time they imply at that rate.

The outputs are checked on the device before anything is written, by code other than the op's own: with a in buffer 0 and the
division's quotient q in buffer 1, BLZ_FOLD_EVAL evaluates both at two random points w: a(w) - a(z) = q(w) (w - z), and d_total
is what EVAL writes for a at z.  The forward exclusive scan is the same division of the polynomial stored top coefficient
first, e(w) (1 - w z) = w a(w) - w^n a_rev(z).  The inclusive scans are tied to the exclusive ones on sampled positions,
inc[p] = a[p] + z exc[p].  2^27 is the only size that reaches the powers above z^(2^21).
Writes profiles/ntt_horner_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_horner_timing.py [--out profiles/ntt_horner_ops.json] [--rounds 9] [--log-size 27] [--timeout 420]
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
MODES = {"inclusive": (False, False), "exclusive": (True, False), "reverse": (False, True), "reverse_exclusive": (True, True)}


def multiply_adds():
    """Per element, from the code.  `lane`: the arithmetic's own count; `issued`: what the SIMDs issue - a tree level with fewer
    nodes than lanes still occupies whole waves (a 256-leaf tree: 9 wave-products of 64 lanes each, per 1024 elements), and the
    carry's product, lane 0's alone, occupies its wave.  k_horner_pow and the scans of the tiles' totals are below 0.01 products
    per element and left out."""
    tile = 1024
    up = 3 / 4                      # the lane's Horner value
    down = (3 + 8 + 4) / 4          # the same, 8 Kogge-Stone steps, the recurrence again from the value before the lane
    horner = {"lane": round((up + 255 / tile + down + 1 / tile) * PRODUCT + 2 * CANON, 2),
              "issued": round((up + 9 * 64 / tile + down + 64 / tile) * PRODUCT + 2 * CANON, 2),
              "products_per_element": {"k_horner_up": round(up + 255 / tile, 3), "k_horner_down": round(down + 1 / tile, 3)}}
    s_up, s_down = (4 + 3) / 4, (4 + 3 + 8 + 1 + 1 + 4) / 4      # tools/ntt_fold_timing.py
    scan_prod = {"lane": round((s_up + s_down + 255 / tile) * PRODUCT, 2), "issued": round((s_up + s_down + 9 * 64 / tile) * PRODUCT, 2)}
    return horner, scan_prod


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

    # buffer 0: the vector under the ops (synthetic non-zero field elements), staged through the copy's source
    copy_bytes = 6 * nbytes // 4
    d_src, d_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_src.ptr, n, 7))
    check(lib().blz_ntt_set_data_device(cl._h, 0, d_src.ptr, nbytes))
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, d_src.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, d_dst.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    rng = random.Random(27)
    z = rng.randrange(2, r)
    d_z = cl.scalar(z)
    out, total = DeviceBuffer(0, 32), DeviceBuffer(0, 32)

    def word(d):
        return int.from_bytes(bytes(d.download(32)), "little")

    def run_op(name):
        if name == "SCAN_PROD":
            cl.vec_scan(NTTClient.SCAN_PROD, 1, 0, total=total)
        else:
            exclusive, reverse = MODES[name]
            cl.vec_horner(1, 0, d_z, exclusive=exclusive, reverse=reverse, total=total)
        cl.wait_result()
        return cl.last_kernel_ms()

    def run_copy():
        ms = C.c_float()
        hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        hip_ok(hip.hipMemcpyAsync(d_dst.ptr, d_src.ptr, copy_bytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
        hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    names = tuple(MODES)
    op_ms = {k: [] for k in names}
    cp_ms = {k: [] for k in names}
    sp_ms = {k: [] for k in names}
    for it in range(rounds + 2):          # two warm-up rounds
        for k in names:
            a, b, c = run_op(k), run_copy(), run_op("SCAN_PROD")
            if it >= 2:
                op_ms[k].append(a)
                cp_ms[k].append(b)
                sp_ms[k].append(c)
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    d_src.free()
    d_dst.free()

    # ---- the outputs, checked
    def evaluate(buf, point):
        dp = cl.scalar(point)
        cl.vec_reduce(NTTClient.FOLD_EVAL, buf, dp, out)
        cl.wait_result()
        dp.free()
        return word(out)

    a_z = evaluate(0, z)
    points = [rng.randrange(2, r) for _ in range(2)]
    a_w = [evaluate(0, w) for w in points]
    run_op("reverse_exclusive")
    if word(total) != a_z:
        raise RuntimeError("the division's d_total is not EVAL of a at z")
    for w, aw in zip(points, a_w):
        if (aw - a_z - evaluate(1, w) * (w - z)) % r != 0:
            raise RuntimeError("a(w) - a(z) != q(w) (w - z)")
    t_a = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    t_e = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    t_i = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    check(lib().blz_ntt_result_device(cl._h, 0, t_a.data_ptr(), nbytes))
    check(lib().blz_ntt_result_device(cl._h, 1, t_e.data_ptr(), nbytes))

    def rows(t, idx):
        v = t[torch.tensor(idx, device="cuda:0")].cpu().tolist()
        return [sum((w & 0xFFFFFFFFFFFFFFFF) << (64 * k) for k, w in enumerate(row)) for row in v]

    srng = random.Random(1)
    sample = sorted(set([0, 1, 2, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 21) - 1, 1 << 21, n // 2, n - 2, n - 1]
                        + [srng.randrange(n) for _ in range(4096)]))
    sample = [p for p in sample if 0 <= p < n]
    va = rows(t_a, sample)
    if rows(t_e, [n - 1]) != [0]:
        raise RuntimeError("the quotient's top coefficient is not 0")
    run_op("reverse")
    check(lib().blz_ntt_result_device(cl._h, 1, t_i.data_ptr(), nbytes))
    if any((x + z * e) % r != i for i, e, x in zip(rows(t_i, sample), rows(t_e, sample), va)):
        raise RuntimeError("reverse: inclusive != a + z exclusive on the sampled positions")
    if word(total) != a_z or rows(t_i, [0])[0] != a_z:
        raise RuntimeError("reverse: d_total or the word at position 0 is not a(z)")
    # forward: e(w) = sum_p e[p] w^p satisfies e(w) (1 - w z) = w a(w) - w^n a_rev(z), a_rev(z) = the forward total
    run_op("exclusive")
    fwd_total = word(total)
    check(lib().blz_ntt_result_device(cl._h, 1, t_e.data_ptr(), nbytes))
    for w, aw in zip(points, a_w):
        if (evaluate(1, w) * (1 - w * z) - (w * aw - pow(w, n, r) * fwd_total)) % r != 0:
            raise RuntimeError("forward exclusive: e(w) (1 - w z) != w a(w) - w^n total")
    if rows(t_e, [0]) != [0]:
        raise RuntimeError("forward exclusive: position 0 is not 0")
    run_op("inclusive")
    check(lib().blz_ntt_result_device(cl._h, 1, t_i.data_ptr(), nbytes))
    if any((x + z * e) % r != i for i, e, x in zip(rows(t_i, sample), rows(t_e, sample), va)):
        raise RuntimeError("forward: inclusive != a + z exclusive on the sampled positions")
    if word(total) != fwd_total or rows(t_i, [n - 1])[0] != fwd_total:
        raise RuntimeError("forward: d_total or the last word is not the exclusive run's total")
    cl.close()

    horner, scan_prod = multiply_adds()
    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "tile": 1024,
           "calib_mad_rate": cal[0], "calib_clock_mhz": cal[2], "checked": True,
           "hbm_bytes": 2 * copy_bytes, "yardstick_copy_bytes": copy_bytes,
           "multiply_adds_per_element": {"horner": horner, "SCAN_PROD": scan_prod},
           "issue_ms_implied": {"horner": round(horner["issued"] * n / cal[0] * 1e3, 4),
                                "SCAN_PROD": round(scan_prod["issued"] * n / cal[0] * 1e3, 4)},
           "ops": {}}
    for k in names:
        om, cm, sm = statistics.median(op_ms[k]), statistics.median(cp_ms[k]), statistics.median(sp_ms[k])
        res["ops"][k] = {
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "achieved_tb_per_s": round(2 * copy_bytes / om / 1e9, 3),
            "yardstick_copy_ms": round(cm, 4), "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_copy": round(om / cm, 4),
            "scan_prod_ms": round(sm, 4), "scan_prod_ms_min_max": [round(min(sp_ms[k]), 4), round(max(sp_ms[k]), 4)],
            "ratio_to_scan_prod": round(om / sm, 4),
        }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_horner_ops.json"))
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
