#!/usr/bin/env python3
"""What the element-wise ops cost at 2^27 over the BLS12-381 scalar field (blz_ntt_vec_op; DESIGN.md section 4, "Element-wise
ops"): medians of blz_ntt_last_kernel_ms for MUL, MULSUB and INV, each beside a yardstick that is none of the code under
test - a device-to-device hipMemcpyAsync on the handle's stream, timed with HIP events in the same process, that moves the same
number of HBM bytes as the op (a copy of B bytes reads B and writes B):
    MUL     reads 2 x 4 GiB, writes 4 GiB  ->  a copy of 6 GiB
    MULSUB  reads 3 x 4 GiB, writes 4 GiB  ->  a copy of 8 GiB
    INV     reads the vector twice (k_vec_inv_up, k_vec_inv_down), writes it once  ->  a copy of 6 GiB
Ops and copies alternate inside every round; blz_calib_mad_rate is taken right behind the timed rounds, and each op's multiply-adds
per element (from the kernels' code, ntt_vec.hip.hpp) give the issue time they imply at that rate.  The timed outputs are checked
on the device before anything is written: MUL and MULSUB on sampled positions against Python integers, INV on ALL positions -
MUL of its output with its input is 1 where the input is non-zero and 0 elsewhere.  Writes profiles/ntt_vec_ops.json.  The device
work runs in ONE child process under its own time limit.

    python tools/ntt_vec_timing.py [--out profiles/ntt_vec_ops.json] [--rounds 9] [--log-size 27] [--timeout 420]
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
    nodes than lanes still occupies whole waves (a 256-leaf tree: 9 wave-products up, 12 down, of 64 lanes each, per 1024 elements)."""
    tile, lanes = 1024, 256
    fermat = 255 + bin(R_BLS381 - 2).count("1") - 1          # squarings and products of x^(r - 2), top bit first
    mid = (7 + 14 + 2 + fermat) * PRODUCT / (8 * tile)         # eight tile totals to a lane
    up_lane = 3 * PRODUCT / 4 + 4 * CANON / 4
    down_lane = (3 + 6) * PRODUCT / 4 + 4 * CANON / 4
    return {
        "MUL": {"lane": 2 * PRODUCT, "issued": 2 * PRODUCT},
        "MULSUB": {"lane": 2 * PRODUCT + CANON, "issued": 2 * PRODUCT + CANON},
        "INV": {"lane": round(up_lane + down_lane + (255 + 255 + 510) * PRODUCT / tile + mid, 2),
                "issued": round(up_lane + down_lane + (9 + 9 + 12) * 64 * PRODUCT / tile + mid, 2),
                "products_per_element": {"lanes": 3.0, "trees": round((255 + 255 + 510) / tile, 3), "totals": round(mid / PRODUCT, 4)}},
    }


def child(rounds: int, logn: int) -> dict:
    import torch

    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import check, lib
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_ntt import NTT, NTTClient, NTTInput

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
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

    d_x, d_y = DeviceBuffer(0, nbytes), DeviceBuffer(0, nbytes)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_x.ptr, n, 7))
    check(blaze_amd.aux().blz_synth_field_elements(0, d_y.ptr, n, 8))
    # the vector under the ops: synthetic elements with zeros planted (alone, adjacent, tile edges, one whole tile)
    t_a = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    t_out = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    check(lib().blz_ntt_set_data_device(cl._h, 0, d_x.ptr, nbytes))
    check(lib().blz_ntt_result_device(cl._h, 0, t_a.data_ptr(), nbytes))
    zeros = [0, 1, 1023, 1024, n // 2, n - 1] + list(range(4096, 5120))
    t_a[torch.tensor([p for p in zeros if p < n], device="cuda:0")] = 0
    torch.cuda.synchronize()
    check(lib().blz_ntt_set_data_device(cl._h, 0, t_a.data_ptr(), nbytes))

    copy_bytes = {"MUL": 6 * nbytes // 4, "MULSUB": 8 * nbytes // 4, "INV": 6 * nbytes // 4}
    d_src, d_dst = DeviceBuffer(0, max(copy_bytes.values())), DeviceBuffer(0, max(copy_bytes.values()))
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, d_src.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, d_dst.nbytes, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def run_op(name):
        if name == "MUL":
            cl.vec_op(NTTClient.MUL, 1, 0, d_x)
        elif name == "MULSUB":
            cl.vec_op(NTTClient.MULSUB, 1, 0, d_x, d_y)
        else:
            cl.vec_op(NTTClient.INV, 1, 0)
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

    def rows(t, idx):
        v = t[torch.tensor(idx, device="cuda:0")].cpu().tolist()
        return [sum((w & 0xFFFFFFFFFFFFFFFF) << (64 * k) for k, w in enumerate(row)) for row in v]

    names = ("MUL", "MULSUB", "INV")
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
    rng = random.Random(1)
    sample = sorted(set([0, 1, 1023, 1024, 4096, 5119, n // 2, n - 1] + [rng.randrange(n) for _ in range(4096)]))
    t_x, t_y = torch.empty_like(t_a), None
    hip_ok(hip.hipMemcpy(t_x.data_ptr(), d_x.ptr, nbytes, 3), "hipMemcpy")
    va, vx = rows(t_a, sample), rows(t_x, sample)
    del t_x
    run_op("MUL")
    check(lib().blz_ntt_result_device(cl._h, 1, t_out.data_ptr(), nbytes))
    if rows(t_out, sample) != [p * q % r for p, q in zip(va, vx)]:
        raise RuntimeError("MUL differs from Python integers on the sampled positions")
    t_y = torch.empty_like(t_a)
    hip_ok(hip.hipMemcpy(t_y.data_ptr(), d_y.ptr, nbytes, 3), "hipMemcpy")
    vy = rows(t_y, sample)
    del t_y
    run_op("MULSUB")
    check(lib().blz_ntt_result_device(cl._h, 1, t_out.data_ptr(), nbytes))
    if rows(t_out, sample) != [(p * q - s) % r for p, q, s in zip(va, vx, vy)]:
        raise RuntimeError("MULSUB differs from Python integers on the sampled positions")
    run_op("INV")
    cl.vec_op(NTTClient.MUL, 1, 1, 0)
    cl.wait_result()
    check(lib().blz_ntt_result_device(cl._h, 1, t_out.data_ptr(), nbytes))
    nonzero = (t_a != 0).any(dim=1)
    good = (t_out[:, 0] == nonzero.to(torch.int64)) & (t_out[:, 1:] == 0).all(dim=1)
    planted = int((~nonzero).sum().item())
    if not bool(good.all().item()) or planted < 1024:
        raise RuntimeError(f"INV: x * x^-1 is not 1 (0 where x = 0) on {int((~good).sum().item())} positions; {planted} zeros")
    cl.close()

    mads = multiply_adds()
    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "tile": 1024,
           "calib_mad_rate": cal[0], "calib_clock_mhz": cal[2], "zeros_planted": planted, "checked": True, "ops": {}}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_vec_ops.json"))
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
