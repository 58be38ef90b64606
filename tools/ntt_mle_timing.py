#!/usr/bin/env python3
"""What the multilinear ops on resident buffers cost over the BLS12-381 scalar field (blz_ntt_vec_mle_fold / _round / _eq;
DESIGN.md section 4, "Multilinear tables"): medians of blz_ntt_last_kernel_ms, each case beside ONE yardstick taken in the same
process, alternating with it inside every round - a device-to-device hipMemcpyAsync on the handle's stream, HIP-event timed, of
the bytes that case moves (a copy of B bytes reads B and writes B) - and blz_calib_mad_rate right behind the timed rounds.
    on the 2^L handle (L = 27: n = 2^27, 4 GiB per table), len = n:
        fold, default and BLZ_MLE_LOW, buffer 0 -> buffer 1    reads 4 GiB, writes 2 GiB: a copy of 3 GiB
        fold in place, default                                 the same bytes
        fold in place, BLZ_MLE_LOW                             through the scratch and 2 GiB copied back: a copy of 5 GiB
        round k = 1, 2, 3 at points = k + 1                    reads k x 4 GiB: a copy of k x 2 GiB
        eq, m = L, into buffer 1                               writes 4 GiB: a copy of 2 GiB
    on a 2^(L - 3) handle: a whole sumcheck of L - 3 variables for sum eq (Az Bz - Cz) = 0 as tests/test_gpu_ntt_mle.py runs it
        (per round two round polynomials, four folds in place, the challenge uploaded as a device word; the tables are synthetic
        with Cz = Az o Bz, no sparse product is timed): the sum of the ops' device times and the wall time of the loop.
The outputs are checked on the device before anything is written, by code other than the op's own: a fold through DOT with a
random vector (sum w dst = sum w lo + r (sum w hi - sum w lo), the halves of the pairs taken by views or by vec_gather); a round
polynomial at every point t through the existing MUL / DOT / SUM over the tables folded at r = t, and out[0] + out[1] against the
reduction of the unfolded tables; the equality table through SUM = 1 and 256 sampled words against the product formula; every
round of the sumcheck through s(0) + s(1) = claim and its end through claim = eq (Az Bz - Cz).
Writes profiles/ntt_mle_ops.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_mle_timing.py [--out profiles/ntt_mle_ops.json] [--rounds 9] [--log-size 27] [--timeout 540]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001   # BLS12-381 Fr
MADS_PER_PRODUCT = 128   # v_mad_u64_u32 of one 8-limb Montgomery product (field.hip.hpp)


def case_table(logn: int):
    """name -> (kind, low, traffic in words read + written, Montgomery products per pair or word, from ntt_mle.hip.hpp)"""
    n = 1 << logn
    return {
        "fold": ("fold", False, n + n // 2, 1),
        "fold_low": ("fold", True, n + n // 2, 1),
        "fold_in_place": ("fold_ip", False, n + n // 2, 1),
        "fold_low_in_place": ("fold_ip", True, n + n // 2 + n, 1),
        "round_k1": ("round", 1, n, 0),
        "round_k2": ("round", 2, 2 * n, 3),
        "round_k3": ("round", 3, 3 * n, 8),
        # one product by the outer word, and the block's table (1023 doublings + 10 conversions of tau) shared by its tiles
        "eq": ("eq", None, n, round(1 + 1033 / 1024 / max(1, (n >> 10) // 2048), 4)),
    }


def interpolate(s, x):
    acc = 0
    for i, si in enumerate(s):
        num = den = 1
        for j in range(len(s)):
            if j != i:
                num = num * (x - j) % R
                den = den * (i - j) % R
        acc += si * num * pow(den, -1, R)
    return acc % R


def child(rounds: int, logn: int) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import BlzVecArg, check, lib
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

    n, half = 1 << logn, 1 << (logn - 1)
    dc = DriverClient(0)
    cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
    stream, dev = C.c_void_p(), C.c_int()
    check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
    rng = random.Random(27)

    # three tables of canonical field elements: a and b in the buffers (and as device words, to put them back), c as device words
    a, b, c = (DeviceBuffer(0, 32 * n) for _ in range(3))
    for i, d in enumerate((a, b, c)):
        check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 31 + i))

    def restore():
        check(lib().blz_ntt_set_data_device(cl._h, 0, a.ptr, a.nbytes))
        check(lib().blz_ntt_set_data_device(cl._h, 1, b.ptr, b.nbytes))

    restore()
    rr = rng.getrandbits(256)
    d_r = cl.scalar(rr)
    tau = [rng.getrandbits(256) for _ in range(logn)]
    point = DeviceBuffer(0, 32 * logn)
    point.upload(b"".join(t.to_bytes(32, "little") for t in tau))
    table = case_table(logn)
    most = max(v[2] for v in table.values()) * 32 // 2
    d_src, d_dst = DeviceBuffer(0, most), DeviceBuffer(0, most)
    hip_ok(hip.hipMemsetAsync(d_src.ptr, 1, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipMemsetAsync(d_dst.ptr, 2, most, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    outs = {}

    def run_op(name):
        kind, arg, _, _ = table[name]
        if kind == "fold":
            cl.vec_mle_fold(1, 0, d_r, low=arg)
        elif kind == "fold_ip":
            cl.vec_mle_fold(0, 0, d_r, low=arg)
        elif kind == "round":
            outs[name] = cl.vec_mle_round(*((0, 1, c)[:arg] + (None,) * (3 - arg)), out=outs.get(name))
        else:
            cl.vec_mle_eq(1, point)
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

    op_ms = {k: [] for k in table}
    cp_ms = {k: [] for k in table}
    for it in range(rounds + 2):          # two warm-up rounds
        for k in table:
            x, y = run_op(k), run_copy(table[k][2] * 32 // 2)
            if it >= 2:
                op_ms[k].append(x)
                cp_ms[k].append(y)
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    d_src.free()
    d_dst.free()

    # ---- the outputs, checked
    def word(d):
        return int.from_bytes(bytes(d.download(32)), "little")

    def view(d, count, first=0):
        return BlzVecArg(d.ptr + 32 * first, 0, 0, count)

    def reduce(op, x, y=None):
        """the reduction over the n positions as an integer; x, y: a buffer index or a BlzVecArg"""
        vx, vy = (v if isinstance(v, BlzVecArg) or v is None else BlzVecArg(None, v, 0, 0) for v in (x, y))
        out = DeviceBuffer(0, 32)
        check(lib().blz_ntt_vec_reduce(cl._h, op, C.byref(vx), None if vy is None else C.byref(vy), out.ptr))
        cl.wait_result()
        v = word(out)
        out.free()
        return v

    SUM, DOT = NTTClient.FOLD_SUM, NTTClient.FOLD_DOT
    inv2 = pow(2, -1, R)
    # w: random words below `half`, zeros above - DOT(buffer, w) sees the words a fold wrote and nothing behind them
    w = DeviceBuffer(0, 32 * n)
    check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 41))
    hip_ok(hip.hipMemsetAsync(w.ptr + 32 * half, 0, 32 * half, stream), "hipMemsetAsync")
    hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    wv = BlzVecArg(w.ptr, 0, 0, n)
    for name in ("fold", "fold_low", "fold_in_place", "fold_low_in_place"):
        kind, low, _, _ = table[name]
        restore()
        run_op(name)
        dst = 1 if kind == "fold" else 0
        got = reduce(DOT, dst, wv)
        if low:   # the halves of the pairs by two decimations of a
            parts = []
            for first in (0, 1):
                cl.vec_gather(dst, a, offset=first, stride=2, length=half)
                cl.wait_result()
                parts.append(reduce(DOT, dst, wv))
            lo, hi = parts
        else:     # ... or as views of a: both operands repeat over the n positions, hence the halving
            lo = reduce(DOT, view(a, half), view(w, half)) * inv2 % R
            hi = reduce(DOT, view(a, half, half), view(w, half)) * inv2 % R
        if got != (lo + rr * (hi - lo)) % R:
            raise RuntimeError(f"{name}: sum w dst differs from sum w lo + r (sum w hi - sum w lo)")
    # the round polynomials: every point through the tables folded at r = t, and s(0) + s(1) through the unfolded ones
    f = [DeviceBuffer(0, 32 * half) for _ in range(3)]
    restore()
    for name in ("round_k1", "round_k2", "round_k3"):   # (the in-place folds of the timed rounds changed buffer 0)
        run_op(name)
    got = {name: [int.from_bytes(bytes(outs[name].download(32, 32 * t)), "little") for t in range(outs[name].nbytes // 32)]
           for name in ("round_k1", "round_k2", "round_k3")}
    for t in range(4):
        d_t = cl.scalar(t)
        for dst, src in zip(f, (0, 1, c)):
            cl.vec_mle_fold(dst, src, d_t)
            cl.wait_result()
        d_t.free()
        fv = [view(d, half) for d in f]
        want = {"round_k1": reduce(SUM, fv[0]) * inv2 % R, "round_k2": reduce(DOT, fv[0], fv[1]) * inv2 % R}
        check(lib().blz_ntt_vec_op(cl._h, NTTClient.MUL, 1, C.byref(fv[0]), C.byref(fv[1]), None))
        cl.wait_result()
        want["round_k3"] = reduce(DOT, 1, fv[2]) * inv2 % R
        restore()
        for name, k in (("round_k1", 1), ("round_k2", 2), ("round_k3", 3)):
            if t <= k and got[name][t] != want[name]:
                raise RuntimeError(f"{name}: out[{t}] differs from the reduction of the tables folded at {t}")
    whole = {"round_k1": reduce(SUM, 0), "round_k2": reduce(DOT, 0, 1)}
    for name, v in whole.items():
        if (got[name][0] + got[name][1]) % R != v:
            raise RuntimeError(f"{name}: out[0] + out[1] differs from the reduction of the whole table")
    # the equality table
    run_op("eq")
    if reduce(SUM, 1) != 1:
        raise RuntimeError("eq: the table does not add up to 1")
    e = DeviceBuffer(0, 32 * n)
    cl.result_device(1, e)
    for p in [0, 1, n - 1] + [rng.randrange(n) for _ in range(253)]:
        v = 1
        for i, t in enumerate(tau):
            v = v * (t if (p >> i) & 1 else 1 - t) % R
        if int.from_bytes(bytes(e.download(32, 32 * p)), "little") != v:
            raise RuntimeError(f"eq: word {p} differs from the product formula")
    for d in f + [e, w, a, b, c, point, d_r] + list(outs.values()):
        d.free()
    cl.close()

    # ---- a whole sumcheck of m variables: sum_p eq(p) (Az(p) Bz(p) - Cz(p)) = 0 with Cz = Az o Bz
    m = logn - 3
    size = 1 << m
    sc = NTTClient(NTT.Ntt, dc, log_size=m, flags=NTTClient.NO_FACTOR_TABLE)
    d_cz, d_eq, d_pt = DeviceBuffer(0, 32 * size), DeviceBuffer(0, 32 * size), DeviceBuffer(0, 32 * m)
    for i in (0, 1):
        check(blaze_amd.aux().blz_synth_field_elements(0, d_eq.ptr, size, 51 + i))
        check(lib().blz_ntt_set_data_device(sc._h, i, d_eq.ptr, d_eq.nbytes))
    sc.vec_op(NTTClient.MUL, 0, 0, 1)   # buffer 0 = Az o Bz ...
    sc.wait_result()
    sc.result_device(0, d_cz)           # ... = Cz
    check(blaze_amd.aux().blz_synth_field_elements(0, d_eq.ptr, size, 51))   # Az again
    check(lib().blz_ntt_set_data_device(sc._h, 0, d_eq.ptr, d_eq.nbytes))
    d_pt.upload(b"".join(rng.getrandbits(256).to_bytes(32, "little") for _ in range(m)))
    s1, s2 = DeviceBuffer(0, 128), DeviceBuffer(0, 128)
    device_ms, claim = 0.0, 0
    t0 = time.perf_counter()
    sc.vec_mle_eq(d_eq, d_pt)
    sc.wait_result()
    device_ms += sc.last_kernel_ms()
    for rnd in range(m):
        length = size >> rnd
        sc.vec_mle_round(d_eq, 0, 1, points=4, length=length, out=s1)
        sc.wait_result()
        device_ms += sc.last_kernel_ms()
        sc.vec_mle_round(d_eq, d_cz, points=4, length=length, out=s2)
        sc.wait_result()
        device_ms += sc.last_kernel_ms()
        x, y = bytes(s1.download()), bytes(s2.download())
        s = [(int.from_bytes(x[32 * t: 32 * t + 32], "little") - int.from_bytes(y[32 * t: 32 * t + 32], "little")) % R for t in range(4)]
        if (s[0] + s[1]) % R != claim:
            raise RuntimeError(f"sumcheck round {rnd}: s(0) + s(1) differs from the claim")
        ch = rng.getrandbits(256)
        d_ch = sc.scalar(ch)
        for tb in (0, 1, d_cz, d_eq):
            sc.vec_mle_fold(tb, tb, d_ch, length)
            sc.wait_result()
            device_ms += sc.last_kernel_ms()
        d_ch.free()
        claim = interpolate(s, ch)
    wall_ms = (time.perf_counter() - t0) * 1e3
    fin = []
    for tb in (0, 1):
        tmp = DeviceBuffer(0, 32 * size)
        sc.result_device(tb, tmp)
        fin.append(word(tmp))
        tmp.free()
    fin += [word(d_cz), word(d_eq)]
    if claim != fin[3] * (fin[0] * fin[1] - fin[2]) % R:
        raise RuntimeError("sumcheck: the last claim differs from eq (Az Bz - Cz) at the challenges")
    sc.close()
    for d in (d_cz, d_eq, d_pt, s1, s2):
        d.free()

    res = {"log_size": logn, "field": "BLS381", "rounds": rounds, "calib_mad_rate": cal[0], "calib_clock_mhz": cal[2], "checked": True,
           "cases": {}}
    for k, (kind, arg, words, products) in table.items():
        om, cm = statistics.median(op_ms[k]), statistics.median(cp_ms[k])
        units = n if kind == "eq" else half   # words written (eq) or pairs
        mads = int(products * MADS_PER_PRODUCT * units)
        res["cases"][k] = {
            "len": n, "bytes_moved": words * 32, "yardstick_copy_bytes": words * 32 // 2,
            "kernel_ms": round(om, 4), "kernel_ms_min_max": [round(min(op_ms[k]), 4), round(max(op_ms[k]), 4)],
            "achieved_tb_per_s": round(words * 32 / om / 1e9, 3),
            "yardstick_copy_ms": round(cm, 4), "yardstick_copy_ms_min_max": [round(min(cp_ms[k]), 4), round(max(cp_ms[k]), 4)],
            "ratio_to_copy": round(om / cm, 4),
            "products_per_unit": products, "product_multiply_adds": mads,
            "multiply_add_issue_ms_at_calibrated_rate": round(mads / cal[0] * 1e3, 4) if cal[0] else None,
        }
    res["sumcheck"] = {"variables": m, "ops": 1 + 6 * m, "device_ms": round(device_ms, 3), "wall_ms": round(wall_ms, 3),
                       "note": "eq, then per round 2 round polynomials (k = 3 and k = 2, 4 points), a challenge upload and 4 folds in place; "
                               "synthetic tables with Cz = Az o Bz, no sparse product"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_mle_ops.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log-size", type=int, default=27)
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
