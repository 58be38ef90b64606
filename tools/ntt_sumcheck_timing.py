#!/usr/bin/env python3
"""What the fused sumcheck step costs over the BLS12-381 scalar field (blz_ntt_sumcheck_step; DESIGN.md section 4, "Sumcheck
step"): medians of blz_ntt_last_kernel_ms with min - max, every case alternating in the same process with its yardsticks.
    the R1CS step with r at len = n = 2^24, and at 2^27 where memory allows (eq and Cz in device words, Az and Bz in the buffers)
        against the six ops it replaces - four vec_mle_fold in place, then round(eq, Az, Bz; 4) and round(eq, Cz; 4) at len / 2 -,
        their kernel times summed: the code of the commit before the step existed;
        against a device-to-device hipMemcpyAsync of 3 len words on the handle's stream, HIP-event timed: the 6 len words the step
        moves (a copy of B bytes reads B and writes B).
    the whole sumcheck of 24 variables for sum eq (Az Bz - Cz) = 0 (synthetic tables with Cz = Az o Bz, no sparse product), both
        ways: 145 ops (eq, then per round two round polynomials, a challenge upload and four folds) and 26 ops (eq, a step without
        r, 23 steps with r, a bind alone); device time (the ops' kernel times summed) and wall time of the loop.
The outputs are checked on the device against the unfused ops before anything is written: from the same tables the step's four
words equal round(eq, Az, Bz) - round(eq, Cz) of the folded tables, and every folded table has the DOT with a random vector that
the table folded by vec_mle_fold has; every round of both sumchecks satisfies s(0) + s(1) = claim, both end in
claim = eq (Az Bz - Cz), and their transcripts are the same bytes.
Writes profiles/ntt_sumcheck_step.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_sumcheck_timing.py [--out profiles/ntt_sumcheck_step.json] [--rounds 9] [--timeout 900] [--no-large]
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


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def child(rounds: int, large: bool) -> dict:
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

    R1CS, DOT = NTTClient.GATE_R1CS, NTTClient.FOLD_DOT
    dc = DriverClient(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def words4(d):
        x = bytes(d.download(128))
        return [int.from_bytes(x[32 * t: 32 * t + 32], "little") for t in range(4)]

    def step_case(logn):
        """the R1CS step with r at len = n = 2^logn beside the six ops it replaces and a copy of the words it moves"""
        n, half = 1 << logn, 1 << (logn - 1)
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        src = [DeviceBuffer(0, 32 * n) for _ in range(4)]   # eq, Az, Bz, Cz as they start
        for i, d in enumerate(src):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 61 + i))
        d_eq, d_cz = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * n)
        tabs = [d_eq, 0, 1, d_cz]

        def restore():
            check(lib().blz_ntt_set_data_device(cl._h, 0, src[1].ptr, src[1].nbytes))
            check(lib().blz_ntt_set_data_device(cl._h, 1, src[2].ptr, src[2].nbytes))
            hip_ok(hip.hipMemcpyAsync(d_eq.ptr, src[0].ptr, 32 * n, 3, stream), "hipMemcpyAsync")
            hip_ok(hip.hipMemcpyAsync(d_cz.ptr, src[3].ptr, 32 * n, 3, stream), "hipMemcpyAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        rng = random.Random(logn)
        d_r = cl.scalar(rng.getrandbits(256))
        out, s1, s2 = DeviceBuffer(0, 128), DeviceBuffer(0, 128), DeviceBuffer(0, 128)
        moved = 3 * n * 32   # bytes the copy yardstick copies: the step reads 4 n words and writes 2 n
        c_src, c_dst = DeviceBuffer(0, moved), DeviceBuffer(0, moved)
        hip_ok(hip.hipMemsetAsync(c_src.ptr, 1, moved, stream), "hipMemsetAsync")
        hip_ok(hip.hipMemsetAsync(c_dst.ptr, 2, moved, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        def fused():
            cl.sumcheck_step(tabs, d_r, gate=R1CS, out=out)
            cl.wait_result()
            return cl.last_kernel_ms()

        def unfused():
            ms = []
            for t in tabs:
                cl.vec_mle_fold(t, t, d_r, n)
                cl.wait_result()
                ms.append(cl.last_kernel_ms())
            for ops, o in (((d_eq, 0, 1), s1), ((d_eq, d_cz), s2)):
                cl.vec_mle_round(*ops, points=4, length=half, out=o)
                cl.wait_result()
                ms.append(cl.last_kernel_ms())
            return ms

        def copy():
            ms = C.c_float()
            hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
            hip_ok(hip.hipMemcpyAsync(c_dst.ptr, c_src.ptr, moved, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
            hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
            hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
            hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
            return float(ms.value)

        f_ms, u_ms, u_parts, c_ms = [], [], [], []
        for it in range(rounds + 2):   # two warm-up rounds; the tables start afresh for each side (restoring is not timed)
            restore()
            x = fused()
            restore()
            y = unfused()
            z = copy()
            if it >= 2:
                f_ms.append(x)
                u_ms.append(sum(y))
                u_parts.append(y)
                c_ms.append(z)
        c_src.free()
        c_dst.free()
        # ---- checked: the same tables through both, digests by DOT with a random vector that is zero above len / 2
        w = DeviceBuffer(0, 32 * n)
        check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 71))
        hip_ok(hip.hipMemsetAsync(w.ptr + 32 * half, 0, 32 * half, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        def digests():
            got = []
            for t in tabs:
                d = cl.vec_reduce(DOT, t, w)
                cl.wait_result()
                got.append(bytes(d.download()))
                d.free()
            return got

        restore()
        unfused()
        want_tables = digests()
        a, b = words4(s1), words4(s2)
        want = [(x - y) % R for x, y in zip(a, b)]
        restore()
        fused()
        if words4(out) != want:
            raise RuntimeError(f"2^{logn}: the step's round polynomial differs from round(eq, Az, Bz) - round(eq, Cz) of the folded tables")
        if digests() != want_tables:
            raise RuntimeError(f"2^{logn}: a table the step folded differs from vec_mle_fold's")
        if len(set(want_tables)) != 4 or not any(want):
            raise RuntimeError(f"2^{logn}: degenerate check")
        for d in src + [d_eq, d_cz, d_r, out, s1, s2, w]:
            d.free()
        cl.close()
        fs, us, cs = stats(f_ms), stats(u_ms), stats(c_ms)
        names = ["fold_eq", "fold_az", "fold_bz", "fold_cz", "round_eq_az_bz", "round_eq_cz"]
        return {"len": n, "bytes_moved": 6 * n * 32, "step": fs, "unfused_six_ops": us,
                "unfused_parts_median_ms": {k: round(statistics.median(p[i] for p in u_parts), 4) for i, k in enumerate(names)},
                "copy_of_the_bytes_moved": cs, "step_to_unfused": round(fs["median_ms"] / us["median_ms"], 4),
                "step_to_copy": round(fs["median_ms"] / cs["median_ms"], 4), "achieved_tb_per_s": round(6 * n * 32 / fs["median_ms"] / 1e9, 3),
                "unfused_spread_ms": round(us["min_max_ms"][1] - us["min_max_ms"][0], 4),
                "step_under_unfused_by_ms": round(us["median_ms"] - fs["median_ms"], 4), "checked": True}

    def sumcheck_case(m):
        size = 1 << m
        sc = NTTClient(NTT.Ntt, dc, log_size=m, flags=NTTClient.NO_FACTOR_TABLE)
        az, bz, cz = (DeviceBuffer(0, 32 * size) for _ in range(3))
        for i, d in enumerate((az, bz)):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, size, 51 + i))
            check(lib().blz_ntt_set_data_device(sc._h, i, d.ptr, d.nbytes))
        sc.vec_op(NTTClient.MUL, 0, 0, 1)   # buffer 0 = Az o Bz ...
        sc.wait_result()
        sc.result_device(0, cz)             # ... = Cz
        d_cz, d_eq, d_pt = DeviceBuffer(0, 32 * size), DeviceBuffer(0, 32 * size), DeviceBuffer(0, 32 * m)
        rng_pt = random.Random(5)
        d_pt.upload(b"".join(rng_pt.getrandbits(256).to_bytes(32, "little") for _ in range(m)))
        s0, s1, s2 = DeviceBuffer(0, 128), DeviceBuffer(0, 128), DeviceBuffer(0, 128)
        tabs = [d_eq, 0, 1, d_cz]

        def finish(claim):
            fin = []
            for tb in (0, 1):
                tmp = DeviceBuffer(0, 32 * size)
                sc.result_device(tb, tmp)
                fin.append(int.from_bytes(bytes(tmp.download(32)), "little"))
                tmp.free()
            fin += [int.from_bytes(bytes(d.download(32)), "little") for d in (d_cz, d_eq)]
            if claim != fin[3] * (fin[0] * fin[1] - fin[2]) % R:
                raise RuntimeError("sumcheck: the last claim differs from eq (Az Bz - Cz) at the challenges")

        def run(fused_path):
            """-> (device ms, wall ms, ops, transcript)"""
            rng = random.Random(9)
            hip_ok(hip.hipMemcpyAsync(d_cz.ptr, cz.ptr, 32 * size, 3, None), "hipMemcpyAsync")
            check(lib().blz_ntt_set_data_device(sc._h, 0, az.ptr, az.nbytes))
            check(lib().blz_ntt_set_data_device(sc._h, 1, bz.ptr, bz.nbytes))
            hip_ok(hip.hipStreamSynchronize(None), "hipStreamSynchronize")
            device_ms, claim, ops, script, d_ch = 0.0, 0, 0, [], None

            def done():
                nonlocal device_ms, ops
                sc.wait_result()
                device_ms += sc.last_kernel_ms()
                ops += 1

            t0 = time.perf_counter()
            sc.vec_mle_eq(d_eq, d_pt)
            done()
            for rnd in range(m):
                length = size >> rnd
                if fused_path:
                    if rnd == 0:
                        sc.sumcheck_step(tabs, gate=R1CS, length=length, out=s0)
                    else:
                        sc.sumcheck_step(tabs, d_ch, gate=R1CS, length=2 * length, out=s0)
                    done()
                    x = bytes(s0.download())
                    s = [int.from_bytes(x[32 * t: 32 * t + 32], "little") for t in range(4)]
                else:
                    if rnd > 0:
                        for tb in tabs:
                            sc.vec_mle_fold(tb, tb, d_ch, 2 * length)
                            done()
                    sc.vec_mle_round(d_eq, 0, 1, points=4, length=length, out=s1)
                    done()
                    sc.vec_mle_round(d_eq, d_cz, points=4, length=length, out=s2)
                    done()
                    x, y = bytes(s1.download()), bytes(s2.download())
                    s = [(int.from_bytes(x[32 * t: 32 * t + 32], "little") - int.from_bytes(y[32 * t: 32 * t + 32], "little")) % R for t in range(4)]
                if (s[0] + s[1]) % R != claim:
                    raise RuntimeError(f"sumcheck round {rnd}: s(0) + s(1) differs from the claim")
                script.append(s)
                ch = rng.getrandbits(256)
                if d_ch is not None:
                    d_ch.free()
                d_ch = sc.scalar(ch)
                claim = interpolate(s, ch)
            if fused_path:
                sc.sumcheck_step(tabs, d_ch, gate=R1CS, points=0, length=2)
                done()
            else:
                for tb in tabs:
                    sc.vec_mle_fold(tb, tb, d_ch, 2)
                    done()
            wall_ms = (time.perf_counter() - t0) * 1e3
            d_ch.free()
            finish(claim)
            return device_ms, wall_ms, ops, script

        res = {True: [], False: []}
        for it in range(rounds + 2):
            for path in (False, True):
                r = run(path)
                if it >= 2:
                    res[path].append(r)
        if res[True][0][3] != res[False][0][3]:
            raise RuntimeError("sumcheck: the fused transcript differs from the unfused one")
        sc.close()
        for d in (az, bz, cz, d_cz, d_eq, d_pt, s0, s1, s2):
            d.free()
        out = {"variables": m, "note": "synthetic tables with Cz = Az o Bz, no sparse product; the host downloads every round polynomial, "
                                       "interpolates the claim and uploads the challenge inside the wall time", "checked": True}
        for path, name in ((False, "unfused"), (True, "fused")):
            out[name] = {"ops": res[path][0][2], "device": stats([r[0] for r in res[path]]), "wall": stats([r[1] for r in res[path]])}
        return out

    res = {"field": "BLS381", "rounds": rounds, "step_r1cs": {}}
    res["step_r1cs"]["2^24"] = step_case(24)
    res["sumcheck_24"] = sumcheck_case(24)
    if large:
        try:
            res["step_r1cs"]["2^27"] = step_case(27)
        except blaze_amd.DriverClientError as e:   # the memory for it (some 64 GiB) is not there: the smaller size stands alone
            res["step_r1cs"]["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_sumcheck_step.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--no-large", action="store_true", help="leave the 2^27 case out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.rounds, not a.no_large)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)]
                       + (["--no-large"] if a.no_large else []), capture_output=True, text=True)
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
