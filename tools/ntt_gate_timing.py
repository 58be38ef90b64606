#!/usr/bin/env python3
"""What the sumcheck step for caller-defined gates costs over the BLS12-381 scalar field (blz_ntt_sumcheck_gate; DESIGN.md
section 4, "Caller-defined gates"): medians of blz_ntt_last_kernel_ms with min - max, every case alternating in the same process
with its yardsticks.
    R1CS written as a sum gate (common = eq, + Az Bz, - Cz) with r at len = n = 2^24, and at 2^27 where memory allows (eq and Cz
        in device words, Az and Bz in the buffers), against BLZ_GATE_R1CS of blz_ntt_sumcheck_step on the same tables - both do
        18 products per quad, so the ratio is the price of the re-reads and the rolled loops - and against a device-to-device
        hipMemcpyAsync of 3 len words, the 6 len words either moves.
    the vanilla PLONK gate eq (qL a + qR b + qM a b - qO c + qC), nine tables in device words, 5 points, with r at len = n =
        2^24, as ONE step, against the sequence of existing ops that comes closest, 48 of them, kernel times summed: nine
        vec_mle_fold in place; round(eq, qL, a; 4), round(eq, qR, b; 4), round(eq, qO, c; 4), round(eq, qC; 4) at len / 2 - degree
        <= 3, the fifth point follows from four on the host -; and for eq qM a b, degree 4 over four tables, which no existing
        round takes, per point t = 0 .. 4: vec_mle_fold of eq, qM, a, b with r = t into len / 4 words (T(t) = lo + t (hi - lo)),
        vec_op MUL twice and vec_reduce DOT on a handle of len / 4 positions; and against a copy of 6.75 len words, the
        13.5 len the step moves.
The outputs are checked on the device before anything is written: the generic R1CS step's four words and its folded tables (a DOT
with a random vector each) equal the specialised step's; the PLONK step's five words equal the sequence's, and its nine folded
tables vec_mle_fold's.  Writes profiles/ntt_gate_step.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_gate_timing.py [--out profiles/ntt_gate_step.json] [--rounds 9] [--timeout 900] [--no-large]
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001   # BLS12-381 Fr
R1CS_TERMS = [(1, [1, 2]), (-1, [3])]                                             # over [eq, Az, Bz, Cz], common = 0
PLONK_TERMS = [(1, [1, 6]), (1, [2, 7]), (1, [3, 6, 7]), (-1, [4, 8]), (1, [5])]  # over [eq, qL, qR, qM, qO, qC, a, b, c], common = 0


def fifth_point(s):
    """s(4) of the polynomial of degree <= 3 through (t, s[t]), t < 4: the fourth finite difference is 0"""
    return (4 * s[3] - 6 * s[2] + 4 * s[1] - s[0]) % R


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def child(rounds: int, large: bool) -> dict:
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

    R1CS, DOT, MUL = NTTClient.GATE_R1CS, NTTClient.FOLD_DOT, NTTClient.MUL
    dc = DriverClient(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def words(d, k):
        x = bytes(d.download(32 * k))
        return [int.from_bytes(x[32 * t: 32 * t + 32], "little") for t in range(k)]

    def stream_of(cl):
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        return stream

    def copier(stream, moved):
        c_src, c_dst = DeviceBuffer(0, moved), DeviceBuffer(0, moved)
        hip_ok(hip.hipMemsetAsync(c_src.ptr, 1, moved, stream), "hipMemsetAsync")
        hip_ok(hip.hipMemsetAsync(c_dst.ptr, 2, moved, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        def copy():
            ms = C.c_float()
            hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
            hip_ok(hip.hipMemcpyAsync(c_dst.ptr, c_src.ptr, moved, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
            hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
            hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
            hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
            return float(ms.value)

        return copy, (c_src, c_dst)

    def digests(cl, tabs, w):
        got = []
        for t in tabs:
            d = cl.vec_reduce(DOT, t, w)
            cl.wait_result()
            got.append(bytes(d.download()))
            d.free()
        return got

    def random_vector(n, half, stream):
        """a random vector that is zero above len / 2: a DOT with it is a digest of a table's folded words"""
        w = DeviceBuffer(0, 32 * n)
        check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 71))
        hip_ok(hip.hipMemsetAsync(w.ptr + 32 * half, 0, 32 * half, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        return w

    def r1cs_case(logn):
        """R1CS as a sum gate beside BLZ_GATE_R1CS and a copy of the words either moves, len = n = 2^logn"""
        n, half = 1 << logn, 1 << (logn - 1)
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        stream = stream_of(cl)
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

        d_r = cl.scalar(random.Random(logn).getrandbits(256))
        out_g, out_s = DeviceBuffer(0, 128), DeviceBuffer(0, 128)
        copy, cbufs = copier(stream, 3 * n * 32)

        def generic():
            cl.sumcheck_gate(tabs, R1CS_TERMS, 0, r=d_r, points=4, out=out_g)
            cl.wait_result()
            return cl.last_kernel_ms()

        def special():
            cl.sumcheck_step(tabs, d_r, gate=R1CS, out=out_s)
            cl.wait_result()
            return cl.last_kernel_ms()

        g_ms, s_ms, c_ms = [], [], []
        for it in range(rounds + 2):   # two warm-up rounds; the tables start afresh for each side (restoring is not timed)
            restore()
            x = generic()
            restore()
            y = special()
            z = copy()
            if it >= 2:
                g_ms.append(x)
                s_ms.append(y)
                c_ms.append(z)
        for d in cbufs:
            d.free()
        w = random_vector(n, half, stream)
        restore()
        special()
        want_tables, want = digests(cl, tabs, w), words(out_s, 4)
        restore()
        generic()
        if words(out_g, 4) != want:
            raise RuntimeError(f"2^{logn}: the generic step's round polynomial differs from BLZ_GATE_R1CS's")
        if digests(cl, tabs, w) != want_tables:
            raise RuntimeError(f"2^{logn}: a table the generic step folded differs from the specialised step's")
        if len(set(want_tables)) != 4 or not any(want):
            raise RuntimeError(f"2^{logn}: degenerate check")
        for d in src + [d_eq, d_cz, d_r, out_g, out_s, w]:
            d.free()
        cl.close()
        gs, ss, cs = stats(g_ms), stats(s_ms), stats(c_ms)
        return {"len": n, "bytes_moved": 6 * n * 32, "products_per_quad": 18, "generic_gate_step": gs, "specialised_r1cs_step": ss,
                "copy_of_the_bytes_moved": cs, "generic_to_specialised": round(gs["median_ms"] / ss["median_ms"], 4),
                "generic_to_copy": round(gs["median_ms"] / cs["median_ms"], 4),
                "specialised_spread_ms": round(ss["min_max_ms"][1] - ss["min_max_ms"][0], 4), "checked": True}

    def plonk_case(logn):
        """the PLONK gate as one step beside the 48 existing ops that come closest and a copy of the words the step moves"""
        n, half, quarter = 1 << logn, 1 << (logn - 1), 1 << (logn - 2)
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        small = NTTClient(NTT.Ntt, dc, log_size=logn - 2, flags=NTTClient.NO_FACTOR_TABLE)   # vec_op and DOT over len / 4 positions
        stream = stream_of(cl)
        src = [DeviceBuffer(0, 32 * n) for _ in range(9)]
        for i, d in enumerate(src):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 81 + i))
        tabs = [DeviceBuffer(0, 32 * n) for _ in range(9)]
        eq, qL, qR, qM, qO, qC, a, b, c = tabs

        def restore():
            for t, s in zip(tabs, src):
                hip_ok(hip.hipMemcpyAsync(t.ptr, s.ptr, 32 * n, 3, stream), "hipMemcpyAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        d_r = cl.scalar(random.Random(100 + logn).getrandbits(256))
        d_t = [cl.scalar(t) for t in range(5)]
        out = DeviceBuffer(0, 32 * 5)
        rounds_out = [DeviceBuffer(0, 128) for _ in range(4)]
        at_t = [DeviceBuffer(0, 32 * quarter) for _ in range(4)]   # eq, qM, a, b at the point t
        dots = [DeviceBuffer(0, 32) for _ in range(5)]
        copy, cbufs = copier(stream, 27 * n * 8)   # 6.75 n words: the step reads 9 n and writes 4.5 n

        def fused():
            cl.sumcheck_gate(tabs, PLONK_TERMS, 0, r=d_r, points=5, out=out)
            cl.wait_result()
            return cl.last_kernel_ms()

        def unfused():
            """-> the kernel times of the 48 ops; rounds_out and dots then hold the parts of the round polynomial"""
            ms = []

            def done(client):
                client.wait_result()
                ms.append(client.last_kernel_ms())

            for t in tabs:
                cl.vec_mle_fold(t, t, d_r, n)
                done(cl)
            for ops, o in (((eq, qL, a), rounds_out[0]), ((eq, qR, b), rounds_out[1]), ((eq, qO, c), rounds_out[2]), ((eq, qC), rounds_out[3])):
                cl.vec_mle_round(*ops, points=4, length=half, out=o)
                done(cl)
            for t in range(5):
                for srct, dst in zip((eq, qM, a, b), at_t):
                    cl.vec_mle_fold(dst, srct, d_t[t], half)
                    done(cl)
                small.vec_op(MUL, 0, at_t[1], at_t[2])
                done(small)
                small.vec_op(MUL, 0, 0, at_t[3])
                done(small)
                small.vec_reduce(DOT, 0, at_t[0], out=dots[t])
                done(small)
            return ms

        def unfused_polynomial():
            parts = [words(o, 4) for o in rounds_out]
            parts = [p + [fifth_point(p)] for p in parts]
            qm = [words(d, 1)[0] for d in dots]
            return [(parts[0][t] + parts[1][t] + qm[t] - parts[2][t] + parts[3][t]) % R for t in range(5)]

        f_ms, u_ms, c_ms = [], [], []
        for it in range(rounds + 2):
            restore()
            x = fused()
            restore()
            y = unfused()
            z = copy()
            if it >= 2:
                f_ms.append(x)
                u_ms.append(sum(y))
                c_ms.append(z)
        assert len(y) == 48
        for d in cbufs:
            d.free()
        w = random_vector(n, half, stream)
        want_tables, want = digests(cl, tabs, w), unfused_polynomial()   # the last round's unfused run is still in place
        restore()
        fused()
        if words(out, 5) != want:
            raise RuntimeError(f"2^{logn}: the PLONK step's round polynomial differs from the unfused sequence's")
        if digests(cl, tabs, w) != want_tables:
            raise RuntimeError(f"2^{logn}: a table the PLONK step folded differs from vec_mle_fold's")
        if len(set(want_tables)) != 9 or not all(want):
            raise RuntimeError(f"2^{logn}: degenerate check")
        for d in src + tabs + d_t + rounds_out + at_t + dots + [d_r, out, w]:
            d.free()
        cl.close()
        small.close()
        fs, us, cs = stats(f_ms), stats(u_ms), stats(c_ms)
        return {"len": n, "tables": 9, "points": 5, "bytes_moved": 27 * n * 16, "products_per_quad": 58, "gate_step": fs, "unfused_ops": 48,
                "unfused_sequence": us, "copy_of_the_bytes_moved": cs, "step_to_unfused": round(fs["median_ms"] / us["median_ms"], 4),
                "step_to_copy": round(fs["median_ms"] / cs["median_ms"], 4), "achieved_tb_per_s": round(27 * n * 16 / fs["median_ms"] / 1e9, 3),
                "checked": True}

    res = {"field": "BLS381", "rounds": rounds, "r1cs_as_a_sum_gate": {}, "plonk_gate": {}}
    res["r1cs_as_a_sum_gate"]["2^24"] = r1cs_case(24)
    res["plonk_gate"]["2^24"] = plonk_case(24)
    if large:
        try:
            res["r1cs_as_a_sum_gate"]["2^27"] = r1cs_case(27)
        except blaze_amd.DriverClientError as e:   # the memory for it (some 64 GiB) is not there: the smaller size stands alone
            res["r1cs_as_a_sum_gate"]["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_gate_step.json"))
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
