#!/usr/bin/env python3
"""What the zerocheck step costs over the BLS12-381 scalar field (blz_ntt_zerocheck_gate; DESIGN.md section 4, "Zerocheck step"):
medians of blz_ntt_last_kernel_ms with min - max, every case alternating in the same process with its yardsticks.
    step legs, with r at len = n = 2^24 and, where memory allows, 2^27:
        R1CS   W (Az Bz - Cz), 3 points, 14 products per quad, against blz_ntt_sumcheck_gate over eq (Az Bz - Cz), 4 points, 18;
        PLONK  W (qL a + qR b + qM a b - qO c + qC), eight tables, 4 points, 50, against the nine tables with common = eq, 5
               points, 58;
        each also against a device-to-device hipMemcpyAsync of half the words the new step moves (a copy reads and writes).
        eq and W are real equality tables of one random point (blz_ntt_vec_mle_eq over m and m - 1 variables), the other tables
        random field elements; every table is restored from a pristine copy before each timed call (not timed).
    a whole 24-variable R1CS zerocheck both ways - vec_mle_eq, the round alone, 23 steps with r, the bind alone; a fresh challenge
        uploaded and the round polynomial downloaded every round, as a prover with a host transcript does -: the sum of the
        kernel times and the wall time of the loop.
The outputs are checked on the device before anything is timed: at every point s(t) = c eq(tau_top, t) u(t) between the two steps'
round polynomials (Python integers on the downloaded words), the tables either folded are equal (a DOT with a random vector each),
and the summed weight is the equality table over one variable fewer.  Writes profiles/ntt_zerocheck_step.json.  The device work
runs in ONE child process under its own time limit.

    python tools/ntt_zerocheck_timing.py [--out profiles/ntt_zerocheck_step.json] [--rounds 9] [--timeout 900] [--no-large]
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
GATES = {
    # name: (tables without eq, terms of the new step, terms over [eq] + tables with common = 0, products per quad new / old)
    "r1cs": (3, [(1, [0, 1]), (-1, [2])], [(1, [1, 2]), (-1, [3])], 14, 18),
    "plonk": (8, [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (-1, [3, 7]), (1, [4])], [(1, [1, 6]), (1, [2, 7]), (1, [3, 6, 7]), (-1, [4, 8]), (1, [5])], 50, 58),
}


def eq1(a, x):
    return (a * x + (1 - a) * (1 - x)) % R


def extend(u):
    """u(len(u)) of the polynomial of degree < len(u) through (t, u[t]): the len(u)-th finite difference is 0"""
    k, s, c = len(u), 0, 1
    for j in range(1, k + 1):
        c = c * (k - j + 1) // j
        s += (-1) ** (j + 1) * c * u[k - j]
    return s % R


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

    DOT = NTTClient.FOLD_DOT
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

    def digest(cl, t, w):
        d = cl.vec_reduce(DOT, t, w)
        cl.wait_result()
        got = bytes(d.download())
        d.free()
        return got

    def eq_tables(cl, m, seed):
        """(tau, the point on the device, eq over m, m - 1 and m - 2 variables as pristine device words)"""
        tau = [random.Random(seed + i).getrandbits(256) for i in range(m)]
        point = DeviceBuffer(0, 32 * m)
        point.upload(b"".join(v.to_bytes(32, "little") for v in tau))
        tabs = []
        for k in (m, m - 1, m - 2):
            d = DeviceBuffer(0, 32 << k)
            cl.vec_mle_eq(d, point, k)
            cl.wait_result()
            tabs.append(d)
        return tau, point, tabs

    def step_case(name, logn):
        """the new step beside blz_ntt_sumcheck_gate with common = eq and a copy, with r at len = n = 2^logn"""
        nt, terms, eq_terms, prod_new, prod_old = GATES[name]
        n, half, quarter = 1 << logn, 1 << (logn - 1), 1 << (logn - 2)
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        stream = stream_of(cl)
        tau, point, (src_e, src_w, eq2) = eq_tables(cl, logn, 500 + logn)
        src = [DeviceBuffer(0, 32 * n) for _ in range(nt)]
        for i, d in enumerate(src):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 91 + i))
        d_e, d_w = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 32 * half)
        tabs = [DeviceBuffer(0, 32 * n) for _ in range(nt)]

        def restore():
            for t, s in zip(tabs + [d_e, d_w], src + [src_e, src_w]):
                hip_ok(hip.hipMemcpyAsync(t.ptr, s.ptr, s.nbytes, 3, stream), "hipMemcpyAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        x = random.Random(logn).getrandbits(256)
        d_r = cl.scalar(x)
        deg = max(len(f) for _, f in terms)
        out_new, out_old = DeviceBuffer(0, 32 * (deg + 1)), DeviceBuffer(0, 32 * (deg + 2))
        # words moved by the new step: every table len read and len / 2 written, the weight len / 2 read and len / 4 written
        moved_words = 1.5 * n * nt + 0.75 * n
        copy, cbufs = copier(stream, int(moved_words * 16))

        def new():
            cl.zerocheck_gate(tabs, terms, d_w, r=d_r, points=deg + 1, out=out_new)
            cl.wait_result()
            return cl.last_kernel_ms()

        def old():
            cl.sumcheck_gate([d_e] + tabs, eq_terms, 0, r=d_r, points=deg + 2, out=out_old)
            cl.wait_result()
            return cl.last_kernel_ms()

        # the check, before anything is timed
        w = DeviceBuffer(0, 32 * n)
        check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 71))
        hip_ok(hip.hipMemsetAsync(w.ptr + 32 * half, 0, 32 * half, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        restore()
        old()
        want_tables, s = [digest(cl, t, w) for t in tabs], words(out_old, deg + 2)
        restore()
        new()
        u = words(out_new, deg + 1)
        c1 = eq1(tau[logn - 1], x)
        u_ext = u + [extend(u)]
        if any(s[t] != c1 * eq1(tau[logn - 2], t) * u_ext[t] % R for t in range(deg + 2)):
            raise RuntimeError(f"{name} 2^{logn}: s(t) = c eq(tau, t) u(t) does not hold between the two steps")
        if [digest(cl, t, w) for t in tabs] != want_tables:
            raise RuntimeError(f"{name} 2^{logn}: a table the new step folded differs from blz_ntt_sumcheck_gate's")
        wq = DeviceBuffer(0, 32 * quarter)   # the weight's first len / 4 words against eq over m - 2 variables, under one random vector
        hip_ok(hip.hipMemcpyAsync(wq.ptr, d_w.ptr, 32 * quarter, 3, stream), "hipMemcpyAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        small = NTTClient(NTT.Ntt, dc, log_size=logn - 2, flags=NTTClient.NO_FACTOR_TABLE)
        wv = DeviceBuffer(0, 32 * quarter)
        check(blaze_amd.aux().blz_synth_field_elements(0, wv.ptr, quarter, 72))
        if digest(small, wq, wv) != digest(small, eq2, wv):
            raise RuntimeError(f"{name} 2^{logn}: the summed weight is not the equality table over one variable fewer")
        if len(set(want_tables)) != nt or not all(u) or not all(s):
            raise RuntimeError(f"{name} 2^{logn}: degenerate check")
        small.close()
        for d in (w, wq, wv):
            d.free()

        n_ms, o_ms, c_ms = [], [], []
        for it in range(rounds + 2):   # two warm-up rounds; the tables start afresh for each side (restoring is not timed)
            restore()
            a = new()
            restore()
            b = old()
            z = copy()
            if it >= 2:
                n_ms.append(a)
                o_ms.append(b)
                c_ms.append(z)
        for d in list(cbufs) + src + tabs + [src_e, src_w, eq2, d_e, d_w, d_r, out_new, out_old, point]:
            d.free()
        cl.close()
        ns, os_, cs = stats(n_ms), stats(o_ms), stats(c_ms)
        return {"len": n, "tables": nt, "points": deg + 1, "products_per_quad": prod_new, "bytes_moved": int(moved_words * 32),
                "zerocheck_step": ns, "sumcheck_gate_with_eq": dict(os_, points=deg + 2, products_per_quad=prod_old, bytes_moved=int(1.5 * n * (nt + 1) * 32)),
                "copy_of_the_bytes_moved": cs, "new_to_old": round(ns["median_ms"] / os_["median_ms"], 4),
                "expected_from_products": round(prod_new / prod_old, 4), "new_range_wholly_below_old": ns["min_max_ms"][1] < os_["min_max_ms"][0],
                "new_to_copy": round(ns["median_ms"] / cs["median_ms"], 4), "achieved_tb_per_s": round(moved_words * 32 / ns["median_ms"] / 1e9, 3),
                "checked": True}

    def whole_zerocheck(m):
        """an m-variable R1CS zerocheck both ways: device time (kernel times summed) and wall time of the m + 2 ops"""
        nt, terms, eq_terms, _, _ = GATES["r1cs"]
        n = 1 << m
        cl = NTTClient(NTT.Ntt, dc, log_size=m, flags=NTTClient.NO_FACTOR_TABLE)
        stream = stream_of(cl)
        rng = random.Random(600 + m)
        point = DeviceBuffer(0, 32 * m)
        point.upload(rng.randbytes(32 * m))
        src = [DeviceBuffer(0, 32 * n) for _ in range(nt)]
        for i, d in enumerate(src):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 95 + i))
        tabs = [DeviceBuffer(0, 32 * n) for _ in range(nt)]
        d_e, d_w = DeviceBuffer(0, 32 * n), DeviceBuffer(0, 16 * n)
        out = DeviceBuffer(0, 32 * 4)

        def run(new):
            for t, s in zip(tabs, src):
                hip_ok(hip.hipMemcpyAsync(t.ptr, s.ptr, s.nbytes, 3, stream), "hipMemcpyAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            dev_ms, polys, d_c = 0.0, [], None
            t0 = time.perf_counter()
            if new:
                cl.vec_mle_eq(d_w, point, m - 1)
            else:
                cl.vec_mle_eq(d_e, point, m)
            cl.wait_result()
            dev_ms += cl.last_kernel_ms()
            for rnd in range(m):
                length = n >> max(rnd - 1, 0)
                if new:
                    cl.zerocheck_gate(tabs, terms, d_w, r=d_c, points=3, length=length, out=out)
                else:
                    cl.sumcheck_gate([d_e] + tabs, eq_terms, 0, r=d_c, points=4, length=length, out=out)
                cl.wait_result()
                dev_ms += cl.last_kernel_ms()
                polys.append(words(out, 3 if new else 4))
                if d_c is not None:
                    d_c.free()
                d_c = cl.scalar(rng.getrandbits(256))
            cl.sumcheck_gate(tabs if new else [d_e] + tabs, terms if new else eq_terms, None if new else 0, r=d_c, points=0, length=2)
            cl.wait_result()
            dev_ms += cl.last_kernel_ms()
            wall_ms = (time.perf_counter() - t0) * 1e3
            d_c.free()
            if not all(any(p) for p in polys):
                raise RuntimeError("whole zerocheck: a round polynomial is all zero")
            return dev_ms, wall_ms

        res = {"new": ([], []), "old": ([], [])}
        for it in range(rounds + 2):
            for way in ("new", "old"):
                d, wl = run(way == "new")
                if it >= 2:
                    res[way][0].append(d)
                    res[way][1].append(wl)
        for d in src + tabs + [d_e, d_w, out, point]:
            d.free()
        cl.close()
        nd, nw, od, ow = stats(res["new"][0]), stats(res["new"][1]), stats(res["old"][0]), stats(res["old"][1])
        return {"variables": m, "ops": m + 2, "zerocheck_gate": {"device": nd, "wall": nw}, "sumcheck_gate_with_eq": {"device": od, "wall": ow},
                "device_new_to_old": round(nd["median_ms"] / od["median_ms"], 4), "wall_new_to_old": round(nw["median_ms"] / ow["median_ms"], 4)}

    res = {"field": "BLS381", "rounds": rounds, "r1cs": {}, "plonk": {}}
    for name in ("r1cs", "plonk"):
        res[name]["2^24"] = step_case(name, 24)
    res["whole_r1cs_zerocheck"] = whole_zerocheck(24)
    if large:
        for name in ("r1cs", "plonk"):
            try:
                res[name]["2^27"] = step_case(name, 27)
            except blaze_amd.DriverClientError as e:   # the memory for it is not there: the smaller size stands alone
                res[name]["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_zerocheck_step.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--no-large", action="store_true", help="leave the 2^27 cases out")
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
