#!/usr/bin/env python3
"""What gate evaluation on resident buffers costs over the BLS12-381 scalar field (blz_ntt_gate_eval; DESIGN.md section 4, "Gate
evaluation"): medians of blz_ntt_last_kernel_ms with min - max, every leg alternating in the same process with its two
yardsticks - the shortest sequence of existing ops that computes the same bytes (kernel times summed; the sequence is written
into the JSON) and a device-to-device hipMemcpyAsync of half the bytes the fused op moves, which moves as many.
    plonk            qL a + qR b + qM a b - qO c + qC over eight n-word tables in device words into buffer 0, n = 2^24 and, where
                     memory allows, 2^27; five vec_op calls
    plonk_scalars    the same gate with the five selectors one word each
    lincomb6         sum_{j < 6} c_j f_j with one-word c_j; six vec_op calls
    plonk_rotated    the first gate with c read four positions ahead; vec_gather into buffer 1 and the five calls
The outputs are checked on the device before anything is written: a DOT of buffer 0 with a random vector after the fused op
equals the one after the sequence.  Writes profiles/ntt_geval_ops.json.  The device work runs in ONE child process under its own
time limit.

    python tools/ntt_geval_timing.py [--out profiles/ntt_geval_ops.json] [--rounds 9] [--timeout 900] [--no-large]
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

PLONK_TERMS = [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (-1, [3, 7]), (1, [4])]   # over [qL, qR, qM, qO, qC, a, b, c]
PLONK_SEQUENCE = ["buf1 = MULSUB(qO, c, qC)", "buf0 = MUL(qM, a)", "buf0 = MULSUB(buf0, b, buf1)", "buf0 = MULADD(qL, a, buf0)",
                  "buf0 = MULADD(qR, b, buf0)"]
LIN_TERMS = [(1, [2 * j, 2 * j + 1]) for j in range(6)]                            # over [c0, f0, c1, f1, ..]
LIN_SEQUENCE = ["buf0 = MUL(c0, f0)"] + [f"buf0 = MULADD(c{j}, f{j}, buf0)" for j in range(1, 6)]


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

    MUL, MULADD, MULSUB, DOT = NTTClient.MUL, NTTClient.MULADD, NTTClient.MULSUB, NTTClient.FOLD_DOT
    dc = DriverClient(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def size_case(logn):
        """every leg at n = 2^logn (the large size: the first leg alone) on one handle and one set of tables"""
        n = 1 << logn
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        full = [DeviceBuffer(0, 32 * n) for _ in range(8)]   # qL, qR, qM, qO, qC, a, b, c - and c0 .. : f0 .. f5 are the first six
        for i, d in enumerate(full):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 131 + i))
        rng = random.Random(logn)
        one = [cl.scalar(rng.getrandbits(256)) for _ in range(6)]
        w = DeviceBuffer(0, 32 * n)
        check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 171))

        def copier(moved):
            c_src, c_dst = DeviceBuffer(0, moved // 2), DeviceBuffer(0, moved // 2)
            hip_ok(hip.hipMemsetAsync(c_src.ptr, 1, moved // 2, stream), "hipMemsetAsync")
            hip_ok(hip.hipMemsetAsync(c_dst.ptr, 2, moved // 2, stream), "hipMemsetAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

            def copy():
                ms = C.c_float()
                hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
                hip_ok(hip.hipMemcpyAsync(c_dst.ptr, c_src.ptr, moved // 2, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
                hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
                hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
                hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
                return float(ms.value)

            return copy, (c_src, c_dst)

        def op(f, *args):
            f(*args)
            cl.wait_result()
            return cl.last_kernel_ms()

        def digest():
            d = cl.vec_reduce(DOT, 0, w)
            cl.wait_result()
            got = bytes(d.download())
            d.free()
            return got

        def plonk_sequence(t, rotated):
            qL, qR, qM, qO, qC, a, b, c = t
            ms = []
            if rotated:
                ms.append(op(cl.vec_rotate, 1, c, 4))
                c = 1
            ms.append(op(cl.vec_op, MULSUB, 1, qO, c, qC))
            ms.append(op(cl.vec_op, MUL, 0, qM, a))
            ms.append(op(cl.vec_op, MULSUB, 0, 0, b, 1))
            ms.append(op(cl.vec_op, MULADD, 0, qL, a, 0))
            ms.append(op(cl.vec_op, MULADD, 0, qR, b, 0))
            return ms

        def lin_sequence(t):
            ms = [op(cl.vec_op, MUL, 0, t[0], t[1])]
            for j in range(1, 6):
                ms.append(op(cl.vec_op, MULADD, 0, t[2 * j], t[2 * j + 1], 0))
            return ms

        def leg(tables, terms, rot, sequence, names, products, words_moved):
            """words_moved: the n-word vectors the fused op reads and writes (one-word tables not counted)"""
            moved = words_moved * n * 32
            copy, cbufs = copier(moved)
            f_ms, s_ms, c_ms = [], [], []
            for it in range(rounds + 2):   # two warm-up rounds
                x = op(cl.gate_eval, 0, tables, terms, None, rot)
                y = sequence()
                z = copy()
                if it >= 2:
                    f_ms.append(x)
                    s_ms.append(sum(y))
                    c_ms.append(z)
            want = digest()   # the last round's sequence is still in buffer 0
            op(cl.vec_op, MUL, 0, w, w)   # (so that the bytes compared next are the fused op's)
            op(cl.gate_eval, 0, tables, terms, None, rot)
            if digest() != want or not any(want):
                raise RuntimeError(f"2^{logn}: the fused op's output differs from the sequence's ({names})")
            for d in cbufs:
                d.free()
            fs, ss, cs = stats(f_ms), stats(s_ms), stats(c_ms)
            return {"n": n, "products_per_position": products, "bytes_moved": moved, "gate_eval": fs, "sequence_of_existing_ops": names,
                    "sequence": ss, "copy_of_the_bytes_moved": cs, "fused_to_sequence": round(fs["median_ms"] / ss["median_ms"], 4),
                    "fused_to_copy": round(fs["median_ms"] / cs["median_ms"], 4), "achieved_tb_per_s": round(moved / fs["median_ms"] / 1e9, 3),
                    "checked": True}

        res = {"plonk": leg(full, PLONK_TERMS, None, lambda: plonk_sequence(full, False), PLONK_SEQUENCE, 9, 9)}
        if logn <= 24:
            scal = one[:5] + full[5:]
            res["plonk_scalars"] = leg(scal, PLONK_TERMS, None, lambda: plonk_sequence(scal, False), PLONK_SEQUENCE, 9, 4)
            lin = [x for j in range(6) for x in (one[j], full[j])]
            res["lincomb6"] = leg(lin, LIN_TERMS, None, lambda: lin_sequence(lin), LIN_SEQUENCE, 12, 7)
            res["plonk_rotated"] = leg(full, PLONK_TERMS, [0] * 7 + [4], lambda: plonk_sequence(full, True),
                                       ["buf1 = GATHER(c, offset 4)", "buf1 = MULSUB(qO, buf1, qC)"] + PLONK_SEQUENCE[1:], 9, 9)
        for d in full + one + [w]:
            d.free()
        cl.close()
        return res

    res = {"field": "BLS381", "rounds": rounds, "2^24": size_case(24)}
    if large:
        try:
            res["2^27"] = size_case(27)
        except blaze_amd.DriverClientError as e:   # the memory for it (some 70 GiB) is not there: the smaller size stands alone
            res["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_geval_ops.json"))
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
