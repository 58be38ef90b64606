#!/usr/bin/env python3
"""What gate evaluation with linear-form factors costs over the BLS12-381 scalar field (blz_ntt_gate_eval_lin; DESIGN.md
section 4, "Gate evaluation with linear forms"): medians of blz_ntt_last_kernel_ms with min - max, every leg alternating in the
same process with its two yardsticks - the shortest sequence of existing ops that computes the same bytes (kernel times summed;
the sequence is written into the JSON) and a device-to-device hipMemcpyAsync of half the bytes the fused op moves, which moves
as many.
    permutation      Z(wX) prod_j (w_j + beta sigma_j + gamma) - Z prod_j (w_j + beta k_j X + gamma) over eight n-word tables in
                     device words (Z under two indices) and four scalars into buffer 0, n = 2^24 and, where memory allows,
                     2^27; six gate_eval calls into device words and a seventh over them
    logup            beta + gamma f1 + gamma^2 f2 + gamma^3 f3, one form of four summands; one gate_eval call of four terms
    numerator        prod_3 (w_j + beta id_j + gamma); three gate_eval calls into device words and a fourth over them
The outputs are checked on the device before anything is written: a DOT of buffer 0 with a random vector after the fused op
equals the one after the sequence.  Writes profiles/ntt_lineval_ops.json.  The device work runs in ONE child process under its
own time limit.

    python tools/ntt_lineval_timing.py [--out profiles/ntt_lineval_ops.json] [--rounds 9] [--timeout 900] [--no-large]
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

FORM = 0x80
# over [Z (rot 1), Z, a, b, c, sigma1, sigma2, sigma3, X, beta, beta k1, beta k2, gamma]
PERM_FORMS = [[(1, None, 2 + j), (1, 9, 5 + j), (1, None, 12)] for j in range(3)] + [[(1, None, 2 + j), (1, 9 + j, 8), (1, None, 12)] for j in range(3)]
PERM_TERMS = [(1, [0, FORM, FORM + 1, FORM + 2]), (-1, [1, FORM + 3, FORM + 4, FORM + 5])]
PERM_ROT = [1] + [0] * 12
FACTOR_TERMS = [(1, [0]), (1, [1, 2]), (1, [3])]   # w + beta sigma + gamma over [w, beta, sigma, gamma]
PERM_SEQUENCE = [f"t{j} = gate_eval(w{j} + beta sigma{j} + gamma)" for j in range(3)] + [f"t{3 + j} = gate_eval(w{j} + (beta k{j}) X + gamma)" for j in range(3)] \
    + ["buf0 = gate_eval(Z(wX) t0 t1 t2 - Z t3 t4 t5)"]
# over [beta, gamma, gamma^2, gamma^3, f1, f2, f3]
LOGUP_FORMS, LOGUP_TERMS = [[(1, None, 0), (1, 1, 4), (1, 2, 5), (1, 3, 6)]], [(1, [FORM])]
LOGUP_SEQUENCE = ["buf0 = gate_eval(beta + gamma f1 + gamma^2 f2 + gamma^3 f3), four terms"]
# over [a, b, c, id1, id2, id3, beta, gamma]
NUM_FORMS, NUM_TERMS = [[(1, None, j), (1, 6, 3 + j), (1, None, 7)] for j in range(3)], [(1, [FORM, FORM + 1, FORM + 2])]
NUM_SEQUENCE = [f"t{j} = gate_eval(w{j} + beta id{j} + gamma)" for j in range(3)] + ["buf0 = gate_eval(t0 t1 t2)"]


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

    MUL, DOT = NTTClient.MUL, NTTClient.FOLD_DOT
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
        full = [DeviceBuffer(0, 32 * n) for _ in range(8)]   # Z, a, b, c, sigma1 .. sigma3, X
        tmp = [DeviceBuffer(0, 32 * n) for _ in range(6)]    # the sequence's temporaries
        for i, d in enumerate(full):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 231 + i))
        rng = random.Random(logn)
        one = [cl.scalar(rng.getrandbits(256)) for _ in range(4)]   # beta, beta k1, beta k2, gamma - and beta, gamma, gamma^2, gamma^3
        w = DeviceBuffer(0, 32 * n)
        check(blaze_amd.aux().blz_synth_field_elements(0, w.ptr, n, 271))

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

        def perm_sequence(t):
            ms = []
            for j in range(3):
                ms.append(op(cl.gate_eval, tmp[j], [t[2 + j], t[9], t[5 + j], t[12]], FACTOR_TERMS))
                ms.append(op(cl.gate_eval, tmp[3 + j], [t[2 + j], t[9 + j], t[8], t[12]], FACTOR_TERMS))
            ms.append(op(cl.gate_eval, 0, [t[0], t[1]] + tmp, [(1, [0, 2, 3, 4]), (-1, [1, 5, 6, 7])], None, [1] + [0] * 7))
            return ms

        def logup_sequence(t):
            return [op(cl.gate_eval, 0, t, [(1, [0]), (1, [1, 4]), (1, [2, 5]), (1, [3, 6])])]

        def num_sequence(t):
            ms = [op(cl.gate_eval, tmp[j], [t[j], t[6], t[3 + j], t[7]], FACTOR_TERMS) for j in range(3)]
            ms.append(op(cl.gate_eval, 0, tmp[:3], [(1, [0, 1, 2])]))
            return ms

        def leg(tables, forms, terms, rot, sequence, names, products, sequence_products, words_moved):
            """words_moved: the n-word vectors the fused op reads and writes (one-word tables not counted)"""
            moved = words_moved * n * 32
            copy, cbufs = copier(moved)
            f_ms, s_ms, c_ms = [], [], []
            for it in range(rounds + 2):   # two warm-up rounds
                x = op(cl.gate_eval_lin, 0, tables, forms, terms, None, rot)
                y = sequence()
                z = copy()
                if it >= 2:
                    f_ms.append(x)
                    s_ms.append(sum(y))
                    c_ms.append(z)
            want = digest()   # the last round's sequence is still in buffer 0
            op(cl.vec_op, MUL, 0, w, w)   # (so that the bytes compared next are the fused op's)
            op(cl.gate_eval_lin, 0, tables, forms, terms, None, rot)
            if digest() != want or not any(want):
                raise RuntimeError(f"2^{logn}: the fused op's output differs from the sequence's ({names})")
            for d in cbufs:
                d.free()
            fs, ss, cs = stats(f_ms), stats(s_ms), stats(c_ms)
            return {"n": n, "products_per_position": products, "sequence_products_per_position": sequence_products, "bytes_moved": moved,
                    "gate_eval_lin": fs, "sequence_of_existing_ops": names, "sequence": ss, "copy_of_the_bytes_moved": cs,
                    "fused_to_sequence": round(fs["median_ms"] / ss["median_ms"], 4), "fused_to_copy": round(fs["median_ms"] / cs["median_ms"], 4),
                    "fused_range_below_sequence_range": fs["min_max_ms"][1] < ss["min_max_ms"][0],
                    "achieved_tb_per_s": round(moved / fs["median_ms"] / 1e9, 3), "checked": True}

        perm = [full[0]] + full + one   # Z twice: rotated by 1 and by 0
        # 10 words: Z's two readings, a, b, c, sigma1 .. sigma3, X, and dst
        res = {"permutation": leg(perm, PERM_FORMS, PERM_TERMS, PERM_ROT, lambda: perm_sequence(perm), PERM_SEQUENCE, 14, 20, 10)}
        if logn <= 24:
            logup = one + full[:3]
            res["logup"] = leg(logup, LOGUP_FORMS, LOGUP_TERMS, None, lambda: logup_sequence(logup), LOGUP_SEQUENCE, 3, 6, 4)
            num = full[1:7] + [one[0], one[3]]
            res["numerator"] = leg(num, NUM_FORMS, NUM_TERMS, None, lambda: num_sequence(num), NUM_SEQUENCE, 6, 9, 7)
        for d in full + tmp + one + [w]:
            d.free()
        cl.close()
        return res

    res = {"field": "BLS381", "rounds": rounds, "2^24": size_case(24)}
    if large:
        try:
            res["2^27"] = size_case(27)
        except blaze_amd.DriverClientError as e:   # the memory for it (some 110 GiB) is not there: the smaller size stands alone
            res["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_lineval_ops.json"))
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
