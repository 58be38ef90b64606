#!/usr/bin/env python3
"""What the one-call fraction GKR (logUp-GKR) costs over the BLS12-381 scalar field (blz_ntt_gkr_prove_frac; DESIGN.md section 4,
"One-call fraction GKR"): medians with min - max, the three legs alternating in the same process, at m = 24, 20 and 16 (2^m
fractions).
    fused     blz_ntt_gkr_prove_frac, one blz_ntt_wait_result: the rounds at live lengths of 256 and below inside one block;
    unfused   the same call with BLZ_GKR_UNFUSED: the chain of the existing launches alone;
    caller    what a caller can do without the op.  Per layer: blz_ntt_fs_challenge with count 0 for lambda, blz_ntt_gate_eval for
              T = P_hi + lambda Q_hi over P_hi, blz_ntt_vec_mle_eq over the point, ONE blz_ntt_sumcheck_prove over views of the
              layer's four tables, blz_ntt_wait_result, the download of the four final words and of lambda, P_hi_f = T_f - lambda
              Q_hi_f on the host, the upload of the four claims side by side, blz_ntt_fs_challenge over them, and the point of the
              next layer turned round on the host and uploaded.
    wall time of each (host clock, from the first call to the last wait) and kernel time - blz_ntt_last_kernel_ms of the one
    call, the sum over the ops for the caller's leg - with blz_ntt_mle_tree(BLZ_TREE_FRAC)'s own time beside them.
The trees and the leaves are restored from pristine copies before each run (not timed).  The outputs of the three legs - rounds,
points, claims, lambdas and the final state - are compared byte for byte and verified (blaze_amd.gkr.verify_fraction) before
anything is timed.
Writes profiles/ntt_gkr_frac.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_gkr_frac_timing.py [--out profiles/ntt_gkr_frac.json] [--rounds 9] [--timeout 900] [--sizes 24,20,16]
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

FIELD = "BLS381"
TERMS = [(1, [0, 3]), (1, [2, 1])]   # P_lo Q_hi + Q_lo T over [P_lo, T, Q_lo, Q_hi]
T_TERMS = [(1, [0]), (1, [1, 2])]    # P_hi + lambda Q_hi over [P_hi, lambda, Q_hi]
TAIL_LOG = 8                         # FGKR_TAIL_LOG


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def child(rounds: int, sizes) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer, fiat_shamir, gkr
    from blaze_amd._lib import check, lib
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_ntt import NTT, NTTClient

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def hip_ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")

    dc = DriverClient(0)
    r = fiat_shamir.MODULUS[FIELD]

    def whole(m):
        n = 1 << m
        lay = gkr.layout_frac(m)
        cl = NTTClient(NTT.Ntt, dc, log_size=m, flags=NTTClient.NO_FACTOR_TABLE)
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        rng = random.Random(900 + m)
        src = [DeviceBuffer(0, 32 * n) for _ in range(4)]   # tree_p, tree_q, a_p, a_q
        check(blaze_amd.aux().blz_synth_field_elements(0, src[2].ptr, n, 311))
        check(blaze_amd.aux().blz_synth_field_elements(0, src[3].ptr, n, 312))
        tree_ms = []
        for it in range(rounds + 2):
            cl.mle_tree(src[0], src[2], NTTClient.TREE_FRAC, dst_q=src[1], a_q=src[3])
            cl.wait_result()
            if it >= 2:
                tree_ms.append(cl.last_kernel_ms())
        ops = [DeviceBuffer(0, 32 * n) for _ in range(4)]
        state0 = rng.randbytes(32)
        d_state, d_w = DeviceBuffer(0, 32), DeviceBuffer(0, 32 * lay.weight_words)
        d_rounds, d_points, d_claims, d_lambdas = (DeviceBuffer(0, 32 * max(w, 1)) for w in (lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words))
        d_chal, d_four, d_rho = DeviceBuffer(0, 32 * m), DeviceBuffer(0, 128), DeviceBuffer(0, 32)

        def restore():
            for t, s in zip(ops, src):
                hip_ok(hip.hipMemcpyAsync(t.ptr, s.ptr, s.nbytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            d_state.upload(state0)
            for d in (d_rounds, d_points, d_claims, d_lambdas):
                d.upload(bytes(d.nbytes))

        def outputs():
            return tuple(bytes(d.download()) for d in (d_rounds, d_points, d_claims, d_lambdas, d_state))

        def one_call(fused):
            t0 = time.perf_counter()
            cl.gkr_prove_frac(*ops, d_state, weight=d_w, rounds=d_rounds, points=d_points, claims=d_claims, lambdas=d_lambdas, fused=fused)
            cl.wait_result()
            wall = (time.perf_counter() - t0) * 1e3
            return wall, cl.last_kernel_ms()

        def caller():
            dev_ms = 0.0

            def done():
                nonlocal dev_ms
                cl.wait_result()
                dev_ms += cl.last_kernel_ms()

            t0 = time.perf_counter()
            for j in range(m):
                k = m - 1 - j
                off = 0 if k == 0 else NTTClient.tree_layer(n, k)[0]
                bp, bq = (ops[2], ops[3]) if k == 0 else (ops[0], ops[1])
                h = 32 << j
                plo, phi, qlo, qhi = bp.view(32 * off, h), bp.view(32 * off + h, h), bq.view(32 * off, h), bq.view(32 * off + h, h)
                z = b""
                if j >= 1:
                    d_lam = d_lambdas.view(32 * j, 32)
                    cl.fs_challenge(d_state, None, 0, r=d_lam)
                    done()
                    cl.gate_eval(phi, [phi, d_lam, qhi], T_TERMS, length=1 << j)
                    done()
                    cl.vec_mle_eq(d_w, d_points.view(32 * lay.points[j - 1], 32 * j), j - 1)
                    done()
                    cl.sumcheck_prove([plo, phi, qlo, qhi], TERMS, d_state, weight=d_w.view(0, 16 << j), points=3, length=1 << j,
                                      rounds=d_rounds.view(32 * lay.rounds[j], 96 * j), challenges=d_chal)
                    done()
                    z = bytes(d_chal.download(32 * j))
                    f = [int.from_bytes(bytes(t.download(32)), "little") for t in (plo, phi, qlo, qhi)]
                    lam = int.from_bytes(bytes(d_lam.download()), "little")
                    f[1] = (f[1] - lam * f[3]) % r
                    four = b"".join(v.to_bytes(32, "little") for v in f)
                else:
                    four = b"".join(bytes(t.download(32)) for t in (plo, phi, qlo, qhi))
                d_four.upload(four)
                d_claims.view(32 * lay.claims[j], 128).upload(four)
                cl.fs_challenge(d_state, d_four, count=4, r=d_rho)
                done()
                row = b"".join(z[32 * i:32 * (i + 1)] for i in reversed(range(j))) + bytes(d_rho.download())
                d_points.view(32 * lay.points[j], 32 * (j + 1)).upload(row)
            wall = (time.perf_counter() - t0) * 1e3
            return wall, dev_ms

        # the check, before anything is timed
        got = {}
        for leg, run in (("fused", lambda: one_call(True)), ("unfused", lambda: one_call(False)), ("caller", caller)):
            restore()
            run()
            got[leg] = outputs()
        if not got["fused"] == got["unfused"] == got["caller"]:
            raise RuntimeError(f"m = {m}: the legs differ in the rounds, the points, the claims, the lambdas or the final state")
        roots = [int.from_bytes(bytes(src[w].view(32 * (n - 2), 32).download()), "little") for w in (0, 1)]
        final, _, _ = gkr.verify_fraction(FIELD, m, roots[0], roots[1], state0, *got["fused"][:4])
        if final != got["fused"][4] or not any(got["fused"][0][-96:]) or got["fused"][4] == state0:
            raise RuntimeError(f"m = {m}: degenerate check")

        res = {leg: ([], []) for leg in ("fused", "unfused", "caller")}
        for it in range(rounds + 2):   # two warm-up rounds; the legs alternate
            for leg, run in (("fused", lambda: one_call(True)), ("unfused", lambda: one_call(False)), ("caller", caller)):
                restore()
                wall, kern = run()
                if it >= 2:
                    res[leg][0].append(wall)
                    res[leg][1].append(kern)
        for d in src + ops + [d_state, d_w, d_rounds, d_points, d_claims, d_lambdas, d_chal, d_four, d_rho]:
            d.free()
        cl.close()
        out = {leg: {"wall": stats(res[leg][0]), "kernel" if leg != "caller" else "kernel_sum": stats(res[leg][1])} for leg in res}
        out.update({
            "variables": m, "layers": m, "sumcheck_rounds": m * (m - 1) // 2,
            "rounds_inside_the_block": m * (m - 1) // 2 - sum(j - TAIL_LOG for j in range(TAIL_LOG + 1, m)),
            "launches_of_k_fgkr_tail": 1 + max(m - 1 - TAIL_LOG, 0),
            "mle_tree_frac": stats(tree_ms),
            "wall_fused_to_caller": round(out["fused"]["wall"]["median_ms"] / out["caller"]["wall"]["median_ms"], 4),
            "wall_fused_to_unfused": round(out["fused"]["wall"]["median_ms"] / out["unfused"]["wall"]["median_ms"], 4),
            "kernel_fused_to_unfused": round(out["fused"]["kernel"]["median_ms"] / out["unfused"]["kernel"]["median_ms"], 4),
            "fused_wall_range_wholly_below_caller": out["fused"]["wall"]["min_max_ms"][1] < out["caller"]["wall"]["min_max_ms"][0],
            "fused_wall_range_wholly_below_unfused": out["fused"]["wall"]["min_max_ms"][1] < out["unfused"]["wall"]["min_max_ms"][0],
            "checked": True})
        return out

    res = {"field": FIELD, "rounds": rounds, "tail_len": 1 << TAIL_LOG, "fraction_sum": {}}
    for m in sizes:
        res["fraction_sum"][f"m={m}"] = whole(m)
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_gkr_frac.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--sizes", default="24,20,16", help="log2 of the numbers of fractions, largest first")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child:
        print("RESULT " + json.dumps(child(a.rounds, sizes)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds),
                        "--sizes", a.sizes], capture_output=True, text=True)
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
