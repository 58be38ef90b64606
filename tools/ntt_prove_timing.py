#!/usr/bin/env python3
"""What the one-call prover saves over the BLS12-381 scalar field (blz_ntt_sumcheck_prove, blz_ntt_fs_challenge; DESIGN.md
section 4, "One-call prover"): medians with min - max, the two sides alternating in the same process.
    one call against the host loop: the R1CS zerocheck W (Az Bz - Cz), 3 points, at m = 24, 20 and 16 variables.
        one call   blz_ntt_sumcheck_prove, one blz_ntt_wait_result, one download of the m x 3 round words;
        host loop  the same m + 2 single ops with, between any two, blz_ntt_wait_result, the download of the round, hashlib
                   (blaze_amd.fiat_shamir), the upload of the challenge into a device word that is reused.
        wall time of each (host clock, ending in a device synchronise) and kernel time - blz_ntt_last_kernel_ms of the chain,
        the sum of the m + 2 ops' for the loop.  The weight is a real equality table (blz_ntt_vec_mle_eq, not timed), the tables
        random field elements; tables, weight and state are restored from pristine copies before each run (not timed).
    the transcript kernel alone: blz_ntt_last_kernel_ms around ONE blz_ntt_fs_challenge at count = 3 and 6 - one and two absorbed
        blocks.  It is the time between two events around one launch of one wave, the events' own cost included.
    per-round overhead of the chain: (chain kernel time - the loop's summed kernel time) / m, beside the loop's per-round host
        cost (its wall time - its kernel time) / m.
The outputs are checked against each other before anything is timed: rounds, challenges and the final state, byte for byte.
Writes profiles/ntt_prove.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_prove_timing.py [--out profiles/ntt_prove.json] [--rounds 9] [--timeout 900] [--sizes 24,20,16]
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
TERMS = [(1, [0, 1]), (-1, [2])]   # Az Bz - Cz over [Az, Bz, Cz]
POINTS = 3


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def child(rounds: int, sizes) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer, fiat_shamir
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

    def stream_of(cl):
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        return stream

    def whole(m):
        n = 1 << m
        cl = NTTClient(NTT.Ntt, dc, log_size=m, flags=NTTClient.NO_FACTOR_TABLE)
        stream = stream_of(cl)
        rng = random.Random(700 + m)
        point = DeviceBuffer(0, 32 * m)
        point.upload(rng.randbytes(32 * m))
        src = [DeviceBuffer(0, 32 * n) for _ in range(3)]
        for i, d in enumerate(src):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 195 + i))
        src_w = DeviceBuffer(0, 16 * n)
        cl.vec_mle_eq(src_w, point, m - 1)
        cl.wait_result()
        tabs = [DeviceBuffer(0, 32 * n) for _ in range(3)]
        d_w = DeviceBuffer(0, 16 * n)
        state0 = rng.randbytes(32)
        d_state, d_rounds, d_chal = DeviceBuffer(0, 32), DeviceBuffer(0, 32 * m * POINTS), DeviceBuffer(0, 32 * m)
        out, d_c = DeviceBuffer(0, 32 * POINTS), DeviceBuffer(0, 32)

        def restore():
            for t, s in zip(tabs + [d_w], src + [src_w]):
                hip_ok(hip.hipMemcpyAsync(t.ptr, s.ptr, s.nbytes, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            d_state.upload(state0)

        def one_call():
            t0 = time.perf_counter()
            cl.sumcheck_prove(tabs, TERMS, d_state, weight=d_w, points=POINTS, length=n, rounds=d_rounds, challenges=d_chal)
            cl.wait_result()
            sent = bytes(d_rounds.download())
            wall = (time.perf_counter() - t0) * 1e3
            return wall, cl.last_kernel_ms(), sent

        def host_loop():
            dev_ms, rows, state = 0.0, [], state0
            t0 = time.perf_counter()
            for i in range(m + 1):
                if i == 0:
                    cl.zerocheck_gate(tabs, TERMS, d_w, points=POINTS, length=n, out=out)
                elif i < m:
                    cl.zerocheck_gate(tabs, TERMS, d_w, r=d_c, points=POINTS, length=n >> (i - 1), out=out)
                else:
                    cl.sumcheck_gate(tabs, TERMS, None, r=d_c, points=0, length=2)
                cl.wait_result()
                dev_ms += cl.last_kernel_ms()
                if i < m:
                    row = bytes(out.download())
                    rows.append(row)
                    state, x = fiat_shamir.absorb(state, row, FIELD)
                    d_c.upload(x.to_bytes(32, "little"))
            wall = (time.perf_counter() - t0) * 1e3
            return wall, dev_ms, b"".join(rows), state

        # the check, before anything is timed
        restore()
        _, _, sent = one_call()
        got = (sent, bytes(d_chal.download()), bytes(d_state.download()))
        restore()
        _, _, rows, state = host_loop()
        chal = fiat_shamir.challenges(state0, [rows[96 * i:96 * (i + 1)] for i in range(m)], FIELD)[1]
        if got != (rows, b"".join(x.to_bytes(32, "little") for x in chal), state):
            raise RuntimeError(f"m = {m}: the one call and the host loop differ in the rounds, the challenges or the final state")
        if not any(rows[-96:]) or len(set(chal)) != m:
            raise RuntimeError(f"m = {m}: degenerate check")

        res = {"one": ([], []), "loop": ([], [])}
        for it in range(rounds + 2):   # two warm-up rounds; the sides alternate
            restore()
            a = one_call()
            restore()
            b = host_loop()
            if it >= 2:
                res["one"][0].append(a[0]); res["one"][1].append(a[1])
                res["loop"][0].append(b[0]); res["loop"][1].append(b[1])
        for d in src + tabs + [src_w, d_w, d_state, d_rounds, d_chal, out, d_c, point]:
            d.free()
        cl.close()
        ow, ok, lw, lk = stats(res["one"][0]), stats(res["one"][1]), stats(res["loop"][0]), stats(res["loop"][1])
        return {"variables": m, "launch_chain": f"{m + 2} step ops + {m} transcript steps", "one_call": {"wall": ow, "kernel": ok},
                "host_loop": {"wall": lw, "kernel_sum": lk}, "wall_one_to_loop": round(ow["median_ms"] / lw["median_ms"], 4),
                "one_call_wall_range_wholly_below_loop": ow["min_max_ms"][1] < lw["min_max_ms"][0],
                "chain_kernel_minus_loop_kernel_sum_ms": round(ok["median_ms"] - lk["median_ms"], 4),
                "chain_overhead_per_round_us": round((ok["median_ms"] - lk["median_ms"]) * 1e3 / m, 3),
                "loop_host_cost_per_round_us": round((lw["median_ms"] - lk["median_ms"]) * 1e3 / m, 3), "checked": True}

    def transcript_alone():
        cl = NTTClient(NTT.Ntt, dc, log_size=4, flags=NTTClient.NO_FACTOR_TABLE)
        rng = random.Random(9)
        raw = rng.randbytes(32 * 8)
        words, d_state, d_r = DeviceBuffer(0, 32 * 8), DeviceBuffer(0, 32), DeviceBuffer(0, 32)
        words.upload(raw)
        res = {}
        for count in (3, 6):
            state = rng.randbytes(32)
            d_state.upload(state)
            ms = []
            for it in range(rounds + 2):
                cl.fs_challenge(d_state, words, count=count, r=d_r)
                cl.wait_result()
                state, x = fiat_shamir.absorb(state, raw[:32 * count], FIELD)
                if bytes(d_state.download()) != state or bytes(d_r.download()) != x.to_bytes(32, "little"):
                    raise RuntimeError(f"transcript step at count {count}: the device and hashlib differ")
                if it >= 2:
                    ms.append(cl.last_kernel_ms())
            res[f"count_{count}"] = dict(stats(ms), absorbed_blocks=4 * (1 + count) // 17 + 1)
        for d in (words, d_state, d_r):
            d.free()
        cl.close()
        return res

    res = {"field": FIELD, "rounds": rounds, "gate": "W (Az Bz - Cz), 3 points", "whole_r1cs_zerocheck": {}}
    res["transcript_step_alone"] = transcript_alone()
    fs3 = res["transcript_step_alone"]["count_3"]["median_ms"]
    for m in sizes:
        case = whole(m)
        # what the m transcript launches account for: m times the step alone, measured above in this process
        case["transcript_launches_account_for_ms"] = round(m * fs3, 4)
        case["kernel_excess_within_the_transcript_launches"] = case["chain_kernel_minus_loop_kernel_sum_ms"] <= m * fs3
        res["whole_r1cs_zerocheck"][f"m={m}"] = case
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_prove.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--sizes", default="24,20,16", help="the numbers of variables, largest first")
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
