#!/usr/bin/env python3
"""What a coset shift costs a 2^27 BLS12-381 transform (blz_ntt_set_coset): kernel-time medians of a
forward and an inverse handle, each toggled between plain and coset, with and without pass 2's per-element factor table; the
wall time of the set_coset call itself (to a shift, to another shift, back to plain); blz_ntt_info bytes before / after.
Writes profiles/ntt_coset_2e27.json.  The device work runs in ONE child process under its own time limit.

    python tools/ntt_coset_timing.py [--out profiles/ntt_coset_2e27.json] [--rounds 9] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(rounds: int) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_ntt import NTT, NTTClient, NTTInput

    logn, g, g2 = 27, 7, 0x1234567890ABCDEF1234567890ABCDEF
    n = 1 << logn
    d_in = DeviceBuffer(0, 32 * n)
    blaze_amd._lib.check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n, 7))
    res = {"log_size": logn, "field": "BLS381", "shift": g, "rounds": rounds}
    for table in (True, False):
        for inverse in (False, True):
            flags = 0 if table else NTTClient.NO_FACTOR_TABLE
            cl = NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, inverse=inverse, flags=flags)
            info0 = cl.info()
            cl.set_data(NTTInput(0, d_in))
            ms = {"plain": [], "coset": []}
            wall = {"to_shift_first": None, "to_shift": [], "to_other_shift": [], "to_plain": []}
            for it in range(rounds + 1):
                for kind in ("plain", "coset"):
                    t0 = time.perf_counter()
                    cl.set_coset(g if kind == "coset" else None)
                    dt = (time.perf_counter() - t0) * 1e3
                    if kind == "coset":
                        if wall["to_shift_first"] is None:
                            wall["to_shift_first"] = dt   # allocates the handle's coset tables
                        else:
                            wall["to_shift"].append(dt)
                    elif it:
                        wall["to_plain"].append(dt)
                    cl.start_process(0)
                    cl.wait_result()
                    if it:
                        ms[kind].append(cl.last_kernel_ms())
            cl.set_coset(g)
            for k in range(3):
                t0 = time.perf_counter()
                cl.set_coset(g2 if k % 2 == 0 else g)
                wall["to_other_shift"].append((time.perf_counter() - t0) * 1e3)
            info1 = cl.info()
            cl.close()
            med = {k: statistics.median(v) for k, v in ms.items()}
            res[("table" if table else "stepped") + ("_inverse" if inverse else "_forward")] = {
                "pass2_factor_table": info0["pass2_factor_table"],
                "kernel_ms_plain": round(med["plain"], 4), "kernel_ms_coset": round(med["coset"], 4),
                "ratio": round(med["coset"] / med["plain"], 4),
                "set_coset_wall_ms": {"first_shift": round(wall["to_shift_first"], 3),
                                      "shift": round(statistics.median(wall["to_shift"]), 3),
                                      "other_shift": round(statistics.median(wall["to_other_shift"]), 3),
                                      "back_to_plain": round(statistics.median(wall["to_plain"]), 3)},
                "device_bytes_before": info0["device_bytes"], "device_bytes_after": info1["device_bytes"],
            }
    d_in.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_coset_2e27.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.rounds)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)],
                       capture_output=True, text=True)
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
