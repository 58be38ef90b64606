#!/usr/bin/env python3
"""What a Poseidon tree costs on the device: kernel-time medians of resident TreeC h = 7 and h = 8 and
TreeD h = 8 on BLS12-381 with tools/poseidon_params.py's t = 9 / 12 blocks of (8, 57) rounds, hashes per second, the definition kernel's time on the same inputs,
blz_calib_mad_rate taken right behind the timed runs, and the issue fraction
    multiply-adds the waves issue (ISA-counted: tests/test_poseidon_isa.py and tests/test_poseidon_sparse_isa.py pin the formulas to
    the code object) / time / that rate.
BOTH round plans are measured in one process, tree by tree: set_round_plan(0) (dense rounds), then set_round_plan(1) (optimised
partial rounds, prepared before the timed runs).  "plan_below_dense_min" says whether the plan's median is below the dense plan's
MINIMUM of the same process: faster by more than the run-to-run spread.
Writes profiles/poseidon_tree_sparse.json (profiles/poseidon_tree.json is the dense-only run of the build before the optimised
rounds existed).  The device work runs in ONE child process under its own time limit.

    python tools/poseidon_timing.py [--out profiles/poseidon_tree_sparse.json] [--rounds 9] [--timeout 300]

--one-tree H: nothing but one TreeC tree of height H whose whole input arrives in ONE set_data call, for a kernel trace - it must show
one launch of the layer kernel per layer, not a batch loop (profiles/poseidon_kernel_stats.txt):
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/poseidon_timing.py --one-tree 6
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
QM = 72   # quotient products of a reduction on BLS12-381 Fr (81 less the 9 by the modulus's lowest limb, which is 1)


RD = 9    # the quotient-digit step (rr_reduce2m)
RF, RP = 8, 57


def wave_mads(t, plan):
    """v_mad_u64_u32 a wave issues for the 64 // t hashes it holds.  Dense: two conversions, and per round the S-box and a matrix
    row of six products per reduction.  Plan: the full rounds with three products per reduction and the quotient-digit step, the
    partial rounds 2 SQR + 2 MUL + that step"""
    mul, sqr = 81 + QM, 45 + QM
    if not plan:
        return 2 * mul + (RF + RP) * (mul + 2 * sqr + 81 * t + QM * ((t + 5) // 6))
    return 2 * mul + RF * (mul + 2 * sqr + 81 * t + QM * ((t + 2) // 3) + RD) + RP * (2 * sqr + 2 * mul + RD)


def lane_mads(h, tree_c, plan):
    total = 0
    for layer in range(0 if tree_c else 1, h):
        n = 8 ** (h - 1 - layer)
        t = 12 if layer == 0 else 9
        hw = 64 // t
        total += -(-n // hw) * wave_mads(t, plan) * 64
    return total


def child(rounds: int) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import buf_ptr, check
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_hash import Hash, PoseidonClient, TreeMode

    import poseidon_params

    wb = b"".join(w.to_bytes(32, "little") for w in poseidon_params.generate("BLS381", [(9, 8, 57), (12, 8, 57)]))
    res = {"field": "BLS381", "rounds_full_partial": [RF, RP], "reps": rounds, "round_forms": ["dense", "plan"]}
    for name, mode, h in (("treec_h7", TreeMode.TreeC, 7), ("treec_h8", TreeMode.TreeC, 8), ("treed_h8", TreeMode.TreeD, 8)):
        tree_c = mode == TreeMode.TreeC
        n_in = (11 if tree_c else 1) * 8 ** (h - 1)
        n_rec = sum(8 ** (h - 1 - layer) for layer in range(0 if tree_c else 1, h))
        d_in = DeviceBuffer(0, 32 * n_in)
        check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n_in, 99 + h))
        cl = PoseidonClient(Hash.Poseidon, DriverClient(0))
        cl.initialize_words(h, mode, wb)
        d_rec = DeviceBuffer(0, 64 * n_rec)
        res[name] = {"hashes": n_rec}
        for form, plan in (("dense", False), ("plan", True)):
            cl.set_round_plan(plan)
            if plan:
                state = cl.prepare_round_plan()
                assert state == {"optimised_partial_rounds": True, "round_plan_check": 1}, state
            assert cl.info()["optimised_partial_rounds"] is plan
            ms = []
            for it in range(rounds + 2):
                cl.set_data(d_in)
                cl.wait_result()
                if it >= 2:
                    ms.append(cl.last_kernel_ms())
                if it < rounds + 1:
                    cl.reset()
            cl.tree_device(d_rec)
            out = (C.c_uint64 * 2)()
            t0 = time.perf_counter()
            check(blaze_amd.aux().blz_test_poseidon_tree_check(0, 1, buf_ptr(wb)[0], len(wb), int(mode), h, d_in.ptr, d_rec.ptr, out))
            def_ms = (time.perf_counter() - t0) * 1e3
            assert out[0] == n_rec and out[1] == 0, list(out)
            cal = (C.c_double * 4)()
            check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
            med = statistics.median(ms)
            mads = lane_mads(h, tree_c, plan)
            res[name][form] = {"kernel_ms": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                               "hashes_per_s": round(n_rec / (med * 1e-3)), "definition_kernel_wall_ms": round(def_ms, 2),
                               "definition_kernel_nodes_checked": int(out[0]),
                               "lane_multiply_adds": mads, "calib_mad_rate": cal[0], "calib_clock_mhz": cal[2],
                               "issue_fraction": round(mads / (med * 1e-3) / cal[0], 4), "device_bytes": cl.info()["device_bytes"]}
        dense, plan = res[name]["dense"], res[name]["plan"]
        res[name]["plan_over_dense"] = round(plan["kernel_ms"] / dense["kernel_ms"], 4)
        res[name]["plan_below_dense_min"] = plan["kernel_ms"] < dense["kernel_ms_min"]
        cl.close()
        d_in.free()
        d_rec.free()
    return res


def one_tree(h: int) -> None:
    import blaze_amd
    import poseidon_params
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import check
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_hash import Hash, PoseidonClient, TreeMode

    n_in = 11 * 8 ** (h - 1)
    d_in = DeviceBuffer(0, 32 * n_in)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n_in, 1))
    cl = PoseidonClient(Hash.Poseidon, DriverClient(0))
    cl.initialize_words(h, TreeMode.TreeC, b"".join(w.to_bytes(32, "little") for w in poseidon_params.generate("BLS381", [(9, 8, 57), (12, 8, 57)])))
    cl.set_data(d_in)
    cl.wait_result()
    n = cl.get_num_of_pending_results()
    print(f"TreeC h = {h}: {n} records pending, {cl.last_kernel_ms():.3f} ms")
    assert n == (8 ** h - 1) // 7
    cl.close()
    d_in.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-tree", type=int, default=0, metavar="H")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_tree_sparse.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.one_tree:
        one_tree(a.one_tree)
        return 0
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
