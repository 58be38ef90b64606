"""Which kernels an MSM task launches, shape by shape: runs the shapes of tests/test_gpu_msm.py::test_every_tail_schedule_is_served
and a few more (STEP_SHAPES; BURST_SHAPES, two tasks in flight) once each (one task at a time otherwise, an empty task - k_emit_infinity - in front of every shape as a separator) so that a kernel trace of
the run can be cut into per-shape launch sequences and two builds of the library (BLAZE_HIP_LIB) compared:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/msm_tail_trace.py          (a run of its own, no counters)
    python3 tools/msm_tail_trace.py --listing OUT > listing.txt                                     (kernel, grid, block per shape)

Launch sequences do not depend on the data (every grid is sized by the plan's bounds), so the inputs are the curve's generator
repeated and random scalars; the results are printed to be compared between the builds, the GPU test checks them against the oracle."""
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (curve, precompute factor, elements, BLAZE_MSM_PLAN, BLAZE_MSM_PIECES)
SHAPES = [
    ("BLS381", 1, 16, None, None),
    ("BLS381", 1, 1 << 12, None, None),
    ("BLS377", 1, 1 << 12, None, None),
    ("BLS381", 1, 1 << 12, None, "3"),
    ("BLS381", 1, 1 << 17, None, None),
    ("BLS381", 8, 1 << 16, None, None),
    ("BLS381", 1, 1 << 13, "c=18", None),
    ("BN254", 1, 1 << 10, None, None),
    ("BN254", 1, 1 << 16, None, None),
    ("BN254", 1, 1 << 14, "c=18", None),
    ("BN254", 8, 1 << 9, None, None),
]
# ... and beside that mirror, the shapes whose launches depend on which sort buffers and which stream a step is given (MsmEngine::step()):
# a lone piecewise task that sorts each piece underneath the accumulation of the one before (ping-pong over both slots' buffers,
# tests/test_gpu_msm.py::test_lone_piecewise_task_sorts_under_its_own_accumulation), and the one-block sort stage of a tiny task
STEP_SHAPES = [
    ("BLS381", 1, 5000, "c=15", "3"),
    ("BLS381", 1, 16, None, None),
]
# ... and a shape run as TWO tasks in flight: the second one's sort stage goes to the sort stream, underneath the first one's
# accumulation ("s3 hidden" of plan_sort(); the first sorts in the open).  c = 15: the smallest forced plan the three-level sort accepts
BURST_SHAPES = [
    ("BLS381", 1, 5000, "c=15", None),
]
ALL_SHAPES = SHAPES + STEP_SHAPES + BURST_SHAPES
MARKER = "k_emit_infinity"


def run_shapes():
    import numpy as np

    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_msm import Curve, MSMClient, MSMInit, MSMInput, MSMParams, PointMemoryType

    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))
    dc = DriverClient(0)
    rng = np.random.default_rng(2024)

    def submit(cl, pts, sc, n):
        p = MSMParams(n, None)
        cl.initialize(p)
        cl.start_process()
        cl.set_data(MSMInput(pts, sc, p))

    def collect(cl):
        cl.wait_result()
        return bytes(cl.result().result)

    for k, (curve, pf, n, plan, pieces) in enumerate(ALL_SHAPES):
        in_flight = 2 if k >= len(SHAPES) + len(STEP_SHAPES) else 1
        for key, val in (("BLAZE_MSM_PLAN", plan), ("BLAZE_MSM_PIECES", pieces)):
            os.environ.pop(key, None)
            if val:
                os.environ[key] = val
        fb = 32 if curve == "BN254" else 48
        g = int(kat[f"{curve}_G_x"], 16).to_bytes(fb, "little") + int(kat[f"{curve}_G_y"], 16).to_bytes(fb, "little")
        sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sc[:, 31] &= 0x0F                                   # < 2^252: canonical in all three scalar fields
        cl = MSMClient(MSMInit(PointMemoryType.DMA, pf == 8, Curve[curve]), dc)
        submit(cl, b"", b"", 0)                             # the separator
        collect(cl)
        for _ in range(in_flight):
            submit(cl, g * (n * pf), sc.tobytes(), n)
        res = b"".join(collect(cl) for _ in range(in_flight))
        print(f"{curve} pf={pf} n={n} plan={plan} pieces={pieces}: result sha256 {hashlib.sha256(res).hexdigest()[:16]}", flush=True)
        cl.close()


def listing(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path, newline="")))
    assert rows, f"no *kernel_trace.csv under {out_dir}"
    order = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))

    def dims(r, what):
        return "x".join(r[f"{what}_{a}"] for a in "XYZ" if f"{what}_{a}" in r)

    shape = -1
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            shape += 1
            print("== shape %d: %s pf=%d n=%d plan=%s pieces=%s" % ((shape,) + ALL_SHAPES[shape]))
        elif shape >= 0:
            print(f"{name.split('(')[0]}  grid {dims(r, 'Grid_Size')}  block {dims(r, 'Workgroup_Size')}")
    assert shape + 1 == len(ALL_SHAPES), f"{shape + 1} separators for {len(ALL_SHAPES)} shapes"


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--listing":
        listing(sys.argv[2])
    else:
        run_shapes()
