"""k_accumulate's line gather (msm_impl.hip.hpp acc_lines_issue / acc_lines_read): the BLS kernels fetch every point as one
128-byte line, eight lanes to a line, through a per-wave LDS image.  Every lane of a wave takes part in every load, so the
kernel's control flow is wave-uniform around them: lanes without a unit, lanes whose run has ended and the lanes outside the
affine + affine first addition all go on fetching.  These are the shapes at which that can go wrong, each against the CPU
oracle (bit-exact), at pf = 1 on BLS12-381 and BLS12-377, with small windows forced through BLAZE_MSM_PLAN."""
import numpy as np
import pytest

import blaze_amd
from blaze_amd import DeviceBuffer
from blaze_amd.ingo_msm import Curve, MSMInput, MSMParams
from gpu_util import msm_client, run_msm, synth
from oracle import pyref

CURVES = ["BLS381", "BLS377"]
SIZES = (1, 7, 63, 64, 65, 129, 1000)
# c = 4: 64 windows of 8 buckets, runs of ~n / 8 (cut at L = 256); c = 7, L = 3: every run in units of <= 3, so most buckets
# span several units and the unit list is long; None: the planner's own choice
PLANS = [None, "c=4,L=256", "c=7,L=3", "c=8,L=16"]


def _random_scalars(n, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=32 * n, dtype=np.uint8).reshape(n, 32)
    raw[:, 31] &= 0x0F                            # < 2^252: canonical in both scalar fields
    return raw


def _points(orc, curve, n, seed):
    """n distinct points (the generator's tile is 256 long: longer inputs repeat it, which is a case of its own below)."""
    out = bytearray()
    for k in range(0, n, 256):
        out += orc.input_generator(curve, min(256, n - k), 1, seed + k)[0]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve", CURVES)
def test_sizes_around_a_wave_and_a_block(gpu, orc, curve, plan, monkeypatch):
    """n = 1 ... 1000: fewer units than one wave, waves with idle lanes, a last block that is partly empty - with random scalars
    (distinct points) and with the harness's own input (n = 1000 repeats a 256-point tile: equal points in one bucket)."""
    if plan:
        monkeypatch.setenv("BLAZE_MSM_PLAN", plan)
    cl = msm_client(curve, 1)
    for n in SIZES:
        pts, sc, exp = orc.input_generator(curve, n, 1, 300 + n)
        assert run_msm(cl, pts, sc, n) == exp, f"{curve} {plan} n={n} harness input"
        pts = _points(orc, curve, n, 900 + n)
        sc = _random_scalars(n, n).tobytes()
        assert run_msm(cl, pts, sc, n) == orc.msm_pippenger(curve, pts, sc, n, 1, threads=8), f"{curve} {plan} n={n} random scalars"
    cl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_short_runs_beside_long_ones_in_one_wave(gpu, orc, curve, monkeypatch):
    """Two very common scalars (45 and 70 copies) among unique ones, 8-bit windows: every window has a run of 45 and one of 70
    beside runs of 1, 2 and 3.  Units are ordered by length, 32 of each long kind - half a wave - so the waves that hold them
    also hold shorter ones, and their lanes finish at different steps.  L = 256 keeps the long runs whole; L = 50 cuts the 70s."""
    n = 200
    pts = _points(orc, curve, n, 17)
    raw = _random_scalars(n, 5)
    raw[10:55] = raw[3]
    raw[60:130] = raw[4]
    sc = raw.tobytes()
    exp = orc.msm_pippenger(curve, pts, sc, n, 1, threads=8)
    for plan in ("c=8,L=256", "c=8,L=50"):
        monkeypatch.setenv("BLAZE_MSM_PLAN", plan)
        cl = msm_client(curve, 1)
        assert run_msm(cl, pts, sc, n) == exp, f"{curve} {plan}"
        cl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_all_scalars_equal(gpu, orc, curve, monkeypatch):
    """One bucket per window holds everything: with L = 16 it spans 44 units (the last one short) and k_combine_units folds
    them; n = 700 of distinct points, and of the repeated 256-point tile (P + P inside the runs)."""
    n = 700
    raw = _random_scalars(n, 9)
    raw[:] = raw[0]
    sc = raw.tobytes()
    monkeypatch.setenv("BLAZE_MSM_PLAN", "c=8,L=16")
    cl = msm_client(curve, 1)
    for pts in (_points(orc, curve, n, 23), orc.input_generator(curve, n, 1, 24)[0]):
        assert run_msm(cl, pts, sc, n) == orc.msm_pippenger(curve, pts, sc, n, 1, threads=8), curve
    cl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_equal_and_opposite_points(gpu, orc, curve, monkeypatch):
    """P + P and P - P in the affine + affine first addition and in the mixed addition, and the restart from infinity: groups
    of points that share a scalar (so a bucket), each group a different arrangement of a point, its copy and its negation."""
    q, fb = pyref.CURVES[curve]["q"], pyref.CURVES[curve]["fq_bytes"]
    base = _points(orc, curve, 12, 31)
    P = [bytes(base[2 * fb * i: 2 * fb * (i + 1)]) for i in range(12)]

    def neg(p):
        return p[:fb] + (q - int.from_bytes(p[fb:], "little")).to_bytes(fb, "little")

    groups = [
        [P[0], P[0]],                              # first addition doubles
        [P[1], neg(P[1])],                         # first addition gives infinity, which is the run's sum
        [P[2], neg(P[2]), P[3]],                   # ... restart from infinity
        [P[4], neg(P[4]), P[5], P[5]],             # ... and double in the mixed addition
        [P[6], P[6], P[6], P[6]],
        [P[7], P[8], neg(P[7]), neg(P[8])],        # the sum cancels in the mixed addition
        [P[9], P[9], neg(P[9]), neg(P[9]), P[10]],
        [P[11]],
    ]
    scal = _random_scalars(len(groups), 77)
    pts = b"".join(p for g in groups for p in g)
    sc = b"".join(scal[i].tobytes() * len(g) for i, g in enumerate(groups))
    n = sum(len(g) for g in groups)
    exp = orc.msm_pippenger(curve, pts, sc, n, 1, threads=1)
    for plan in ("c=8,L=256", "c=8,L=2", None):
        if plan:
            monkeypatch.setenv("BLAZE_MSM_PLAN", plan)
        else:
            monkeypatch.delenv("BLAZE_MSM_PLAN", raising=False)
        cl = msm_client(curve, 1)
        assert run_msm(cl, pts, sc, n) == exp, f"{curve} {plan}"
        cl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_task_in_three_pieces(gpu, orc, curve, monkeypatch):
    """k_accumulate_cont: the first piece starts its runs with the affine + affine addition (`first`), the others resume from the
    bucket sums - both through the image.  Random scalars, and the common-scalar mix whose long runs span several units."""
    monkeypatch.setenv("BLAZE_MSM_PIECES", "3")
    for n, plan in ((1000, "c=8,L=256"), (1000, "c=4,L=16"), (4000, None)):
        if plan:
            monkeypatch.setenv("BLAZE_MSM_PLAN", plan)
        else:
            monkeypatch.delenv("BLAZE_MSM_PLAN", raising=False)
        pts = _points(orc, curve, n, 41)
        raw = _random_scalars(n, 43)
        raw[100:400] = raw[7]
        for sc in (_random_scalars(n, 42).tobytes(), raw.tobytes()):
            cl = msm_client(curve, 1)
            assert run_msm(cl, pts, sc, n) == orc.msm_pippenger(curve, pts, sc, n, 1, threads=8), f"{curve} n={n} {plan}"
            cl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_two_tasks_in_flight_with_the_three_level_sort(gpu, orc, curve, monkeypatch):
    """BLAZE_SORT_HIDE=2 at 2^16: the three-level sort of one task runs while the other task's accumulation holds its LDS images.
    Results in flight == results one task at a time == the oracle's (linearity over P_i = (i + 1) G)."""
    monkeypatch.setenv("BLAZE_SORT_HIDE", "2")
    n = 1 << 16
    dp, ds0 = synth(curve, n, seed=31)
    ds1 = DeviceBuffer(0, n * 32)
    blaze_amd._lib.check(blaze_amd.aux().blz_synth_scalars(0, int(Curve[curve]), ds1.ptr, n, 32))
    exp = []
    for d in (ds0, ds1):
        k = orc.index_weighted_sum(curve, d.download(), n, 0, threads=8)
        exp.append(orc.result_from_affine(curve, orc.generator_mul(curve, k)))
    params = MSMParams(n, None)
    cl = msm_client(curve, 1)
    alone = [run_msm(cl, dp, d, n) for d in (ds0, ds1)]
    order = [0, 1, 1, 0, 1, 0]
    got = []
    for k, which in enumerate(order):
        cl.initialize(params); cl.start_process(); cl.set_data(MSMInput(dp, (ds0, ds1)[which], params))
        if k >= 1:
            cl.wait_result(); got.append(cl.result().result)
    cl.wait_result(); got.append(cl.result().result)
    cl.close()
    for b in (dp, ds0, ds1):
        b.free()
    assert alone == exp
    assert got == [alone[w] for w in order]


def test_sort_fit_counts_lds():
    """MsmEngine::begin() hides a sort only if one of its blocks fits on a CU BESIDE the accumulation's: two accumulation waves per
    SIMD at 200 VGPRs are four blocks of 128 lanes per CU, and with the line gather each holds a 16 KiB image - 64 of the CU's
    160 KiB.  A sort block gets what is left, 96 KiB, and not a KiB more (the level-1 scatter took 123 KiB before it was cut to
    83); the register term is what it was, and a count that is not known fits, as before."""
    fits = blaze_amd.aux().blz_test_sort_fits_beside
    KiB = 1024
    assert fits(200, 72, 16 * KiB, 83 * KiB) == 1
    assert fits(200, 72, 16 * KiB, 96 * KiB) == 1
    assert fits(200, 72, 16 * KiB, 96 * KiB + 1) == 0
    assert fits(200, 72, 16 * KiB, 123 * KiB) == 0          # the level-1 scatter with 12 scalars per lane
    assert fits(194, 72, 16 * KiB, 96 * KiB) == 1           # (registers are allocated in eights: still two waves)
    assert fits(200, 72, 24 * KiB, 64 * KiB) == 1 and fits(200, 72, 24 * KiB, 65 * KiB) == 0
    # three accumulation waves per SIMD (136 registers) are six blocks
    assert fits(136, 72, 16 * KiB, 64 * KiB) == 1 and fits(136, 72, 16 * KiB, 65 * KiB) == 0
    # an accumulation without LDS leaves all of it; the register term alone decides, as it always did
    assert fits(200, 72, 0, 123 * KiB) == 1
    assert fits(200, 80, 0, 123 * KiB) == 1 and fits(208, 72, 0, 0) == 0 and fits(200, 88, 16 * KiB, 8 * KiB) == 0
    # counts that could not be read
    assert fits(0, 72, 16 * KiB, 200 * KiB) == 1 and fits(200, 72, -1, 200 * KiB) == 1 and fits(200, 72, 16 * KiB, 0) == 1
