"""Resident-base window tables by default (csrc/arena_tables.hip, the auto policy): a pf = 1 HBM handle whose table mode was
never set gets the table of its bases once the SECOND scalars-only task in a row runs over the identical bases and scalar range
with no write in between - built at once on the handle's stream ahead of that task, adopted by the first task launched after
the build is through - within a size threshold (BLAZE_MSM_PLAN auto_table_min, 2^24 by default; 1 here) and a memory budget,
and gives the memory back when an allocation of the library fails.  Every result below is compared with the CPU oracle AND
with the bytes of a handle that switched tables off (set_window_table(0))."""
import pytest

import blaze_amd
from blaze_amd import DeviceBuffer
from blaze_amd.ingo_msm import MSMInput, MSMParams, PointMemoryType
from gpu_util import msm_client, run_msm, synth
from oracle import pyref

pytestmark = pytest.mark.gpu
ADDR = 0x100000
TINY = "auto_table_min=1"
_CACHE = {}


def _release():
    blaze_amd._lib.check(blaze_amd.lib().blz_arena_release(0))


def _tables(cl):
    return cl.memory_info()["arena_window_tables"]


def _inputs(orc, curve, n, pf=1):
    """Bases and three scalar sets with their expected results, computed once per shape.  pf = 1: base 7 repeats base 3 and
    base 9 is its negative, all three under one scalar (a doubling and a cancellation inside one bucket, on table rows once
    the table serves them); set 0 carries scalars >= r up to 2^256 - 1 (the top window absorbs the last digit carry)."""
    key = (curve, n, pf)
    if key in _CACHE:
        return _CACHE[key]
    pts, sc, _ = orc.input_generator(curve, n, pf, 7000 + n)
    pts, sc = bytearray(pts), bytearray(sc)
    fb, q, r = pyref.CURVES[curve]["fq_bytes"], pyref.CURVES[curve]["q"], pyref.CURVES[curve]["r"]
    ps = 2 * fb
    if pf == 1:
        pts[ps * 7: ps * 8] = pts[ps * 3: ps * 4]
        y = int.from_bytes(pts[ps * 3 + fb: ps * 4], "little")
        pts[ps * 9: ps * 10] = pts[ps * 3: ps * 3 + fb] + ((q - y) % q).to_bytes(fb, "little")
        sc[32 * 7: 32 * 8] = sc[32 * 3: 32 * 4]
        sc[32 * 9: 32 * 10] = sc[32 * 3: 32 * 4]
        for i, v in enumerate([(1 << 256) - 1, (1 << 256) - 2, 1 << 255]):
            sc[32 * i: 32 * i + 32] = v.to_bytes(32, "little")
        for i, v in enumerate([r, r + 1, r - 1, 0, 1]):
            sc[32 * (20 + i): 32 * (21 + i)] = v.to_bytes(32, "little")
    sets = [bytes(sc), bytes(sc[32 * 11:]) + bytes(sc[:32 * 11]), bytes(sc[32 * 100:]) + bytes(sc[:32 * 100])]
    exp = [orc.msm_pippenger(curve, bytes(pts), s, n, pf, threads=8) for s in sets]
    _CACHE[key] = (bytes(pts), sets, exp)
    return _CACHE[key]


def _masked(sc, n, lo, hi):
    out = bytearray(len(sc))
    mask = ((1 << (hi - lo)) - 1) << lo
    for i in range(n):
        v = int.from_bytes(sc[32 * i: 32 * i + 32], "little") & mask
        out[32 * i: 32 * i + 32] = v.to_bytes(32, "little")
    return bytes(out)


def _off_client(curve, pf=1):
    off = msm_client(curve, pf, PointMemoryType.HBM)
    if pf == 1:
        off.set_window_table(0)
    return off


@pytest.mark.parametrize("curve,n", [("BLS381", 257), ("BLS381", 8192), ("BLS377", 257), ("BLS377", 8192)])
def test_second_task_builds_third_task_adopts(gpu, orc, curve, n, monkeypatch):
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    pts, sets, exp = _inputs(orc, curve, n)
    _release()
    cl, off = msm_client(curve, 1, PointMemoryType.HBM), _off_client(curve)
    cl.load_data_to_hbm(pts, ADDR, 0)
    for k in range(3):
        got = run_msm(cl, None, sets[k], n, hbm=(ADDR, 0))
        info = cl.window_table_info()
        assert got == exp[k], f"{curve} n={n} task {k + 1}"
        assert run_msm(off, None, sets[k], n, hbm=(ADDR, 0)) == got and off.window_table_info()["bytes"] == 0
        if k < 2:
            assert info["bytes"] == 0, (k, info)       # task 1: no evidence yet; task 2 starts the build and takes the plain path
        else:
            assert info["bytes"] > 0 and info["windows"] * info["window_bits"] >= 257, info
    assert _tables(cl) >= cl.window_table_info()["bytes"] > 0
    # ... and it stays: the first scalar set again, from the table
    assert run_msm(cl, None, sets[0], n, hbm=(ADDR, 0)) == exp[0] and cl.window_table_info()["bytes"] > 0
    cl.close(); off.close()
    _release()


NO_TRIGGER = ["one_task", "rewrite_between", "sub_ranges", "scalar_ranges", "bn254", "pf8", "dma_handle", "explicit_off", "process_off",
              "below_threshold"]


@pytest.mark.parametrize("case", NO_TRIGGER)
def test_no_trigger(gpu, orc, case, monkeypatch):
    """What must NOT start a build: arena_window_tables stays 0 and no task reports a table."""
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY + ",auto_table=0" if case == "process_off" else TINY)
    if case == "below_threshold":
        monkeypatch.delenv("BLAZE_MSM_PLAN")
    curve = "BN254" if case == "bn254" else "BLS381"
    pf = 8 if case == "pf8" else 1
    n = 1024 if pf == 8 else 8192
    pts, sets, exp = _inputs(orc, curve, n, pf)
    ps = 2 * pyref.CURVES[curve]["fq_bytes"]
    _release()
    cl = msm_client(curve, pf, PointMemoryType.DMA if case == "dma_handle" else PointMemoryType.HBM)
    off = _off_client(curve, pf)
    cl.load_data_to_hbm(pts, ADDR, 0)
    if case == "explicit_off":
        cl.set_window_table(0)

    def task(k, sc=None, want=None, m=n, off_bytes=0):
        sc, want = sets[k] if sc is None else sc, exp[k] if want is None else want
        got = run_msm(cl, None, sc, m, hbm=(ADDR, off_bytes))
        assert got == want, f"{case} task {k}"
        assert cl.window_table_info()["bytes"] == 0 and _tables(cl) == 0, f"{case} task {k}"
        return got

    if case == "one_task":
        task(0)
    elif case == "rewrite_between":
        for k in range(3):
            task(k)
            cl.load_data_to_hbm(pts, ADDR, 0)      # the same bytes: a write all the same (the epoch moves)
    elif case == "sub_ranges":
        m = n - 1
        for k, first in enumerate((0, 1, 0, 1)):
            sc = sets[k % 3][: 32 * m]
            want = orc.msm_pippenger(curve, pts[ps * first: ps * (first + m)], sc, m, 1, threads=8)
            got = task(k, sc, want, m, ps * first)
            assert run_msm(off, None, sc, m, hbm=(ADDR, ps * first)) == got
    elif case == "scalar_ranges":
        for k, (lo, hi) in enumerate(((0, 128), (128, 256), (0, 128), (128, 256))):
            cl.set_scalar_range(lo, hi)
            off.set_scalar_range(lo, hi)
            got = task(k, sets[0], orc.msm_pippenger(curve, pts, _masked(sets[0], n, lo, hi), n, 1, threads=8))
            assert run_msm(off, None, sets[0], n, hbm=(ADDR, 0)) == got
    else:
        for k in range(3):
            got = task(k)
            assert run_msm(off, None, sets[k], n, hbm=(ADDR, 0)) == got
    cl.close(); off.close()
    _release()


def test_explicit_modes_stay_paced(gpu, orc, monkeypatch):
    """set_window_table(2) means what it meant: the first task over the bases enqueues its share of the build and takes the
    plain path; the table is there for a later task, or at once for a host that waits in prepare_window_table."""
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n = "BLS381", 8192
    pts, sets, exp = _inputs(orc, curve, n)
    _release()
    cl = msm_client(curve, 1, PointMemoryType.HBM)
    cl.set_window_table(2)
    cl.load_data_to_hbm(pts, ADDR, 0)
    assert run_msm(cl, None, sets[0], n, hbm=(ADDR, 0)) == exp[0]
    assert cl.window_table_info()["bytes"] == 0
    assert cl.prepare_window_table(n, (ADDR, 0))
    assert run_msm(cl, None, sets[1], n, hbm=(ADDR, 0)) == exp[1]
    built = cl.window_table_info()["bytes"]
    assert built > 0
    # a table a handle asked for is that handle's: an unset handle is not served from it and builds no second one beside it
    auto = msm_client(curve, 1, PointMemoryType.HBM)
    before = _tables(cl)
    for k in range(3):
        assert run_msm(auto, None, sets[k], n, hbm=(ADDR, 0)) == exp[k]
        assert auto.window_table_info()["bytes"] == 0 and _tables(cl) == before
    cl.close(); auto.close()
    _release()


def test_budget_refuses_and_a_rewrite_rearms(gpu, orc, monkeypatch):
    curve, n = "BLS381", 8192
    pts, sets, exp = _inputs(orc, curve, n)
    _release()
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY + ",table_budget_bytes=1")
    cl = msm_client(curve, 1, PointMemoryType.HBM)
    cl.load_data_to_hbm(pts, ADDR, 0)
    for k in range(3):
        assert run_msm(cl, None, sets[k], n, hbm=(ADDR, 0)) == exp[k]
        assert cl.window_table_info()["bytes"] == 0 and _tables(cl) == 0
    # the refusal stands until the next write, whatever the budget is by then
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    for k in range(2):
        assert run_msm(cl, None, sets[k], n, hbm=(ADDR, 0)) == exp[k]
        assert cl.window_table_info()["bytes"] == 0 and _tables(cl) == 0
    cl.load_data_to_hbm(pts, ADDR, 0)
    seen = []
    for k in range(3):
        assert run_msm(cl, None, sets[k], n, hbm=(ADDR, 0)) == exp[k]
        seen.append(cl.window_table_info()["bytes"] > 0)
    assert seen == [False, False, True]
    cl.close()
    _release()


def test_small_rewrite_patches_rows(gpu, orc, monkeypatch):
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n = "BLS381", 8192
    pts, sets, exp = _inputs(orc, curve, n)
    _release()
    cl, off = msm_client(curve, 1, PointMemoryType.HBM), _off_client(curve)
    cl.load_data_to_hbm(pts, ADDR, 0)
    for k in range(3):
        assert run_msm(cl, None, sets[k], n, hbm=(ADDR, 0)) == exp[k]
    built = cl.window_table_info()["bytes"]
    assert built > 0
    # 64 bases rewritten with other bases of the set: the table stays and follows the new bytes at once
    new = bytearray(pts)
    new[96 * 512: 96 * 576] = pts[96 * 100: 96 * 164]
    cl.load_data_to_hbm(bytes(new[96 * 512: 96 * 576]), ADDR, 96 * 512)
    want = orc.msm_pippenger(curve, bytes(new), sets[0], n, 1, threads=8)
    assert run_msm(cl, None, sets[0], n, hbm=(ADDR, 0)) == want
    assert cl.window_table_info()["bytes"] == built
    assert run_msm(off, None, sets[0], n, hbm=(ADDR, 0)) == want
    cl.close(); off.close()
    _release()


def test_whole_rewrite_drops_the_table_and_the_count_starts_again(gpu, orc, monkeypatch):
    """17.3 MB of bases (more than a patch may cover), P_i = (i + 1) G: expected value by linearity."""
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n = "BLS381", 180000
    dp, ds = synth(curve, n, seed=33)
    k = orc.index_weighted_sum(curve, ds.download(), n, 0, threads=8)
    exp = orc.result_from_affine(curve, orc.generator_mul(curve, k))
    _release()
    cl, off = msm_client(curve, 1, PointMemoryType.HBM), _off_client(curve)
    cl.load_data_to_hbm(dp, 0, 0)
    assert run_msm(off, None, ds, n, hbm=(0, 0)) == exp
    seen = []
    for t in range(6):
        if t == 3:
            held = _tables(cl)
            cl.load_data_to_hbm(dp, 0, 0)
            assert _tables(cl) == held - seen_bytes          # the table went with the write (the build's scratch rows stay)
        assert run_msm(cl, None, ds, n, hbm=(0, 0)) == exp, t
        seen.append(cl.window_table_info()["bytes"] > 0)
        seen_bytes = cl.window_table_info()["bytes"]
    assert seen == [False, False, True, False, False, True]
    cl.close(); off.close(); dp.free(); ds.free()
    _release()


def test_two_tasks_in_flight_across_the_switch(gpu, orc, monkeypatch):
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n = "BLS381", 8192
    pts, sets, exp = _inputs(orc, curve, n)
    _release()
    cl = msm_client(curve, 1, PointMemoryType.HBM)
    cl.load_data_to_hbm(pts, ADDR, 0)
    params = MSMParams(n, (ADDR, 0))
    order = [0, 1, 2, 1, 0, 2]
    got, tabled = [], []
    for k, which in enumerate(order):
        cl.initialize(params); cl.start_process(); cl.set_data(MSMInput(None, sets[which], params))
        tabled.append(cl.window_table_info()["bytes"] > 0)
        if k >= 1:
            cl.wait_result(); got.append(cl.result().result)
    cl.wait_result(); got.append(cl.result().result)
    assert got == [exp[w] for w in order]
    # task 2 starts the build ahead of itself; task 3 is submitted while task 2 is still in flight (the build may not be
    # through); task 4 is submitted after task 2 was collected, behind the build
    assert tabled[:2] == [False, False] and tabled[3:] == [True, True, True], tabled
    cl.close()
    _release()


def test_diet_until_the_trigger(gpu, orc, monkeypatch):
    """Under BLZ_ARENA_DROP_RAW an unset handle's extent loses its raw bytes like a plain handle's; the build brings them back."""
    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n = "BLS381", 8192
    pts, sets, exp = _inputs(orc, curve, n)
    m = n - 1
    sub = [s[: 32 * m] for s in sets]
    sub_exp = [orc.msm_pippenger(curve, pts[: 96 * m], s, m, 1, threads=8) for s in sub]
    _release()
    L = blaze_amd.lib()
    blaze_amd._lib.check(L.blz_arena_set_policy(0, 1))
    try:
        cl = msm_client(curve, 1, PointMemoryType.HBM)
        cl.load_data_to_hbm(pts, ADDR, 0)
        assert run_msm(cl, None, sets[0], n, hbm=(ADDR, 0)) == exp[0]              # the canonical check is enqueued
        assert run_msm(cl, None, sub[0], m, hbm=(ADDR, 0)) == sub_exp[0]           # other bases: the count starts again; raw dropped
        assert cl.memory_info()["arena_raw"] == 0 and _tables(cl) == 0
        assert run_msm(cl, None, sub[1], m, hbm=(ADDR, 0)) == sub_exp[1]           # the second task over them: restore + build
        assert cl.window_table_info()["bytes"] == 0 and cl.memory_info()["arena_raw"] > 0
        assert run_msm(cl, None, sub[2], m, hbm=(ADDR, 0)) == sub_exp[2]
        assert cl.window_table_info()["bytes"] > 0
        assert cl.get_data_from_hbm(len(pts), ADDR, 0) == pts
        cl.close()
    finally:
        blaze_amd._lib.check(L.blz_arena_set_policy(0, 0))
        _release()


def test_release_under_memory_pressure(gpu, orc, monkeypatch):
    """The auto-built table is the library's own decision, so the library gives it back: with less device memory free than the
    staging buffer of a 2^20-element task's host scalars needs (32 MiB), but enough once the n = 8192 table is released, the
    allocation succeeds at its second attempt, the table is gone from memory_info, the task - completed by a second slice once
    the test has given its blocks back - equals the oracle, and the table's extent stays on the plain path until its next write."""
    import torch

    monkeypatch.setenv("BLAZE_MSM_PLAN", TINY)
    curve, n, nbig = "BLS381", 8192, 1 << 20
    pts, sets, exp = _inputs(orc, curve, n)
    dp, ds = synth(curve, nbig, seed=44)
    big_sc = ds.download()
    k = orc.index_weighted_sum(curve, big_sc, nbig, 0, threads=8)
    big_exp = orc.result_from_affine(curve, orc.generator_mul(curve, k))
    _release()
    cl, big = msm_client(curve, 1, PointMemoryType.HBM), _off_client(curve)
    hogs, small = [], []
    try:
        cl.load_data_to_hbm(pts, ADDR, 0)
        for j in range(3):
            assert run_msm(cl, None, sets[j], n, hbm=(ADDR, 0)) == exp[j]
        table = cl.window_table_info()["bytes"]
        before = _tables(cl)
        assert table > (8 << 20) and before >= table
        big.load_data_to_hbm(dp, 1 << 40, 0)
        for _ in range(3):    # the workspace of both engine slots and the Montgomery copy in place (device scalars are used in place)
            assert run_msm(big, None, ds, nbig, hbm=(1 << 40, 0)) == big_exp
        need = nbig * 32                                                 # what the next task must allocate: its scalars' staging buffer
        torch.cuda.synchronize()
        # The bulk goes to one torch block sized from mem_get_info; that figure is not what an allocation can still get (memory
        # freed earlier is credited late, and a 36 MiB hipMalloc succeeded with 22 MiB reported free), so the last GiB is taken in
        # blocks of the library's allocator, probing: in the end an allocation of `need` bytes fails and one of need - 2 MiB
        # did not - too little for the buffer, enough with the table's 17 MiB.
        for _ in range(4):
            free, _total = torch.cuda.mem_get_info(0)
            if free < (2 << 30):
                break
            hogs.append(torch.empty(free - (1 << 30), dtype=torch.uint8, device="cuda:0"))

        def fits(nbytes):
            try:
                probe = DeviceBuffer(0, nbytes)
            except blaze_amd.DriverClientError:
                return False
            probe.free()
            return True

        for step in (1 << 30, 128 << 20, 16 << 20, 2 << 20):
            while fits(need + step - (2 << 20)) and len(small) < 400:
                small.append(DeviceBuffer(0, step))
        assert not fits(need) and table > (4 << 20), (len(small), table)
        # the task's first slice: its staging buffer is allocated here - fails, the table goes, the retry succeeds - and only
        # copies follow.  No kernel runs on the full device: the tail's kernels keep lane-private memory the runtime allocates
        # per dispatch (374 MB for this task), which a device with less than the table's 17 MiB free cannot give - the queue
        # aborts.  The blocks are given back before the slice that completes the task and launches it.
        half = nbig // 2
        params = MSMParams(nbig, (1 << 40, 0))
        big.initialize(params); big.start_process()
        big.set_data(MSMInput(None, big_sc[: 32 * half], MSMParams(half, (1 << 40, 0))))
        assert _tables(cl) == before - table
        while small:
            small.pop().free()
        hogs.clear()
        torch.cuda.empty_cache()
        big.set_data(MSMInput(None, big_sc[32 * half:], MSMParams(nbig - half, (1 << 40, 0))))
        big.wait_result()
        assert big.result().result == big_exp
        # no rebuild into the same shortage: plain path until the next write, then the policy is armed again
        for j in range(3):
            assert run_msm(cl, None, sets[j], n, hbm=(ADDR, 0)) == exp[j]
            assert cl.window_table_info()["bytes"] == 0
        cl.load_data_to_hbm(pts, ADDR, 0)
        seen = []
        for j in range(3):
            assert run_msm(cl, None, sets[j], n, hbm=(ADDR, 0)) == exp[j]
            seen.append(cl.window_table_info()["bytes"] > 0)
        assert seen == [False, False, True]
    finally:
        while small:
            small.pop().free()
        hogs.clear()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        cl.close(); big.close(); dp.free(); ds.free()
        _release()
