"""The MSM tail's schedule - which fold, reduce-level and finish kernels a task runs behind its accumulation - is decided
once, by plan_tail() (msm.hip), and is pure host arithmetic over the window plan: pinned here without a device, through
blz_test_msm_tail_plan, against the Python restatement of the rules (tests/msm_tail_ref.py), the structural invariants the
kernels depend on, and the literal schedules of the smallest default shape of every distinct one."""
import ctypes as C

import pytest

import blaze_amd
import msm_tail_ref as ref

CURVE_ID = {"BLS377": 0, "BLS381": 1, "BN254": 2}
FIELDS = [("BLS377", 0), ("BLS381", 0), ("BN254", 0), ("BN254", 1)]
SIZES = [1 << k for k in range(27)] + [3000, 70001] + [(1 << k) + d for k in (8, 13, 17, 22) for d in (-1, 1)]
SHAPES = [(256, 1), (32, 8), (64, 4)]          # scalar bits, points per element


def tail_plan(curve, repr_, npts, sbits=256, pieces=1, table_c=0, bit_lo=0, bit_hi=0):
    """(return code, plan = (c, W, G, L, Bw, Wv, ebits, table), widths, line) from the library"""
    out = (C.c_uint32 * 8)()
    wd = (C.c_uint8 * 96)()
    text = C.create_string_buffer(512)
    rc = blaze_amd.aux().blz_test_msm_tail_plan(CURVE_ID[curve], repr_, npts, sbits, pieces, table_c, bit_lo, bit_hi, out, wd, text, len(text))
    plan = tuple(out)
    return rc, plan, list(wd)[:plan[1]], text.value.decode()


def check_point(curve, repr_, npts, **kw):
    """One grid point: the library's line equals the restated rules', and the invariants hold on it."""
    rc, plan, widths, line = tail_plan(curve, repr_, npts, **kw)
    what = f"{curve} repr={repr_} npts={npts} {kw}"
    assert rc == 0, (what, blaze_amd.lib().blz_last_error_message())
    rr, row = laws = ref.LAWS[(curve, repr_)]
    assert line == ref.schedule(npts, plan, widths, laws, kw.get("pieces", 1)), what
    folds, tail = line.split(" | ")
    levels, finish = tail.split()[:-1], tail.split()[-1]
    assert levels[0].startswith("L0") and all(not x.startswith("L0") for x in levels[1:]), what
    kinds = [x[2:] if i == 0 else x[1:] for i, x in enumerate(levels)]
    if "fold_row_weak" in folds:
        assert kinds[0] == "row", what                                  # the weak form has one reader
    if "row" in kinds:
        assert set(kinds[kinds.index("row"):]) == {"row"} and finish == "finish_row", what
    assert (finish == "finish_row") == row, what
    if not row:
        assert "row" not in line, what
    if not rr:
        assert not set(kinds) & {"rr", "quad"} and " hot" not in folds and "fold_wave" not in folds, what
    else:
        assert "w32" not in kinds, what
    assert "rr" not in kinds[1:], what                                  # the lane-per-segment level is a level 0
    c, W, G, L, Bw, Wv, ebits, table = plan
    shape = ref.levels_of(Bw, G)
    assert len(kinds) == len(shape) <= 16 and shape[-1][2] == 1, what   # the levels end at T == 1
    return line


@pytest.mark.parametrize("curve,repr_", FIELDS)
def test_schedule_matches_the_restated_rules(curve, repr_):
    for sbits, per_element in SHAPES:
        for n in SIZES:
            for pieces in (1, 3):
                check_point(curve, repr_, n * per_element, sbits=sbits, pieces=pieces)


@pytest.mark.parametrize("curve,repr_", FIELDS)
def test_table_and_range_plans(curve, repr_):
    for bases in (1 << 12, 1 << 20, 1 << 23):
        for c in range(16, 27):
            line = check_point(curve, repr_, bases, table_c=c)
            assert " hot" not in line                                   # a table plan has no hot suffix
    for n in SIZES:
        for pieces in (1, 3):
            check_point(curve, repr_, n, bit_lo=64, bit_hi=160, pieces=pieces)


@pytest.mark.parametrize("override", ["c=4,L=256", "c=9,L=3", "c=16,L=256", "c=18", "split_ns=0"])
def test_plan_overrides(override, monkeypatch):
    monkeypatch.setenv("BLAZE_MSM_PLAN", override)
    served = 0
    for curve, repr_ in FIELDS:
        for n in SIZES:
            rc, _plan, _widths, _line = tail_plan(curve, repr_, n)
            if rc == 4 and b"no window plan" in blaze_amd.lib().blz_last_error_message():
                continue                                                # (c = 4 cannot index 2^26 points x 65 windows)
            for pieces in (1, 3):
                check_point(curve, repr_, n, pieces=pieces)
            served += 1
    assert served >= 4 * 30


# the smallest default shape of every distinct schedule: (curve, repr, points, scalar bits, pieces, BLAZE_MSM_PLAN, (c, W), line)
PINNED = [
    ("BLS381", 0, 16, 256, 1, None, (3, 86), "units0 fold_row_weak | L0row finish_row"),
    ("BLS381", 0, 1 << 12, 256, 1, None, (9, 29), "units2 hot_row fold_row_weak | L0row Lrow Lrow finish_row"),
    ("BLS377", 0, 1 << 12, 256, 1, None, (9, 29), "units2 hot_row fold_row_weak | L0row Lrow Lrow finish_row"),
    ("BLS381", 0, 1 << 12, 256, 3, None, (9, 29), "units2 fold_wave | L0row Lrow Lrow finish_row"),
    ("BLS381", 0, 1 << 17, 256, 1, None, (13, 20), "units4 hot_row fold_lane | L0quad Lrow Lrow Lrow finish_row"),
    ("BLS381", 0, 1 << 19, 32, 1, None, (17, 2), "units4 fold_row_strict | L0quad Lrow Lrow Lrow Lrow Lrow finish_row"),
    ("BLS381", 0, 1 << 13, 256, 1, "c=18", (18, 15), "units3 fold_lane | L0rr Lquad Lrow Lrow Lrow Lrow finish_row"),
    ("BLS381", 0, 1 << 23, 256, 1, None, (19, 15), "units4 fold_none | L0rr Lquad Lrow Lrow Lrow Lrow finish_row"),
    ("BN254", 0, 1 << 10, 256, 1, None, (7, 37), "units2 hot fold_wave | L0quad Lquad finish"),
    ("BN254", 0, 1 << 16, 256, 1, None, (13, 20), "units3 hot fold_lane | L0quad Lquad Lquad Lquad finish"),
    ("BN254", 0, 1 << 14, 256, 1, "c=18", (18, 15), "units3 fold_lane | L0rr Lquad Lquad Lquad Lquad Lquad finish"),
    ("BN254", 1, 1 << 12, 32, 1, None, (9, 4), "units2 fold_lane | L0w32 Lw32 Lw32 finish"),
]


def pinned_id(row):
    return f"{row[0]}-r{row[1]}-{row[2]}x{row[3]}b-p{row[4]}" + (f"-{row[5]}" if row[5] else "")


@pytest.mark.parametrize("row", PINNED, ids=pinned_id)
def test_pinned_schedules(row, monkeypatch):
    curve, repr_, npts, sbits, pieces, override, cw, want = row
    if override:
        monkeypatch.setenv("BLAZE_MSM_PLAN", override)
    rc, plan, _widths, line = tail_plan(curve, repr_, npts, sbits=sbits, pieces=pieces)
    assert rc == 0 and plan[:2] == cw and line == want
    if (curve, sbits, npts, override) == ("BLS381", 256, 1 << 13, "c=18"):
        assert plan[2] == 1966080


def test_refusals_come_at_plan_time():
    """What the launchers could only get wrong silently is an error of the plan, before anything is enqueued."""
    rc, *_ = tail_plan("BLS381", 0, 0)
    assert rc == 4
    rc, *_ = tail_plan("BLS381", 0, 1 << 12, bit_lo=8, bit_hi=160)         # unaligned scalar range
    assert rc == 4
    assert blaze_amd.aux().blz_test_msm_tail_plan(7, 0, 16, 256, 1, 0, 0, 0, (C.c_uint32 * 8)(), None, C.create_string_buffer(64), 64) == 4
    text = C.create_string_buffer(8)                                       # a line that does not fit is not truncated
    assert blaze_amd.aux().blz_test_msm_tail_plan(1, 0, 16, 256, 1, 0, 0, 0, (C.c_uint32 * 8)(), None, text, len(text)) == 4
