"""The MSM sort stage's choice - which of the three digit sorts a task runs in front of its accumulation, and on which stream -
is decided once, by plan_sort() (msm_sort_stage.hip), and is pure host arithmetic over the window plan and four inputs: pinned
here without a device, through blz_test_msm_sort_plan, against the Python transcription of the booleans MsmEngine::begin() and
sort_slice() used to compute (tests/msm_sort_ref.py), the invariants of the five lines, and the literal lines of today's
default shapes."""
import ctypes as C
import itertools

import pytest

import blaze_amd
import msm_sort_ref as ref
from test_msm_tail_plan import CURVE_ID, FIELDS, SHAPES, SIZES, tail_plan

LINES = {"lds open", "tiny open", "s3 open", "s3 hidden", "s3 pingpong"}
INPUTS = list(itertools.product((0, 1, 2), (False, True), (False, True), (False, True)))   # hide_env, other_busy, recent_hot, fits


def sort_plan(curve, repr_, npts, sbits=256, pieces=1, table_c=0, bit_lo=0, bit_hi=0, hide_env=1, other_busy=False, recent_hot=False, fits=True):
    """(return code, line) from the library"""
    text = C.create_string_buffer(64)
    rc = blaze_amd.aux().blz_test_msm_sort_plan(CURVE_ID[curve], repr_, npts, sbits, pieces, table_c, bit_lo, bit_hi, hide_env, int(other_busy),
                                                int(recent_hot), int(fits), text, len(text))
    return rc, text.value.decode()


def tasks():
    """The tasks of the grid: (BLAZE_MSM_PLAN or None, curve, repr, points, keywords of the task)."""
    for curve, repr_ in FIELDS:
        for sbits, per_element in SHAPES:
            for n in SIZES:
                for pieces in (1, 3):
                    yield None, curve, repr_, n * per_element, dict(sbits=sbits, pieces=pieces)
        for bases in (1 << 12, 1 << 20):
            for c in range(16, 27):
                yield None, curve, repr_, bases, dict(table_c=c)
        for pieces in (1, 3):
            yield None, curve, repr_, 1 << 20, dict(bit_lo=64, bit_hi=160, pieces=pieces)
        yield "c=15", curve, repr_, 5000, dict(pieces=3)      # the shape of the ping-pong GPU test


@pytest.fixture(scope="module")
def grid():
    """[(what, task keywords, inputs, the library's line, the restated booleans' line)], computed once."""
    rows = []
    with pytest.MonkeyPatch.context() as mp:
        for override, curve, repr_, npts, kw in tasks():
            if override:
                mp.setenv("BLAZE_MSM_PLAN", override)
            else:
                mp.delenv("BLAZE_MSM_PLAN", raising=False)
            rc, plan, widths, _tail = tail_plan(curve, repr_, npts, **kw)
            assert rc == 0, (curve, repr_, npts, kw, blaze_amd.lib().blz_last_error_message())
            for hide_env, busy, hot, fits in INPUTS:
                inputs = dict(hide_env=hide_env, other_busy=busy, recent_hot=hot, fits=fits)
                rc, line = sort_plan(curve, repr_, npts, **kw, **inputs)
                what = f"{curve} repr={repr_} npts={npts} {kw} {override or ''} {inputs}"
                assert rc == 0, (what, blaze_amd.lib().blz_last_error_message())
                want = ref.line(npts, plan, widths, kw.get("sbits", 256), kw.get("pieces", 1), hide_env, busy, hot, fits)
                rows.append((what, dict(kw, table=bool(plan[7]), nslices=ref.pieces_of(npts, kw.get("pieces", 1), bool(plan[7]))), inputs, line, want))
    return rows


def test_line_matches_the_restated_booleans(grid):
    assert len(grid) >= 4 * (len(SIZES) * len(SHAPES) * 2 + 22 + 2 + 1) * len(INPUTS)
    for what, _kw, _inputs, line, want in grid:
        assert line == want, what


def test_the_grid_holds_every_line_where_it_belongs(grid):
    assert {line for _w, _kw, _i, line, _want in grid} == LINES
    for what, kw, inputs, line, _want in grid:
        if line == "tiny open":
            assert kw["nslices"] == 1 and not kw["table"], what
        if line == "s3 pingpong":
            assert kw["nslices"] > 1, what
        if line.endswith("hidden"):
            assert inputs["other_busy"], what
        if kw["table"]:
            assert line.startswith("s3"), what                  # a table task has no other sort
        if inputs["hide_env"] == 0 and not kw["table"]:
            assert not line.startswith("s3"), what


def test_todays_default_lines(monkeypatch):
    """BLAZE_SORT_HIDE unset (1), a build whose three-level sort fits beside the accumulation unless said otherwise."""
    monkeypatch.delenv("BLAZE_MSM_PLAN", raising=False)
    big = 1 << 24
    assert sort_plan("BLS381", 0, big) == (0, "lds open")                                          # other slot idle
    assert sort_plan("BLS381", 0, big, other_busy=True) == (0, "s3 hidden")
    assert sort_plan("BLS381", 0, big, other_busy=True, recent_hot=True) == (0, "lds open")
    assert sort_plan("BLS381", 0, big, other_busy=True, fits=False) == (0, "lds open")
    assert sort_plan("BLS381", 0, 16) == (0, "tiny open")
    monkeypatch.setenv("BLAZE_MSM_PLAN", "c=15")
    assert sort_plan("BLS381", 0, 5000, pieces=3) == (0, "s3 pingpong")


def test_refusals():
    assert sort_plan("BLS381", 0, 0)[0] == 4
    assert sort_plan("BLS381", 0, 1 << 12, bit_lo=8, bit_hi=160)[0] == 4                          # unaligned scalar range
    assert blaze_amd.aux().blz_test_msm_sort_plan(7, 0, 16, 256, 1, 0, 0, 0, 1, 0, 0, 1, C.create_string_buffer(64), 64) == 4
    text = C.create_string_buffer(4)                                                              # a line that does not fit is not truncated
    assert blaze_amd.aux().blz_test_msm_sort_plan(1, 0, 16, 256, 1, 0, 0, 0, 1, 0, 0, 1, text, len(text)) == 4
