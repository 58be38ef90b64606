"""The MSM sort stage's choice restated in Python: which of the three digit sorts a task runs in front of its accumulation and
on which stream, as MsmEngine::begin() and sort_slice() decided it BEFORE the decision moved into plan_sort()
(msm_sort_stage.hip) - a transcription of their booleans (s3, fits, hide, pingpong, use_s3, tiny), statement by statement, not
of the rules plan_sort() is written in.  It takes the window plan as blz_test_msm_tail_plan returns it; msm_sort3_ok (plain
plans) and msm_sort_tiny_ok are restated from those numbers.  tests/test_msm_sort_plan.py compares its line with the library's
over a grid of shapes."""
from msm_tail_ref import pieces_of


def sort3_ok(plan, widths, sbits):
    """msm_sort3_ok: every window a whole number of level-1 bins (2^14 buckets), at most 2048 of those and 2048 x 256 level-2 bins."""
    c, W, G, L, Bw, Wv, ebits, table = plan
    if table:
        return True                                  # (msm_task_plan refuses a table plan outside the sort's range)
    if sbits not in (256, 64, 32) or W < 1:
        return False
    if any(w < 15 or w > 23 for w in widths):
        return False
    if G >> 14 > 2048 or G & ((1 << 14) - 1):
        return False
    return G >> 7 <= 2048 * 256


def sort_tiny_ok(plan, npts, sbits):
    """msm_sort_tiny_ok: the bucket space fits one block's LDS, the scalars are few enough for one block to walk twice."""
    c, W, G, L, Bw, Wv, ebits, table = plan
    if table or W < 1 or sbits not in (256, 64, 32):
        return False
    return 0 < G <= 24576 and npts <= 20480 and 1 <= L <= 1024


def line(npts, plan, widths, sbits, pieces, hide_env, other_busy, recent_hot, fits_beside):
    """The canonical line (msm_engine.hpp describe(SortPlan)) of a task of npts points on the window plan
    plan = (c, W, G, L, Bw, Wv, ebits, table), asked for in `pieces` pieces; hide_env: BLAZE_SORT_HIDE; other_busy: the handle's other
    slot holds a task; recent_hot: recent_hot[0] || recent_hot[1]; fits_beside: what sort_fits() answers."""
    table = bool(plan[7])
    nslices = pieces_of(npts, pieces, table)

    # ---- begin()
    s3 = table or (hide_env != 0 and nslices == 1 and sort3_ok(plan, widths, sbits))
    fits = True
    if s3 and hide_env == 1 and not table:
        if recent_hot:
            s3 = False
    if s3 and hide_env == 1:
        fits = fits_beside
        if not fits and not table:
            s3 = False
    hide = s3 and other_busy and hide_env != 0 and fits
    pingpong = (nslices > 1 and hide_env != 0 and not other_busy and not table and sort3_ok(plan, widths, sbits) and not recent_hot
                and fits_beside)
    if pingpong:
        s3 = True
        hide = True
    use_s3 = s3 and (hide or hide_env == 2 or table)
    sort_hidden = hide

    # ---- sort_slice() (a one-piece task's piece is the whole task: np == npts)
    tiny = not use_s3 and nslices == 1 and sort_tiny_ok(plan, npts, sbits)

    kind = "s3" if use_s3 else "tiny" if tiny else "lds"
    where = "pingpong" if pingpong else "hidden" if sort_hidden else "open"
    return kind + " " + where
