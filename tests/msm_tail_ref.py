"""The MSM tail's schedule restated in Python: which unit folds, bucket-reduce levels and finish kernel a task runs behind its
accumulation, as the launchers decided it BEFORE the decision moved into plan_tail() (msm.hip) - a transcription of that
run_accumulate_t / run_reduce_t, condition by condition, including the row-tail condition they computed twice (once per
launcher).  It takes the window plan as blz_test_msm_tail_plan returns it and does not port the window search.
tests/test_msm_tail_plan.py compares its line with the library's over a grid of shapes."""

# (rr, row): the group laws of a field besides the 32-bit thread law - the reduced-radix thread law + the DPP quad law on it,
# and the wave-wide row law (the reduced-radix fields on the loose 28-bit budget)
LAWS = {("BLS377", 0): (True, True), ("BLS381", 0): (True, True), ("BN254", 0): (True, False), ("BN254", 1): (False, False)}
MAX_SLICES = 64


def pieces_of(npts, want, table):
    """MsmEngine::begin: the pieces a task asked for in `want` pieces is enqueued in (whole 16-point groups; not phased)."""
    if want < 1 or table:
        want = 1
    want = min(want, MAX_SLICES)
    per = ((2 * npts + 2 * want - 1) // (2 * want) + 15) & ~15
    return (npts + per - 1) // per if want > 1 else 1


def seg0_of(G):
    seg0 = 64
    while seg0 > 8 and G // seg0 < 262144:
        seg0 >>= 1
    return seg0


def levels_of(Bw, G):
    """[(M, SEG, T)] of the bucket reduce: level 0 in segments of seg0, the upper levels in segments of 8, down to T = 1."""
    out, M = [], Bw
    while True:
        SEG = seg0_of(G) if not out else 8
        T = (M + SEG - 1) // SEG
        out.append((M, SEG, T))
        M = T
        if T == 1:
            return out


def schedule(npts, plan, widths, laws, pieces=1):
    """The canonical line (msm_engine.hpp describe) of a task of npts points on the window plan
    plan = (c, W, G, L, Bw, Wv, ebits, table), widths = its window widths, asked for in `pieces` pieces."""
    c, W, G, L, Bw, Wv, ebits, table = plan
    rr, row = laws
    one_piece = pieces_of(npts, pieces, table) == 1          # run_accumulate_t's slice < 0
    boff = [0] * (W + 1)
    if table:
        boff[W] = G
    else:
        for w in range(W):
            boff[w + 1] = boff[w] + (1 << (widths[w] - 1))
        assert boff[W] == G

    # ---- run_accumulate_t
    maxunits = (npts * (W if table else 1) + L - 1) // L
    passes, stride = 0, 1
    while stride < maxunits:
        passes += 1
        stride *= 16
    thr = 64 if (npts * W // (G or 1) > L // 2 or npts <= 1 << 22) else 0
    hot_start = G
    row_fold = row and one_piece and thr != 0 and G <= 1 << 17 and npts * W // L <= 1 << 17
    # small_row_tail: run_reduce_t's level-0 condition, derived a second time
    row_tail = row_fold and ((Bw + seg0_of(G) - 1) // seg0_of(G)) * Wv <= 8192
    if rr and not table and one_piece and ebits > 0:
        offs, off = [], 0
        for w in range(W):
            offs.append(off)
            off += widths[w]
        lowest, any_hot = -1, False
        for w in range(W - 1, -1, -1):
            cw = widths[w]
            t = min(ebits - offs[w], cw)
            slots = float(1 << (cw - 1))
            active = slots if t >= cw else float((1 << t) + 1) if t > 0 else 1.0 if t == 0 else 0.0
            active = min(active, slots)
            entries = float(npts) if t >= 0 else 0.0
            hot = active > 0 and entries / active >= 12.0 * L
            if not hot and entries > 0:
                break
            lowest = w
            any_hot = any_hot or hot
        if any_hot and lowest > 0 and G - boff[lowest] <= 16384:
            hot_start = boff[lowest]
    words = ["units%d" % passes]
    if rr and hot_start < G:
        words.append("hot_row" if row else "hot")
    if row_fold:
        fold = ("row_weak" if row_tail else "row_strict") if hot_start > 0 else "none"
    elif thr and hot_start > 0:
        fold = "wave" if rr and hot_start <= 32768 else "lane"
    else:
        fold = "none"
    words += ["fold_" + fold, "|"]

    # ---- run_reduce_t
    row_levels = False
    for level, (_M, _SEG, T) in enumerate(levels_of(Bw, G)):
        nthreads = T * Wv
        if row and nthreads <= 8192:
            row_levels = True
        if row_levels:
            kind = "row"
        elif level == 0:
            kind = ("quad" if nthreads <= 131072 else "rr") if rr else "w32"
        else:
            kind = "quad" if rr else "w32"
        words.append(("L0" if level == 0 else "L") + kind)
    words.append("finish_row" if row else "finish")
    return " ".join(words)
