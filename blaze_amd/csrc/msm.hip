// Pippenger windowed-bucket G1 MSM for gfx950 (the device task of SURVEY.md a7: what the FPGA
// bitstream behind src/ingo_msm/msm_hw_code.rs:6-54 computes; kernels are new design).
//
// Pipeline (main stream, then the tail stream from the second reduce level on):
//   msm_sort_stage.hip   the sort stage, by one of three sorts (plan_sort()): signed window digits of every scalar ->
//                  count[] per bucket, (point index | sign) entries grouped by bucket, bucket offsets + accumulate-unit
//                  offsets (runs split at L), unit -> bucket map, the units ordered by run length (descending)
//   k_accumulate   one lane per unit: gathers its run of points, XYZZ mixed adds   [phase 1]
//   k_combine_units   only when a bucket needed more than one unit
//   k_reduce_level Sum_b b*S_b per virtual window by segmented running sums        [phase 2]
//   k_finish(_row) stitch virtual windows, Horner over windows, one inversion, Z=1|y|x  [phase 3]
// A task is enqueued in steps - begin / per piece sort_slice + accumulate_slice / end - so that host buffers can be handed to
// the device piece by piece while they cross the PCIe link (pieces share one bucket space: k_accumulate_cont).
//
// HBM layout: points AoS Montgomery (one 128-B line per BLS point, 64 B per BN254 point), scalars raw
// 32 B LE, entries u32, bucket partials AoS XYZZ (4N dwords).  The arithmetic (v_mad_u64_u32) bounds
// the dominant kernels, not HBM.
#include "msm_engine.hpp"
#include <mutex>
#include "field.hip.hpp"
#include "msm_digits.hip.hpp"

namespace blz {

size_t fq_bytes(int curve) { return curve == BLZ_BN254 ? 32 : 48; }
size_t mont_point_bytes(int curve) { return curve == BLZ_BN254 ? 64 : 128; }

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
// Window choice by a cost model fitted to MI355X measurements (tools/sweep_c.py, 2^16..2^26 points):
//   0.163 ns per entry (digit sort + one mixed add), 0.62 ns per occupied bucket (two full adds in the
//   bucket reduce, unit bookkeeping), 0.03 ns per empty bucket.
// `ebits` is the expected significant width of the scalars (bit length of r: 255 / 253 / 254; 32 for a
// pf = 8 chunk).  It only steers the choice - W always covers sbits + 1 bits, so scalars above 2^ebits
// are still summed correctly - but it matters: the top window holds ebits - (W-1) c real bits, i.e.
// fewer occupied buckets than 2^(c-1), or (c = 17 on 255-bit scalars) nothing but the carry of the
// window below.  A window whose entries fall into a handful of buckets used to cost 0.1 - 0.4 ns per
// entry extra; with the run-splitting units, the cooperative fills and the quad-folded combine it is
// within noise (t_hot), so odd c are no longer avoided.
//
// Layouts searched: W windows, the lowest k of width cmin+1, the next W-1-k of width cmin, and a top
// window of max(cmin, what is left of sbits+1) bits (its upper bits are zero for canonical scalars, so
// its signed digits never go negative; only 2^(real bits) of its buckets are occupied).  k = 0 with a
// top window of cmin bits is the uniform plan; BLAZE_MSM_PLAN c= forces that one.
// Unit length: a unit is one lane's sequential chain (L mixed adds of ~15 us each when the SIMD has
// little else to run), so on small inputs long units ARE the runtime: 2^18 points, c = 13 spent
// 3.7 of 7.2 ms waiting for the 256-long units of the short top window.  Keep the longest chain
// below about half of the throughput-bound time of the whole accumulation.
static uint32_t unit_length(uint32_t npts, int W) {
    const double chain = (double)npts * W * 5.5e-6;
    uint32_t L = 16;
    while (L < 256 && 2.0 * L <= chain) L <<= 1;
    return L;
}

static MsmPlan search_plan(uint32_t npts, int sbits, int ebits, int force_c, int split_ns, int max_w) {
    MsmPlan best;
    double best_cost = 1e300;
    const double t_entry = 0.163, t_bucket = 0.62, t_empty = 0.03, t_hot = 0.01;
    const int need = sbits + 1;
    const double t_split = (double)split_ns;
    for (int cmin = 3; cmin <= 23; ++cmin) {
        if (force_c > 0 && cmin != force_c) continue;
        for (int W = 1; W <= max_w; ++W) {
            // entries are indexed with u32, and the kernels' strided walks over them (i += stride, up to 2^24 lanes) must not wrap:
            // at 2^32 - 4 entries they did - wrong sums after seconds of re-walking the bins (tests/probes/big_probe.py)
            if ((uint64_t)npts * W > MSM_MAX_ENTRIES) break;
            const int lower = W - 1;
            for (int k = 0; k <= lower; ++k) {
                if (force_c > 0 && k != 0) break;
                if (k > 0 && cmin + 1 > 23) break;
                const int low_bits = lower * cmin + k;
                if (low_bits >= need + cmin) break;            // a window too many
                int top = need - low_bits;
                if (top < cmin) top = cmin;
                if (top > 23) continue;
                if (top - cmin > 7) continue;                  // k_finish walks 2^(top - cmin) virtual windows in sequence
                if (force_c > 0 && top != cmin) continue;
                // cost over the windows
                double cost = 0;
                uint64_t G = 0;
                int off = 0;
                for (int w = 0; w < W; ++w) {
                    const int cw = w == lower ? top : (w < k ? cmin + 1 : cmin);
                    const double Bw = (double)(1ull << (cw - 1));
                    // (plan_tail() keeps its own copy of this occupancy model: there t == 0 counts npts entries, not half, and `active` is not clamped to `entries`)
                    int t = ebits - off;                        // real scalar bits in this window
                    if (t > cw) t = cw;
                    double entries, active;
                    if (t >= cw) { entries = npts; active = Bw; }
                    else if (t > 0) { entries = npts; active = (double)(1ull << t) + 1; if (active > Bw) active = Bw; }
                    else if (t == 0) { entries = 0.5 * npts; active = 1; }   // carry of a full window below
                    else { entries = 0; active = 0; }
                    if (active > entries) active = entries;
                    cost += entries * t_entry + active * t_bucket + (Bw - active) * t_empty;
                    if (active > 0 && entries / active > 8192.0) cost += entries * t_hot;
                    G += 1ull << (cw - 1);
                    off += cw;
                    // a window of m > 1 virtual windows costs k_finish 2 (m - 1) + 1 more quad additions
                    // (~6 us each, sequential): irrelevant at 2^26, decisive below 2^21
                    const int m = 1 << (cw - cmin);
                    if (m > 1) cost += (2.0 * (m - 1) + 1.0) * t_split;
                }
                if (G > (1ull << 26)) continue;                 // workspace bound (partials: 192 B each)
                if (cost < best_cost) {
                    best_cost = cost;
                    best = MsmPlan();
                    best.npts = npts; best.sbits = sbits; best.W = W; best.G = G;
                    best.c = k > 0 ? cmin + 1 : cmin;
                    best.Bw = 1u << (cmin - 1);
                    uint32_t b = 0;
                    for (int w = 0; w < W; ++w) {
                        const int cw = w == lower ? top : (w < k ? cmin + 1 : cmin);
                        best.width[w] = (uint8_t)cw;
                        best.boff[w] = b;
                        b += 1u << (cw - 1);
                    }
                    best.boff[W] = b;
                    best.Wv = (int)(G >> (cmin - 1));
                    best.cost = cost;
                    best.ebits = ebits;
                }
            }
        }
    }
    best.L = unit_length(npts, best.W);
    return best;
}

// The search walks a few hundred thousand layouts (0.2 - 0.6 ms of host time): a task of 8192 elements - the reference's
// default size - is done on the device in 1.9 ms and asks for its plan twice (set_data's check, begin()), so the last few
// answers are kept.  Keyed on everything the search reads.
MsmPlan make_plan(uint32_t npts, int sbits, int ebits, int force_c) {
    if (ebits <= 0 || ebits > sbits) ebits = sbits;
    const int split_ns = plan_override("split_ns", 6000);  // BLAZE_MSM_PLAN: tests set 0 - mixed widths at any size
    struct Memo {
        uint32_t npts = 0;
        int sbits = 0, ebits = 0, force_c = 0, split_ns = 0;
        MsmPlan plan;
    };
    static std::mutex mu;
    static Memo memo[16];
    static unsigned next = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const Memo& m : memo)
            if (m.sbits == sbits && m.npts == npts && m.ebits == ebits && m.force_c == force_c && m.split_ns == split_ns) return m.plan;
    }
    // The 64-bit chunks of a checked precompute table (arena_tables.hip resolve_arena_task): the cost model, fitted to 256-bit scalars,
    // moves from four windows of 16 / 17 bits to three of 22 / 22 / 21 at 2^24.5 points; measured (BN254, same box), the three-window
    // plan already wins at 2^24 points (5.60 against 6.53 ms per MSM) and loses at 2^22 (2.67 against 1.81): four windows leave
    // 163 K buckets of hundreds of entries - a few units per lane - and the accumulation's last wave of units idles the chip.
    const int max_w = (sbits == 64 && force_c == 0 && npts >= (3u << 22)) ? 3 : MSM_MAX_W;
    const MsmPlan P = search_plan(npts, sbits, ebits, force_c, split_ns, max_w);
    std::lock_guard<std::mutex> lk(mu);
    Memo& m = memo[next++ % 16];
    m.npts = npts; m.sbits = sbits; m.ebits = ebits; m.force_c = force_c; m.split_ns = split_ns;
    m.plan = P;
    return P;
}

// Window-table plans (msm_engine.hpp MsmPlan::table, msm_impl.hip.hpp k_build_window_table).  Costs fitted to the round-3 kernels on the table
// shape: 0.130 ns per entry (one mixed addition; the sort is hidden), 0.34 ns per bucket slot (two full additions in the
// level-0 reduce - 12.6 ms for the 2^25 buckets of c = 26 - scans, unit lists).  2^26 bases: c = 26, 10 windows (671 M
// additions instead of the 805 M of the 12-window plan without a table: 106.6 ms per MSM against 116.2; c = 24, 11 windows:
// 108.7); 2^24: c = 24 (30.0 against 33.2 ms); 2^23: c = 22 (17.2 against 18.3 ms).
int table_window_bits(uint32_t npts, int need_bits) {
    const int forced = plan_override("table_c", 0);
    int best = 0;
    double best_cost = 1e300;
    for (int c = 16; c <= 26; ++c) {
        if (forced > 0 && c != forced) continue;
        const int W = table_windows(c, need_bits);
        if (c > 16 && table_windows(c - 1, need_bits) == W && forced <= 0) continue;   // same additions, twice the buckets: dominated
        if ((uint64_t)npts * W >= (1ull << 30)) continue;
        const double cost = (double)npts * W * 0.130 + (double)(1ull << (c - 1)) * 0.34;
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}

MsmPlan make_table_plan(uint32_t npts, int c, int need_bits) {
    MsmPlan P;
    if (c < 16 || c > 26 || need_bits < 2 || need_bits > 257) return P;
    const int W = table_windows(c, need_bits);
    if ((uint64_t)npts * W >= (1ull << 30)) return P;
    P.npts = npts; P.sbits = need_bits - 1; P.c = c; P.W = W; P.table = true;
    P.G = 1ull << (c - 1);
    for (int w = 0; w < W; ++w) { P.width[w] = (uint8_t)c; P.boff[w] = 0; }
    P.boff[W] = (uint32_t)P.G;
    P.Bw = 1u << (c - 1 - 5);   // the one window is walked as 32 virtual windows (k_finish stitches them)
    P.Wv = 32;
    P.L = unit_length(npts, W);
    return P;
}

// ------------------------------------------------------------------------------------------------
// tail plan (msm_engine.hpp TailPlan): host arithmetic over the window plan, no device
// ------------------------------------------------------------------------------------------------
int plan_tail(const MsmPlan& P, TailTraits tr, bool piecewise, TailPlan& T) {
    T = TailPlan();
    // ---- unit folds.  A bucket holds at most one entry per point (window-table tasks: one per point and window)
    // (64-bit stride: with BLAZE_MSM_PLAN L < 8 and close to 2^31 points, maxunits exceeds 2^28 and a u32 stride would wrap to 0)
    const uint64_t maxunits = ((uint64_t)P.npts * (P.table ? P.W : 1) + P.L - 1) / P.L;
    for (uint64_t stride = 1; stride < maxunits; stride *= 16) ++T.unit_passes;
    // where the plan itself says that buckets hold several units each (mean run > L / 2), the lane-per-bucket fold takes
    // every bucket of up to 64 units and the tree only the hot ones beyond
    // (... and for every task of up to 2^22 points: one window of such a task can be twice as dense as the mean - the top real
    // window of 255-bit scalars below r covers 0x39f6 of its 2^15 buckets at c = 16 - and the quad tree, built for a handful of
    // hot buckets, spent 0.48 ms of a 4.8 ms 2^20 task on its 14 K two-unit buckets; one pass over the unit offsets is nothing here)
    T.thr = ((uint64_t)P.npts * P.W / (P.G ? P.G : 1) > P.L / 2 || P.npts <= (1u << 22)) ? 64u : 0u;
    // The windows the plan knows to be hot (the top ones, where the scalars' bits run out: a few buckets with long runs):
    // a suffix [hot_start, G) of the bucket space goes to k_fold_hot - eight waves per bucket, sixteen on the row law - and the
    // other folds leave it alone.  Only for a small suffix of a larger space: where EVERY window is like that (the precompute
    // shapes) the lane-per-bucket fold is the throughput-bound answer.
    T.hot_start = (uint32_t)P.G;
    if (tr.rr && !P.table && !piecewise && P.ebits > 0) {
        int lowest = -1, off = 0;
        bool any = false;
        int offs[MSM_MAX_W];
        for (int w = 0; w < P.W; ++w) { offs[w] = off; off += P.width[w]; }
        for (int w = P.W - 1; w >= 0; --w) {
            const int cw = P.width[w];
            // (search_plan()'s occupancy model, not quite: t == 0 counts npts entries here, half of them there, and only the planner clamps `active` to `entries`)
            int t = P.ebits - offs[w];
            if (t > cw) t = cw;
            const double slots = (double)(1ull << (cw - 1));
            double active = t >= cw ? slots : t > 0 ? (double)(1ull << t) + 1.0 : t == 0 ? 1.0 : 0.0;
            if (active > slots) active = slots;
            const double entries = t >= 0 ? (double)P.npts : 0.0;
            const bool hot = active > 0 && entries / active >= 12.0 * (double)P.L;   // a dozen units or more per bucket
            if (!hot && entries > 0) break;       // a normal window: the suffix ends above it
            lowest = w;
            any = any || hot;
        }
        if (any && lowest > 0 && P.G - P.boff[lowest] <= 16384) T.hot_start = P.boff[lowest];
    }
    if (T.hot_start < P.G) T.hot = tr.row ? TailPlan::HOT_ROW : TailPlan::HOT_WAVES8;

    // ---- bucket reduce
    // level 0 is throughput-bound (2 adds per bucket): long segments; the upper levels have few
    // lanes and are latency-bound on their sequential chain: short segments, more levels
    // (a small bucket space cannot fill the chip with long segments: the level wants >= 2^18 lanes - two full rounds of
    // two waves per SIMD - before it wants long segments; the extra segment sums are absorbed by the upper levels, which
    // run on the tail stream).  Same-box sweeps, profiles/r03_seg_sweep.txt: 17.8 M bucket slots (the 2^26 plan) 64 best; 12.6 M: 32 (61.9 against 62.9 ms per MSM);
    // 5 - 7 M: 16 (17.2 against 17.8); 2.1 M (2^22): 8 (10.1 against 11.1).  Powers of two only: the upper levels weigh
    // segment t by shifts.
    uint32_t seg0 = 64;
    while (seg0 > 8 && P.G / seg0 < 262144) seg0 >>= 1;
    seg0 = (uint32_t)exp_knob("BLAZE_MSM_SEG", (int)seg0);
    const uint32_t segu = (uint32_t)exp_knob("BLAZE_MSM_SEG_UPPER", 8);
    const uint32_t quad_max = (uint32_t)exp_knob("BLAZE_REDUCE_QUAD_MAX", 131072), row_max = (uint32_t)exp_knob("BLAZE_REDUCE_ROW_MAX", 8192);
    bool row_levels = false;
    int shift = 0;
    for (uint32_t M = P.Bw;;) {
        if (T.levels == 16) return fail(BLZ_ERR_UNKNOWN, "bucket reduce of %u buckets per window needs more than 16 levels (segments of %u / %u)", P.Bw, seg0, segu);
        TailPlan::Level& l = T.level[T.levels];
        l.M = M;
        l.SEG = T.levels == 0 ? seg0 : segu;
        l.T = l.SEG ? (M + l.SEG - 1) / l.SEG : M;
        l.shift = shift;
        // few segments: one per wave on the row law, from here to the end (k_reduce_level_row); else level 0 a lane per segment
        // (a quad while the level is small), the upper levels a quad
        if (tr.row && l.T * (uint32_t)P.Wv <= row_max) row_levels = true;
        l.kind = row_levels ? TailPlan::Level::ROW : !tr.rr ? TailPlan::Level::W32
                 : T.levels > 0 || l.T * (uint32_t)P.Wv <= quad_max ? TailPlan::Level::QUAD : TailPlan::Level::RR;
        for (uint32_t t = 1; t < l.SEG; t <<= 1) ++shift;   // (the next level weighs this one's segments by shifts)
        ++T.levels;
        M = l.T;
        if (M == 1) break;
    }

    // ---- bucket folds.  Where the curve has the row law, a task of up to 2^17 bucket slots and units folds its buckets on it: one
    // wave per bucket; the sums leave in the accumulator form unless everything behind them runs on the row law too
    // (a latency tool: chip-wide the row law adds ~5 x slower than one lane per point - 2^18 elements, 82 K buckets of four units:
    // 0.41 ms against the lane-per-bucket fold's 0.19 - so only while the units to fold are few)
    if (T.thr == 0 || T.hot_start == 0) T.fold = TailPlan::FOLD_NONE;
    else if (tr.row && !piecewise && P.G <= (1u << 17) && (uint64_t)P.npts * P.W / P.L <= (1u << 17))
        T.fold = T.level[0].kind == TailPlan::Level::ROW ? TailPlan::FOLD_ROW_WEAK : TailPlan::FOLD_ROW_STRICT;
    else   // small bucket spaces: one wave per bucket (latency), else one lane (throughput)
        T.fold = tr.rr && T.hot_start <= 32768 ? TailPlan::FOLD_WAVE : TailPlan::FOLD_LANE;

    // ---- finish
    T.finish_row = tr.row;
    FinishPlan& fp = T.fp;
    fp.W = P.W;
    fp.logV = 0;
    while ((1u << fp.logV) < P.Bw) ++fp.logV;
    if (P.table) {
        // one bucket set for all the scalar's windows (their weights are in the table's points): a single window at bit 0
        fp.W = 1;
        fp.v0[0] = 0;
        fp.m[0] = (uint8_t)(P.G >> fp.logV);
        fp.off[0] = 0;
    } else {
        int off = P.base_bit;
        for (int w = 0; w < P.W; ++w) {
            const uint32_t v0 = P.boff[w] >> fp.logV, m = (P.boff[w + 1] - P.boff[w]) >> fp.logV;
            if (v0 > 0xffffu || m > 0xffu || off > 0xffff)
                return fail(BLZ_ERR_UNKNOWN, "window plan outside k_finish's table range (window %d: v0=%u m=%u off=%d)", w, v0, m, off);
            fp.v0[w] = (uint16_t)v0;
            fp.m[w] = (uint8_t)m;
            fp.off[w] = (uint16_t)off;
            off += P.width[w];
        }
    }

    // ---- what the launchers could only get wrong silently
    const char* bad = nullptr;
    if ((T.hot == TailPlan::HOT_WAVES8 || T.fold == TailPlan::FOLD_WAVE) && !tr.rr) bad = "a reduced-radix fold";
    if ((T.hot == TailPlan::HOT_ROW || T.fold == TailPlan::FOLD_ROW_STRICT || T.fold == TailPlan::FOLD_ROW_WEAK || T.finish_row) && !tr.row) bad = "a row-law kernel";
    if (!T.finish_row && tr.row) bad = "the quad walk";   // (k_finish exists for the fields without the row law only)
    if (T.fold == TailPlan::FOLD_ROW_WEAK && T.level[0].kind != TailPlan::Level::ROW) bad = "a weak row fold without a row level 0 behind it";
    for (int l = 0; l < T.levels && !bad; ++l) {
        const TailPlan::Level::Kind k = T.level[l].kind;
        if (k == TailPlan::Level::ROW ? !tr.row : k == TailPlan::Level::W32 ? tr.rr : !tr.rr) bad = "a reduce level on a law the field lacks";
        else if (k == TailPlan::Level::RR && l > 0) bad = "the lane-per-segment reduced-radix level above level 0";
        else if (l > 0 && T.level[l - 1].kind == TailPlan::Level::ROW && k != TailPlan::Level::ROW) bad = "a row level in front of another law's";
    }
    if (bad) return fail(BLZ_ERR_UNKNOWN, "tail plan names %s (%s)", bad, describe(T).c_str());
    return BLZ_OK;
}

std::string describe(const TailPlan& T) {
    static const char* const hot[] = {"", " hot", " hot_row"};
    static const char* const fold[] = {"none", "lane", "wave", "row_strict", "row_weak"};
    static const char* const kind[] = {"w32", "rr", "quad", "row"};
    std::string s = "units" + std::to_string(T.unit_passes) + hot[T.hot] + " fold_" + fold[T.fold] + " |";
    for (int l = 0; l < T.levels; ++l) s += std::string(l ? " L" : " L0") + kind[T.level[l].kind];
    return s + (T.finish_row ? " finish_row" : " finish");
}

__global__ __launch_bounds__(64) void k_words_to_pinned(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n) {
    __builtin_amdgcn_s_setprio(3);
    if (threadIdx.x < n) __hip_atomic_store(dst + threadIdx.x, src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
int copy_words_to_pinned(void* host_pinned, const void* d_src, uint32_t dwords, hipStream_t st) {
    if (dwords > 64) return fail(BLZ_ERR_UNKNOWN, "copy_words_to_pinned: %u dwords", dwords);
    hipLaunchKernelGGL(k_words_to_pinned, dim3(1), dim3(64), 0, st, (uint32_t*)host_pinned, (const uint32_t*)d_src, dwords);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_READ);
    return BLZ_OK;
}

// p[i] = i: the "every bucket has exactly one sum, at its own index" unit_off of piecewise tasks (begin() / end())
__global__ __launch_bounds__(256) void k_iota(uint32_t* __restrict__ p, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] = (uint32_t)i;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

const MsmCurveOps* msm_ops_for(int curve, int repr) {
    switch (curve) {
        case BLZ_BLS377: return &msm_ops_bls377();
        case BLZ_BLS381: return &msm_ops_bls381();
        case BLZ_BN254: return repr ? &msm_ops_bn254_w32() : &msm_ops_bn254();
    }
    return nullptr;
}

int msm_points_from_mont(int format_id, const void* d_mont, void* d_raw, uint64_t npts, hipStream_t st) {
    const MsmCurveOps* ops = (format_id >> 16) ? nullptr : msm_ops_for(format_id & 0xff, (format_id >> 8) & 0xff);   // (an even-base copy is not the whole table)
    if (!ops) return fail(BLZ_ERR_UNKNOWN, "no conversion back from Montgomery format 0x%x", format_id);
    return ops->points_from_mont(d_mont, d_raw, npts, st);
}
int msm_points_all_canonical(int format_id, const void* d_raw, uint64_t npts, uint32_t* flag, hipStream_t st) {
    const MsmCurveOps* ops = msm_ops_for(format_id & 0xff, (format_id >> 8) & 0xff);
    if (!ops) return fail(BLZ_ERR_UNKNOWN, "unknown Montgomery format 0x%x", format_id);
    return ops->points_all_canonical(d_raw, npts, flag, st);
}

int MsmEngine::init(int device_id, int curve_id, int precompute_factor) {
    device = device_id;
    curve = curve_id;
    repr = 0;
    if (curve == BLZ_BN254) {
        // (experiment builds: BLAZE_BN254_REPR = 0 | 1 overrides the choice by precompute factor)
        repr = exp_knob("BLAZE_BN254_REPR", precompute_factor > 1 ? 1 : 0) ? 1 : 0;
    }
    if (!msm_ops_for(curve, repr)) return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d", curve);
    BLZ_TRY(use_device(device));
    // The runtime multiplexes a process's streams over a few hardware queues PER PRIORITY LEVEL, and which queue a new stream
    // lands on depends on every stream the process ever created or destroyed: a handle opened after another one was closed had
    // its sort stream on the main stream's queue - the "hidden" sort then simply waits for the accumulation it should run
    // beneath (config 3: 91 -> 111 ms per MSM, silently).  Streams of another priority level live on queues of their own, so
    // the streams that must run BESIDE the main stream's long kernels - the hidden sort, the tail (reduce levels, Horner walk:
    // the result of task k is due while task k + 1 accumulates), the exchange / combine - are created at the high level; their
    // kernels are short and already raise their wave priority (s_setprio).  Same-box A/B on the headline: 116.7 / 117.0 ms.
    int prio_low = 0, prio_high = 0;
    BLZ_HIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipStreamCreateWithPriority(&tail_stream, hipStreamNonBlocking, prio_high), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipStreamCreateWithPriority(&aux_stream, hipStreamNonBlocking, prio_high), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipStreamCreateWithPriority(&sort_stream, hipStreamNonBlocking, prio_high), BLZ_ERR_UNKNOWN);
    last_sort_done = nullptr;
    for (auto& S : slots) {
        BLZ_TRY(for_each_event(S, [](hipEvent_t& e, bool timed) -> int {
            if (timed) BLZ_HIP(hipEventCreate(&e), BLZ_ERR_UNKNOWN);
            else BLZ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming), BLZ_ERR_UNKNOWN);
            return BLZ_OK;
        }));
        BLZ_HIP(hipHostMalloc((void**)&S.result_h, 256), BLZ_ERR_UNKNOWN);
        BLZ_HIP(hipHostMalloc((void**)&S.stats_h, 64), BLZ_ERR_UNKNOWN);
        memset(S.stats_h, 0, 64);
    }
    BLZ_HIP(hipHostMalloc((void**)&combine_h, 256), BLZ_ERR_UNKNOWN);
    for (auto& B : sbuf) BLZ_TRY(B.stats.reserve(64));
    BLZ_TRY(result.reserve(256 * 64));
    return BLZ_OK;
}

bool MsmEngine::destroy() {
    if (!stream) return true;
    (void)hipSetDevice(device);
    if (sync_stream_bounded(stream, "free: main stream") != BLZ_OK || sync_stream_bounded(tail_stream, "free: tail stream") != BLZ_OK ||
        sync_stream_bounded(sort_stream, "free: sort stream") != BLZ_OK) {
        // work that never completes still references the buffers: freeing them would block (or fault); leak them
        BLZ_LOG(0, "MSM engine freed while its device work is wedged: workspace and streams are leaked");
        stream = tail_stream = aux_stream = sort_stream = nullptr;
        return false;
    }
    for_each_buf([](DevBuf& b) { b.release(); });
    for (auto& S : slots) {
        (void)for_each_event(S, [](hipEvent_t& e, bool) -> int { if (e) (void)hipEventDestroy(e); return BLZ_OK; });
        if (S.result_h) (void)hipHostFree(S.result_h);
        if (S.stats_h) (void)hipHostFree(S.stats_h);
        S = MsmSlot();
    }
    inputs_event = nullptr;
    if (combine_h) (void)hipHostFree(combine_h);
    combine_h = nullptr;
    for (hipStream_t s : {stream, tail_stream, aux_stream, sort_stream}) (void)hipStreamDestroy(s);
    stream = tail_stream = aux_stream = sort_stream = nullptr;
    last_sort_done = nullptr;
    return true;
}

bool MsmEngine::can_accept() const {
    for (const auto& S : slots)
        if (!S.busy) return true;
    return false;
}

int MsmEngine::sync_all() {
    BLZ_TRY(use_device(device));
    BLZ_TRY(sync_stream_bounded(stream, "reset: main stream"));
    BLZ_TRY(sync_stream_bounded(tail_stream, "reset: tail stream"));
    BLZ_TRY(sync_stream_bounded(aux_stream, "reset: exchange stream"));
    BLZ_TRY(sync_stream_bounded(sort_stream, "reset: sort stream"));
    for (auto& S : slots) { S.busy = false; S.open = false; S.task_inputs_event = nullptr; }
    return BLZ_OK;
}

int MsmEngine::points_to_mont(const void* d_raw, void* d_mont, uint32_t npts) {
    BLZ_TRY(use_device(device));
    return msm_ops_for(curve, repr)->points_to_mont(*this, d_raw, d_mont, npts);
}

int MsmEngine::points_to_mont_even(const void* d_raw, void* d_mont, uint32_t nq) {
    BLZ_TRY(use_device(device));
    return msm_ops_for(curve, repr)->points_to_mont_even(*this, d_raw, d_mont, nq);
}
int MsmEngine::check_precompute(const void* d_raw, uint64_t nelem, uint32_t* flag, hipStream_t st) {
    BLZ_TRY(use_device(device));
    return msm_ops_for(curve, 0)->check_precompute(*this, d_raw, nelem, flag, st);   // (reads wire-format points: always on the faster arithmetic)
}

int MsmEngine::build_table(const void* d_raw, void* d_table, uint32_t npts, int c, int W, int base_shift, void* scratch, uint32_t* flag,
                           hipStream_t st) {
    BLZ_TRY(use_device(device));
    return msm_ops_for(curve, repr)->build_table(*this, d_raw, d_table, npts, c, W, base_shift, scratch, flag, st);
}
size_t MsmEngine::table_scratch_bytes(int W) const { return msm_ops_for(curve, repr)->table_scratch_bytes(W); }

static const int kScalarFieldBits[3] = {253, 255, 254};  // bit length of r (BLS12-377 / 381 / BN254)

MsmPlan MsmEngine::plan_for(uint32_t npts, int sbits) const {
    const int ebits = sbits == 256 ? kScalarFieldBits[curve] : sbits;
    return make_plan(npts, sbits, ebits, plan_override("c", 0));
}

static MsmPlan range_plan(int curve, uint32_t npts, int bit_lo, int bit_hi) {
    const int vbits = bit_hi - bit_lo;
    int ebits = kScalarFieldBits[curve] - bit_lo;   // real bits of canonical scalars inside the range
    if (ebits > vbits) ebits = vbits;
    if (ebits < 1) ebits = 1;
    MsmPlan P = make_plan(npts, vbits, ebits, plan_override("c", 0));
    P.base_bit = bit_lo;
    return P;
}
MsmPlan MsmEngine::plan_for_range(uint32_t npts, int bit_lo, int bit_hi) const { return range_plan(curve, npts, bit_lo, bit_hi); }

int msm_task_plan(int curve, uint32_t npts, int sbits, int table_c, int bit_lo, int bit_hi, MsmPlan& P, bool* ranged_out) {
    if (curve < 0 || curve > 2) return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d", curve);
    const int ebits = sbits == 256 ? kScalarFieldBits[curve] : sbits;
    const bool ranged = bit_hi > bit_lo && !(bit_lo == 0 && bit_hi >= sbits);
    if (ranged && (sbits != 256 || (bit_lo & 31) || (bit_hi & 31) || bit_hi > 256))
        return fail(BLZ_ERR_INVALID_PARAM, "scalar range [%d, %d): 32-bit aligned ranges of 256-bit scalars", bit_lo, bit_hi);
    // (a window table of a ranged handle holds 2^(lo + c j) P: the plan covers hi - lo bits + the carry, no closing doublings)
    P = table_c > 0 ? make_table_plan(npts, table_c, ranged ? bit_hi - bit_lo + 1 : 257)
        : ranged    ? range_plan(curve, npts, bit_lo, bit_hi)
                    : make_plan(npts, sbits, ebits, plan_override("c", 0));
    if (P.c == 0) return fail(BLZ_ERR_INVALID_PARAM, "no window plan for npts=%u sbits=%d%s", npts, sbits, table_c > 0 ? " (window table)" : "");
    if (P.table && !msm_sort3_ok(P, sbits)) return fail(BLZ_ERR_INVALID_PARAM, "window-table task outside the sort's range (c=%d)", P.c);
    P.L = (uint32_t)plan_override("L", (int)P.L);
    if (P.L < 1) P.L = 1;
    if (P.L > (uint32_t)MAX_L) P.L = MAX_L;
    if (ranged_out) *ranged_out = ranged;
    return BLZ_OK;
}

int msm_task_pieces(const MsmPlan& P, int want, bool phased, uint32_t* per_out) {
    if (want < 1 || P.table) want = 1;
    if (want > MSM_MAX_SLICES) want = MSM_MAX_SLICES;
    // pieces of whole 16-point groups (keeps every piece's scalars 16-byte aligned; pf = 8: whole elements)
    // A task whose pieces arrive over the link (phased) ends with HALF a piece: behind the last byte sit that piece's
    // accumulation, the bucket reduce and the tail, and the accumulation is the one part of it that shrinks with the piece
    // (config 2: 13.5 -> 13.0 ms, the lone 2^26 HBM flow 138.6 -> 133); the pieces before it are 1 / (2 k - 1) larger.
    const uint64_t halves = (phased && want >= 4) ? 2ull * want - 1 : 2ull * want;
    const uint32_t per = (uint32_t)(((2ull * P.npts + halves - 1) / halves + 15) & ~(uint64_t)15);
    if (want > 1) want = (int)(((uint64_t)P.npts + per - 1) / per);
    *per_out = want > 1 ? per : P.npts;
    return want;
}

// A task is enqueued in four steps - begin(), then per piece sort_slice() and accumulate_slice(), then end() - so that a
// caller whose inputs arrive over time (msm_stage.hip: host buffers crossing the PCIe link piece by piece, the reference's
// own flow: msm_api.rs:175-202 streams interleaved chunks of scalars and points into the card while it computes) can hand
// each piece to the device when it has landed.  run() is the four steps back to back for inputs that are all there.
//
// A task of ONE piece is the classic pipeline: sort stage (hidden underneath the other slot's accumulation when there is
// one), k_accumulate into per-unit sums, unit folds, bucket reduce over sums[unit_off[g]].  A task of SEVERAL pieces sorts
// and accumulates piece by piece over the same bucket space: the bucket sums live in `bucket_sums`, indexed by bucket;
// k_accumulate_cont resumes a bucket's sum where the previous piece left it (msm_impl.hip.hpp), runs longer than L go through the
// unit folds and k_merge_buckets, and the reduce reads bucket_sums through the identity map.
int MsmEngine::take_slot(int* slot_out) {
    int slot = (rr_cursor + 1) % MSM_QUEUE_DEPTH;
    if (slots[slot].busy) slot = (slot + 1) % MSM_QUEUE_DEPTH;
    if (slots[slot].busy) return fail(BLZ_ERR_INVALID_PARAM, "task queue full (%d tasks in flight)", MSM_QUEUE_DEPTH);
    *slot_out = slot;
    return BLZ_OK;
}

int MsmEngine::step(int slot, int piece, bool curve_kernels, std::optional<MsmStep>& out) {
    BLZ_TRY(use_device(device));
    if (slot < 0 || slot >= MSM_QUEUE_DEPTH || !slots[slot].open) return fail(BLZ_ERR_INVALID_PARAM, "slot %d has no task being enqueued", slot);
    MsmSlot& S = slots[slot];
    if (curve_kernels && S.repr != repr) return fail(BLZ_ERR_INVALID_PARAM, "the handle's arithmetic changed while task %d was being enqueued", slot);
    if (S.slices == 1) piece = -1;
    // a ping-pong task's pieces alternate between the slot's own set and the other slot's; end() reads the slot's own
    const int set = S.sort.where == SortPlan::PINGPONG && piece >= 0 ? (slot + piece) % MSM_QUEUE_DEPTH : slot;
    out.emplace(MsmStep{slot, S, piece, S.plan, sbuf[set], stream, S.sort.where != SortPlan::OPEN ? sort_stream : stream});
    return BLZ_OK;
}

int MsmEngine::begin(uint32_t npts, int sbits, int* slot_out, int table_c, int bit_lo, int bit_hi, int nslices, bool phased) {
    BLZ_TRY(use_device(device));
    const MsmCurveOps* ops = msm_ops_for(curve, repr);
    hipStream_t st = stream;
    if (npts == 0) return fail(BLZ_ERR_INVALID_PARAM, "begin: empty task");
    int slot = -1;
    BLZ_TRY(take_slot(&slot));
    MsmSlot& S = slots[slot];
    MsmPlan P;
    bool ranged = false;
    BLZ_TRY(msm_task_plan(curve, npts, sbits, table_c, bit_lo, bit_hi, P, &ranged));
    const uint64_t G = P.G;
    uint32_t per = npts;
    nslices = msm_task_pieces(P, nslices, phased, &per);
    BLZ_TRY(plan_tail(P, ops->tail, nslices > 1, S.tail));   // (a refusal leaves the slot free)
    // The sort stage's outputs are per slot (SortBufs); the scratch the sorts share is protected by chaining every sort stage
    // behind the one before (last_sort_done).
    // (fits: a build whose register and LDS counts cannot be read is taken to fit; k_accumulate_cont shares k_accumulate's register cap)
    const SortInputs sort_in = {env_int("BLAZE_SORT_HIDE", 1), slots[(slot + 1) % MSM_QUEUE_DEPTH].busy, recent_hot[0] || recent_hot[1],
                                msm_sort_fits_beside(ops->accumulate_vgprs(), msm_sort3_max_vgprs(P.table), ops->accumulate_lds(), msm_sort3_max_lds(P.table))};
    const SortPlan sort = plan_sort(P, npts, sbits, nslices, sort_in);
    BLZ_LOG(2, "msm plan: npts=%u sbits=%d c=%d W=%d Bw=%u G=%llu L=%u pieces=%d sort: %s tail: %s", npts, sbits, P.c, P.W, P.Bw,
            (unsigned long long)G, P.L, nslices, describe(sort).c_str(), describe(S.tail).c_str());
    const uint64_t max_entries = (uint64_t)per * P.W;
    const uint64_t max_units = G + max_entries / P.L + 1;
    if (max_units >= (1ull << 32)) return fail(BLZ_ERR_INVALID_PARAM, "unit bound %llu exceeds 32 bits", (unsigned long long)max_units);

    rr_cursor = slot;
    if (slot_out) *slot_out = slot;
    S.plan = P;
    S.npts = npts;
    S.sbits = sbits;
    S.ranged = ranged;
    S.bit_lo = bit_lo;
    S.bit_hi = bit_hi;
    S.repr = repr;
    S.slices = nslices;
    S.pts_per_slice = per;
    S.max_units = max_units;
    S.sort = sort;
    S.acc_pp_recorded[0] = S.acc_pp_recorded[1] = false;
    S.phased = phased;
    S.task_inputs_event = inputs_event;
    S.accum_timed = false;
    BLZ_HIP(hipEventRecord(S.ev[0], st), BLZ_ERR_UNKNOWN);
    for (int b = 0; b < MSM_QUEUE_DEPTH; ++b) {
        if (b != slot && sort.where != SortPlan::PINGPONG) continue;   // (a ping-pong task's pieces use both slots' sets)
        BLZ_TRY(sbuf[b].count.reserve((G + 1) * 4 + 16));
        BLZ_TRY(sbuf[b].off.reserve((G + 2) * 4));
        BLZ_TRY(sbuf[b].unit_off.reserve((G + 2) * 4));
        BLZ_TRY(sbuf[b].entries.reserve(max_entries * 4));
    }
    BLZ_TRY(blocksums.reserve((size_t)((G + 1 + SCAN_TILE - 1) / SCAN_TILE) * 8));
    if (nslices > 1) {
        const size_t sum_bytes = (size_t)ops->tail.partial_dwords * 4;
        BLZ_TRY(bucket_sums.reserve((G + 1) * sum_bytes));
        BLZ_TRY(bucket_ident.reserve((G + 2) * 4));
        launch_zero(bucket_sums.p, ((G + 1) * sum_bytes + 15) / 16, st);   // all-zero = infinity
        BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    }
    S.open = true;
    S.busy = true;
    return BLZ_OK;
}

// the sort stage of piece `sl`: np points whose scalars start at d_scalars (np x sbits / 8 bytes)
int MsmEngine::sort_slice(int slot, int sl, const void* d_scalars, uint32_t np) {
    std::optional<MsmStep> C;
    BLZ_TRY(step(slot, sl, false, C));
    MsmSlot& S = C->S;
    if (sl < 0 || sl >= S.slices || np == 0 || np > S.pts_per_slice) return fail(BLZ_ERR_INVALID_PARAM, "piece %d of %d with %u points", sl, S.slices, np);
    rr_cursor = slot;
    MsmSlot& O = slots[(slot + 1) % MSM_QUEUE_DEPTH];
    const bool hide = S.sort.where != SortPlan::OPEN, pingpong = S.sort.where == SortPlan::PINGPONG;
    hipStream_t ss = C->sort_stream;
    if (last_sort_done) BLZ_HIP(hipStreamWaitEvent(ss, last_sort_done, 0), BLZ_ERR_UNKNOWN);
    if (hide) {
        // whoever read this buffer set last must have let go of it: the accumulation two pieces back (ping-pong), else the
        // slot's previous task (its level-0 reduce read unit_off last) - and the OTHER slot's last task too if that was a
        // ping-pong task, which borrowed this slot's set
        if (pingpong && S.acc_pp_recorded[sl & 1]) {
            BLZ_HIP(hipStreamWaitEvent(ss, S.ev_acc_pp[sl & 1], 0), BLZ_ERR_UNKNOWN);
        } else {
            if (S.l0_recorded) BLZ_HIP(hipStreamWaitEvent(ss, S.ev_l0, 0), BLZ_ERR_UNKNOWN);
            if (O.sort.where == SortPlan::PINGPONG && O.l0_recorded) BLZ_HIP(hipStreamWaitEvent(ss, O.ev_l0, 0), BLZ_ERR_UNKNOWN);
        }
    }
    BLZ_HIP(hipEventRecord(S.ev_s0, ss), BLZ_ERR_UNKNOWN);   // ev_s0 .. ev_s1: the sort stage, whichever stream it is on
    BLZ_TRY(msm_sort_stage(*this, *C, d_scalars, np));
    hipEvent_t sorted = pingpong ? S.ev_sorted_pp[sl & 1] : S.ev_sorted;
    BLZ_HIP(hipEventRecord(sorted, ss), BLZ_ERR_UNKNOWN);
    last_sort_done = sorted;
    BLZ_HIP(hipEventRecord(S.ev_s1, ss), BLZ_ERR_UNKNOWN);
    // run() (inputs all there before the task began): the staged inputs have been consumed once the LAST sort has read
    // the scalars - and, in DMA mode, once the to-Montgomery pass, which msm_stage.hip enqueued on the MAIN stream ahead of
    // run(), has read the raw points (ev[0] sits behind it): only then may a later task's host -> device copies overwrite
    // this staging set (msm_stage.hip's copy stream waits for the event).  On the sort stream the wait comes last, behind
    // ev_sorted, so it delays nothing but the event.  (Phased tasks: end() records it.)
    if (!S.phased && S.task_inputs_event && sl + 1 == S.slices) {
        if (hide) BLZ_HIP(hipStreamWaitEvent(ss, S.ev[0], 0), BLZ_ERR_UNKNOWN);
        BLZ_HIP(hipEventRecord(S.task_inputs_event, ss), BLZ_ERR_UNKNOWN);
        S.task_inputs_event = nullptr;
    }
    return BLZ_OK;
}

// the accumulation of piece `sl` (its sort stage has been enqueued): d_pts = Montgomery points of the piece's first point
int MsmEngine::accumulate_slice(int slot, int sl, const void* d_pts) {
    std::optional<MsmStep> C;
    BLZ_TRY(step(slot, sl, true, C));
    MsmSlot& S = C->S;
    const MsmCurveOps* ops = msm_ops_for(curve, repr);
    rr_cursor = slot;
    const bool pingpong = S.sort.where == SortPlan::PINGPONG;
    if (S.sort.where != SortPlan::OPEN) BLZ_HIP(hipStreamWaitEvent(stream, pingpong ? S.ev_sorted_pp[sl & 1] : S.ev_sorted, 0), BLZ_ERR_UNKNOWN);
    BLZ_TRY(ops->run_accumulate(*this, *C, d_pts, (uint32_t)S.max_units));
    if (S.slices > 1) BLZ_TRY(ops->merge_buckets(*this, *C));
    if (pingpong) {
        BLZ_HIP(hipEventRecord(S.ev_acc_pp[sl & 1], stream), BLZ_ERR_UNKNOWN);
        S.acc_pp_recorded[sl & 1] = true;
    }
    return BLZ_OK;
}

// every piece is enqueued: bucket reduce + tail
int MsmEngine::end(int slot) {
    std::optional<MsmStep> C;
    BLZ_TRY(step(slot, -1, true, C));
    MsmSlot& S = C->S;
    const MsmCurveOps* ops = msm_ops_for(curve, repr);
    rr_cursor = slot;
    if (S.task_inputs_event) {
        // phased task: every reader of the staged inputs - the pieces' sorts and the caller's to-Montgomery passes - is on
        // the main stream or has been waited for by it
        BLZ_HIP(hipEventRecord(S.task_inputs_event, stream), BLZ_ERR_UNKNOWN);
        S.task_inputs_event = nullptr;
    }
    if (S.slices > 1) {
        hipLaunchKernelGGL(k_iota, dim3(1024), dim3(256), 0, stream, bucket_ident.as<uint32_t>(), S.plan.G + 2);
        BLZ_TRY(ops->run_reduce(*this, *C, bucket_sums.p, bucket_ident.p));
    } else {
        BLZ_TRY(ops->run_reduce(*this, *C, partial.p, C->B.unit_off.p));
    }
    S.l0_recorded = true;
    S.open = false;
    return BLZ_OK;
}

// give up a task whose inputs never arrived in full (a copy failed): what was enqueued runs to completion and is ignored
void MsmEngine::abandon(int slot) {
    if (slot < 0 || slot >= MSM_QUEUE_DEPTH) return;
    MsmSlot& S = slots[slot];
    if (S.busy && S.open) {
        S.busy = false;
        S.open = false;
        S.task_inputs_event = nullptr;
    }
}

int MsmEngine::run(const void* d_pts, const void* d_scalars, uint32_t npts, int sbits, int* slot_out, int table_c, int bit_lo,
                   int bit_hi) {
    BLZ_TRY(use_device(device));
    if (npts == 0) {
        hipStream_t st = stream;
        int slot = -1;
        BLZ_TRY(take_slot(&slot));
        rr_cursor = slot;
        MsmSlot& S = slots[slot];
        if (slot_out) *slot_out = slot;
        BLZ_HIP(hipEventRecord(S.ev[0], st), BLZ_ERR_UNKNOWN);
        BLZ_TRY(msm_ops_for(curve, repr)->emit_infinity(*this, slot));
        for (int i = 1; i <= 4; ++i) BLZ_HIP(hipEventRecord(S.ev[i], st), BLZ_ERR_UNKNOWN);
        BLZ_TRY(copy_words_to_pinned(S.result_h, slot_result(slot), (uint32_t)(3 * fq_bytes(curve) / 4), st));
        BLZ_HIP(hipEventRecord(S.ev_done, st), BLZ_ERR_UNKNOWN);
        S.plan = MsmPlan();
        S.accum_timed = false;
        S.open = false;
        S.busy = true;
        return BLZ_OK;
    }
    // resident inputs: one piece (BLAZE_MSM_PIECES = n forces n: tests of the piecewise path at sizes the oracle checks)
    int pieces = env_int("BLAZE_MSM_PIECES", 1);
    int slot = -1;
    BLZ_TRY(begin(npts, sbits, &slot, table_c, bit_lo, bit_hi, pieces, false));
    if (slot_out) *slot_out = slot;
    MsmSlot& S = slots[slot];
    int rc = BLZ_OK;
    for (int sl = 0; sl < S.slices && rc == BLZ_OK; ++sl) {
        const uint32_t p0 = (uint32_t)sl * S.pts_per_slice;
        const uint32_t np = npts - p0 < S.pts_per_slice ? npts - p0 : S.pts_per_slice;
        rc = sort_slice(slot, sl, (const char*)d_scalars + (size_t)p0 * (sbits / 8), np);
        if (rc == BLZ_OK) rc = accumulate_slice(slot, sl, (const char*)d_pts + (size_t)p0 * mont_point_bytes(curve));
    }
    if (rc == BLZ_OK) rc = end(slot);
    if (rc != BLZ_OK) abandon(slot);
    return rc;
}

int MsmEngine::finish(int slot, uint8_t* out) {
    BLZ_TRY(use_device(device));
    if (slot < 0 || slot >= MSM_QUEUE_DEPTH || !slots[slot].busy) return fail(BLZ_ERR_INVALID_PARAM, "no task in slot %d", slot);
    if (slots[slot].open) return fail(BLZ_ERR_INVALID_PARAM, "task in slot %d never received all of its data", slot);
    MsmSlot& S = slots[slot];
    // bounded: a wedged kernel must not hang the host for ever (common.hpp); on expiry the slot stays busy
    BLZ_TRY(sync_event_bounded(S.ev_done, "wait_result: MSM task"));
    S.busy = false;
    if (S.plan.c) {
        BLZ_LOG(2, "msm: units=%u max_bucket=%u entries=%u", S.stats_h[0], S.stats_h[1], S.stats_h[2]);
        if ((uint64_t)S.stats_h[0] > S.max_units) return fail(BLZ_ERR_UNKNOWN, "unit count %u exceeds its bound", S.stats_h[0]);
        // hot-bucket guard of begin(): this task's largest bucket against the mean of the sort that produced it
        const uint64_t mean = (uint64_t)S.stats_h[2] / (S.plan.G ? S.plan.G : 1) + 1;
        recent_hot[1] = recent_hot[0];
        recent_hot[0] = (uint64_t)S.stats_h[1] > 64 * mean + 4096;
    }
    memcpy(out, S.result_h, 3 * fq_bytes(curve));
    float t = 0;
    (void)hipEventElapsedTime(&t, S.ev[0], S.ev[4]); last_ms[0] = t;
    last_ms[1] = 0;
    if (S.accum_timed && S.plan.c) {
        if (S.slices > 1) {   // piecewise task: the sum of the pieces' k_accumulate_cont launches
            for (int i = 0; i < S.slices; ++i)
                if (hipEventElapsedTime(&t, S.slice_ev[2 * i], S.slice_ev[2 * i + 1]) == hipSuccess) last_ms[1] += t;
        } else {
            (void)hipEventElapsedTime(&t, S.ev[5], S.ev[6]);
            last_ms[1] = t;
        }
    }
    last_sort_hidden = S.sort.where != SortPlan::OPEN && S.plan.c != 0;
    if (S.plan.c) (void)hipEventElapsedTime(&t, S.ev_s0, S.ev_s1);   // the sort stage: on the main stream, or on sort_stream underneath the previous task
    else t = 0;
    last_ms[2] = t;
    (void)hipEventElapsedTime(&t, S.ev[1], S.ev[2]); last_ms[3] = t;
    (void)hipEventElapsedTime(&t, S.ev[2], S.ev[3]); last_ms[4] = t;
    (void)hipEventElapsedTime(&t, S.ev[3], S.ev[4]); last_ms[5] = t;
    last_ms[6] = (float)S.plan.c;
    last_ms[7] = (float)S.plan.W;
    return BLZ_OK;
}

int MsmEngine::combine_partials(const uint8_t* partials, size_t cnt, uint8_t* out, bool on_device) {
    BLZ_TRY(use_device(device));
    return msm_ops_for(curve, repr)->combine(*this, partials, cnt, out, on_device);
}

}  // namespace blz
