// Folds along a resident buffer (blz_ntt_vec_reduce, blz_ntt_vec_scan), templated on the scalar field like the element-wise ops
// whose operands, wire format and 8 x 32-bit arithmetic (field.hip.hpp, vec_canon) they share.  Blocks never wait for one
// another: every dependency between blocks is a separate launch on the handle's stream, as with BLZ_VEC_INV; a result does
// not depend on the order in which blocks run (no atomics).
//
// REDUCE: k_fold_part, at most VEC_MAX_BLOCKS blocks.  Lane g = block x 256 + lane of S = blocks x 256 owns the positions
// g, g + S, g + 2S ... (a wave's loads stay contiguous) and keeps one accumulator; the block's 256 accumulators meet in an LDS
// tree and ONE partial per block goes to the workspace; k_fold_fin, one block, folds the <= 2048 partials into d_out, canonical.
//   SUM   acc += canon(a): no product.
//   DOT   acc += mont(a, canon(b)) = a b / R, below 2m for any 256-bit a: one product per element; the stray 1 / R comes off once,
//         in k_fold_fin (a product by R^2).
//   EVAL  sum_p a[p] z^p = sum_g z^g sum_k a[g + k S] (z^S)^k: Horner along the lane's stride from the top, acc = acc z^S + a[p],
//         one product per element.  The weight z^g = z^lane (z^256)^block is applied once: the LDS tree folds x[t] += z^w x[t + w]
//         for w = 128 .. 1, and k_fold_fin is the same evaluation of the partials at z^256.  The powers z^(2^i) come from
//         squaring z on the device (one lane per block, 19 products, into LDS); the host never sees z.  No power multiplies the
//         term of position 0, so 0^0 = 1.
//
// SCAN: reduce-then-scan over tiles of FOLD_TILE = 1024 positions, lane t owning the FOUR CONSECUTIVE positions 4t .. 4t + 3.
//   k_fold_scan_up    one total per tile (the lane's 3 combines, then a 256-leaf LDS tree);
//   k_fold_scan_down  the tile again with a carry-in: the lane's running values, a 256-wide Kogge-Stone scan of the lanes' totals
//                     in LDS (8 steps), the carry applied to the lane's four values.  Every lane reads what it owns before it
//                     writes it, and owns it alone: dst may be the buffer a names.
//   The totals are scanned (exclusively, in place) by the same two kernels, WIRE = false, level by level: scan_ladder.  No
//   chain is longer than 3 + 8 + 1 combines per level.
//   PROD works in Montgomery form: a raw product chain would pick up a power of 1 / R that depends on the position.  Words are
//   converted on load (mont(x, R^2) is below 2m for any 256-bit x); the way back costs one product per LANE, not per word: the
//   lane's carry-in c R becomes c (a product by the integer 1) and mont(c, v R) = c v is plain already; totals stay in
//   Montgomery form.  SUM takes its words through vec_canon and stores through fp_reduce.
//   Positions past the end of a part-filled tile count as the identity.
//   Nothing is special-cased for zeros: a zero simply stays in every later product.
//
// WORKSPACE: the handle's `scratch`, n x 32 bytes, n = 2^logn, logn >= 1.
//   reduce: blocks = min(ceil(n / 256), 2048) partials.  ceil(n / 256) <= n for every n >= 1.
//   scan:   scan_plan lays it out, scan_ws_words counts it, and a static_assert holds it within n words.
#pragma once
#include <type_traits>

#include "ntt_vec.hip.hpp"

namespace blz {

enum { FOLD_SUM = 0, FOLD_DOT = 1, FOLD_EVAL = 2 };   // enum blz_fold_op
enum { SCAN_SUM = 0, SCAN_PROD = 1 };                 // enum blz_scan_op
constexpr int FOLD_PER_LANE = 4;
static_assert(NTT_FOLD_TILE == (uint64_t)VEC_THREADS * FOLD_PER_LANE, "tile = block x elements per lane");
constexpr int FOLD_LOG_THREADS = 8;
static_assert(VEC_THREADS == 1 << FOLD_LOG_THREADS, "the powers of z are indexed by log2 of a lane distance");
constexpr int FOLD_POWERS = 20;   // z^(2^i), i < 20: the largest is the stride of 2048 blocks x 256 lanes
static_assert(VEC_MAX_BLOCKS * VEC_THREADS == 1u << (FOLD_POWERS - 1), "z^S of the widest grid is the last power");

// ---- what the blocks of a fold, a scan and a weighted scan share
// pw[i] = z^(2^i) in Montgomery form, i < npow: the squaring chain; ONE lane calls it
template <class Fr>
BLZ_DEV void fold_square_chain(uint32_t* pw, const uint32_t* z, int npow) {
    Fp<Fr> p;
    fp_load(p, z);
    fp_to_mont(p, p);
    fp_store(pw, p);
#pragma unroll 1
    for (int i = 1; i < npow; ++i) {
        fp_sqr(p, p);
        fp_store(pw + i * 8, p);
    }
}

// The lanes' 256 values -> x[0] in LDS: x[t] = combine(x[t], x[t + w], log2 w) for w = 128 .. 1.  Every lane calls it.
template <class Fr, class Combine>
BLZ_DEV void fold_block_tree(uint32_t* x, const Fp<Fr>& v, Combine&& combine) {
    using E = Fp<Fr>;
    const uint32_t t = threadIdx.x;
    fp_store(x + t * 8, v);
    __syncthreads();
    int lw = FOLD_LOG_THREADS - 1;
#pragma unroll 1
    for (uint32_t w = VEC_THREADS / 2; w >= 1; w >>= 1, --lw) {
        if (t < w) {
            E l, r;
            fp_load(l, x + t * 8);
            fp_load(r, x + (t + w) * 8);
            combine(l, r, lw);
            fp_store(x + t * 8, l);
        }
        __syncthreads();
    }
}

// pw[i] = z^(2^i) in Montgomery form, i < FOLD_POWERS (LDS); every lane calls it, lane 0 squares
template <class Fr>
BLZ_DEV void fold_powers(uint32_t* pw, const uint32_t* z) {
    if (threadIdx.x == 0) fold_square_chain<Fr>(pw, z, FOLD_POWERS);
    __syncthreads();
}

// the block's accumulators -> x[0] in LDS.  EVAL: x[t] += z^(w 2^base) x[t + w], so x[0] = sum_t (z^(2^base))^t acc_t
template <class Fr, bool EVAL>
BLZ_DEV void fold_tree(uint32_t* x, const uint32_t* pw, int base, const Fp<Fr>& acc) {
    fold_block_tree<Fr>(x, acc, [&](Fp<Fr>& l, Fp<Fr>& r, int lw) {
        if constexpr (EVAL) {
            Fp<Fr> zw;
            fp_load(zw, pw + (base + lw) * 8);
            fp_mul(r, r, zw);
        }
        fp_add(l, l, r);
    });
}

// partial[block] = the fold of the positions the block's lanes own (DOT: with the stray 1 / R; EVAL: short of the block's weight)
template <class Fr, int OP>
__global__ __launch_bounds__(VEC_THREADS) void k_fold_part(uint32_t* partial, NttVecArg a, NttVecArg b, uint64_t n, int log_stride) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    __shared__ __attribute__((aligned(16))) uint32_t pw[(OP == FOLD_EVAL ? FOLD_POWERS : 1) * 8];
    const uint64_t stride = 1ull << log_stride;   // gridDim.x * VEC_THREADS, a power of two
    const uint64_t g = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    E acc;
    fp_zero(acc);
    if constexpr (OP == FOLD_EVAL) {
        fold_powers<Fr>(pw, b.p);
        E zs;
        fp_load(zs, pw + log_stride * 8);
        // n and the stride are powers of two: a lane below n owns max(n / stride, 1) positions, all below n
        if (g < n) {
#pragma unroll 1
            for (uint64_t k = n > stride ? n >> log_stride : 1; k-- > 0;) {
                E v;
                fp_load(v, a.p + ((g + (k << log_stride)) & a.mask) * 8);
                vec_canon(v);
                fp_mul(acc, acc, zs);
                fp_add(acc, acc, v);
            }
        }
    } else {
#pragma unroll 1
        for (uint64_t e = g; e < n; e += stride) {
            E v;
            fp_load(v, a.p + (e & a.mask) * 8);
            if constexpr (OP == FOLD_DOT) {
                E y;
                fp_load(y, b.p + (e & b.mask) * 8);
                vec_canon(y);
                fp_mul(v, v, y);
            } else {
                vec_canon(v);
            }
            fp_add(acc, acc, v);
        }
    }
    fold_tree<Fr, OP == FOLD_EVAL>(x, pw, 0, acc);
    vec_copy32(partial + (size_t)blockIdx.x * 8, x);
}

// out = the fold of `count` partials (a power of two, <= VEC_MAX_BLOCKS), canonical; one block
template <class Fr, int OP>
__global__ __launch_bounds__(VEC_THREADS) void k_fold_fin(uint32_t* out, const uint32_t* partial, uint32_t count, NttVecArg b) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    __shared__ __attribute__((aligned(16))) uint32_t pw[(OP == FOLD_EVAL ? FOLD_POWERS : 1) * 8];
    const uint32_t t = threadIdx.x;
    E acc;
    fp_zero(acc);
    if constexpr (OP == FOLD_EVAL) {
        // partial j weighs (z^256)^j: Horner with (z^256)^256 along the lane's stride, the tree with the powers from z^256 up
        fold_powers<Fr>(pw, b.p);
        E zs;
        fp_load(zs, pw + 2 * FOLD_LOG_THREADS * 8);
        if (t < count) {
#pragma unroll 1
            for (uint32_t k = count > VEC_THREADS ? count >> FOLD_LOG_THREADS : 1; k-- > 0;) {
                E v;
                fp_load(v, partial + (size_t)(t + (k << FOLD_LOG_THREADS)) * 8);
                fp_mul(acc, acc, zs);
                fp_add(acc, acc, v);
            }
        }
    } else {
#pragma unroll 1
        for (uint32_t e = t; e < count; e += VEC_THREADS) {
            E v;
            fp_load(v, partial + (size_t)e * 8);
            fp_add(acc, acc, v);
        }
    }
    fold_tree<Fr, OP == FOLD_EVAL>(x, pw, FOLD_LOG_THREADS, acc);
    if (t == 0) {
        E r;
        fp_load(r, x);
        if constexpr (OP == FOLD_DOT) fp_to_mont(r, r);   // (sum a b / R) R^2 / R
        fp_reduce(r);
        fp_store(out, r);
    }
}

// ---- scans
template <class Fr, int OP>
BLZ_DEV void scan_identity(Fp<Fr>& r) {
    if constexpr (OP == SCAN_PROD) fp_one(r); else fp_zero(r);
}
template <class Fr, int OP>
BLZ_DEV void scan_combine(Fp<Fr>& r, const Fp<Fr>& a, const Fp<Fr>& b) {
    if constexpr (OP == SCAN_PROD) fp_mul(r, a, b); else fp_add(r, a, b);
}
// the lane's four consecutive elements in the scan's own form (WIRE: from 256-bit words; else as an earlier level left them),
// the identity past `count`
template <class Fr, int OP, bool WIRE>
BLZ_DEV void scan_load(Fp<Fr> (&x)[FOLD_PER_LANE], NttVecArg a, uint64_t first, uint64_t count) {
#pragma unroll
    for (int j = 0; j < FOLD_PER_LANE; ++j) {
        const uint64_t e = first + j;
        if (e < count) {
            fp_load(x[j], a.p + (e & a.mask) * 8);
            if constexpr (WIRE) {
                if constexpr (OP == SCAN_PROD) fp_to_mont(x[j], x[j]); else vec_canon(x[j]);
            }
        } else {
            scan_identity<Fr, OP>(x[j]);
        }
    }
}
// WIRE: canonical on the way out
template <class Fr, bool WIRE>
BLZ_DEV void scan_store(uint32_t* p, const Fp<Fr>& v) {
    Fp<Fr> r = v;
    if constexpr (WIRE) fp_reduce(r);
    fp_store(p, r);
}

// totals[tile] = the fold of the tile's elements, in the scan's own form
template <class Fr, int OP, bool WIRE>
__global__ __launch_bounds__(VEC_THREADS) void k_fold_scan_up(uint32_t* totals, NttVecArg a, uint64_t count) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint32_t t = threadIdx.x;
    E v[FOLD_PER_LANE];
    scan_load<Fr, OP, WIRE>(v, a, (uint64_t)blockIdx.x * NTT_FOLD_TILE + (uint64_t)t * FOLD_PER_LANE, count);
#pragma unroll
    for (int j = 1; j < FOLD_PER_LANE; ++j) scan_combine<Fr, OP>(v[0], v[0], v[j]);
    fold_block_tree<Fr>(x, v[0], [](E& l, const E& r, int) { scan_combine<Fr, OP>(l, l, r); });
    vec_copy32(totals + (size_t)blockIdx.x * 8, x);
}

// dst[e] = carry[tile] o a[tile's first] o .. o a[e] (exclusive: .. o a[e - 1]), e < count; carry == nullptr: the identity (the
// single tile of a one-block scan).  total (nullable): the last tile's last inclusive value, in wire form.  dst may be a.p.
template <class Fr, int OP, bool WIRE>
__global__ __launch_bounds__(VEC_THREADS) void k_fold_scan_down(uint32_t* dst, NttVecArg a, const uint32_t* carry, uint64_t count,
                                                                 uint32_t exclusive, uint32_t* total) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * NTT_FOLD_TILE + (uint64_t)t * FOLD_PER_LANE;
    E v[FOLD_PER_LANE];
    scan_load<Fr, OP, WIRE>(v, a, first, count);
#pragma unroll
    for (int j = 1; j < FOLD_PER_LANE; ++j) scan_combine<Fr, OP>(v[j], v[j - 1], v[j]);   // the lane's inclusive values
    // Kogge-Stone over the lanes' totals: after the step of distance d, x[t] folds the lanes t - 2d + 1 .. t
    E s = v[FOLD_PER_LANE - 1];
    fp_store(x + t * 8, s);
    __syncthreads();
#pragma unroll 1
    for (uint32_t d = 1; d < VEC_THREADS; d <<= 1) {
        E o;
        if (t >= d) fp_load(o, x + (t - d) * 8); else scan_identity<Fr, OP>(o);
        __syncthreads();
        scan_combine<Fr, OP>(s, o, s);
        fp_store(x + t * 8, s);
        __syncthreads();
    }
    // what precedes the lane: the tile's carry-in and the lanes below
    E c, below;
    if (carry) fp_load(c, carry + (size_t)blockIdx.x * 8); else scan_identity<Fr, OP>(c);
    if (t > 0) fp_load(below, x + (t - 1) * 8); else scan_identity<Fr, OP>(below);
    scan_combine<Fr, OP>(c, c, below);
    // the way back from Montgomery form, once per lane: c / R times an element's v R is their plain product
    if constexpr (WIRE && OP == SCAN_PROD) vec_strip_mont(c);
    E last = c;   // the value before the lane's first element; then the inclusive value of each
#pragma unroll
    for (int j = 0; j < FOLD_PER_LANE; ++j) {
        E inc;
        scan_combine<Fr, OP>(inc, c, v[j]);
        if (first + j < count) scan_store<Fr, WIRE>(dst + (first + j) * 8, exclusive ? last : inc);
        last = inc;
    }
    if (total && blockIdx.x == gridDim.x - 1 && t == VEC_THREADS - 1) scan_store<Fr, true>(total, last);
}

inline int fold_log2(uint64_t v) {
    int l = 0;
    while ((1ull << l) < v) ++l;
    return l;
}

template <class Fr>
int ntt_vec_reduce_t(hipStream_t st, int op, uint32_t* out, NttVecArg a, NttVecArg b, uint64_t n, uint32_t* ws) {
    uint64_t blocks = (n + VEC_THREADS - 1) / VEC_THREADS;   // a power of two: n is
    if (blocks > VEC_MAX_BLOCKS) blocks = VEC_MAX_BLOCKS;
    const int ls = fold_log2(blocks) + FOLD_LOG_THREADS;
    const dim3 grid((unsigned)blocks), one(1), thr(VEC_THREADS);
    switch (op) {
        case FOLD_SUM:
            hipLaunchKernelGGL((k_fold_part<Fr, FOLD_SUM>), grid, thr, 0, st, ws, a, a, n, ls);
            hipLaunchKernelGGL((k_fold_fin<Fr, FOLD_SUM>), one, thr, 0, st, out, (const uint32_t*)ws, (uint32_t)blocks, a);
            break;
        case FOLD_DOT:
            hipLaunchKernelGGL((k_fold_part<Fr, FOLD_DOT>), grid, thr, 0, st, ws, a, b, n, ls);
            hipLaunchKernelGGL((k_fold_fin<Fr, FOLD_DOT>), one, thr, 0, st, out, (const uint32_t*)ws, (uint32_t)blocks, b);
            break;
        case FOLD_EVAL:
            hipLaunchKernelGGL((k_fold_part<Fr, FOLD_EVAL>), grid, thr, 0, st, ws, a, b, n, ls);
            hipLaunchKernelGGL((k_fold_fin<Fr, FOLD_EVAL>), one, thr, 0, st, out, (const uint32_t*)ws, (uint32_t)blocks, b);
            break;
        default: return fail(BLZ_ERR_INVALID_PARAM, "unknown reduction %d", op);
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

// ---- the ladder of a tiled scan (the scans here, the weighted scans of ntt_horner.hip.hpp)
// One tile: a single down launch.  More: up over the tiles, the totals scanned exclusively in place - by one block while they
// fill one tile, else through a second level (n > 2^20; at most 128 totals of the totals at 2^27) -, down over the tiles with
// the totals as carries.  scan_plan alone lays the workspace out: `tiles` totals, `tiles2` behind them, the op's own at `free`.
struct ScanPlan {
    uint64_t tiles = 1, tiles2 = 0, words = 0;   // tiles2 == 0: no second level; words: the 32-byte words the levels take
    uint32_t *t1 = nullptr, *t2 = nullptr, *free = nullptr;
};
constexpr ScanPlan scan_plan(uint64_t n, uint32_t* ws) {   // ws == nullptr: the counts only
    ScanPlan p;
    p.tiles = (n + NTT_FOLD_TILE - 1) / NTT_FOLD_TILE;
    if (p.tiles == 1) return p;   // one block, no carry, no workspace
    p.tiles2 = p.tiles > NTT_FOLD_TILE ? (p.tiles + NTT_FOLD_TILE - 1) / NTT_FOLD_TILE : 0;
    p.words = p.tiles + p.tiles2;
    if (ws) p.t1 = ws, p.t2 = ws + p.tiles * 8, p.free = ws + p.words * 8;
    return p;
}
// the words of workspace a scan of 2^logn elements takes (a weighted scan keeps logn powers of z at `free`): n exist
constexpr uint64_t scan_ws_words(int logn, bool horner) {
    const ScanPlan p = scan_plan(1ull << logn, nullptr);
    return p.words + (horner && p.tiles > 1 ? (uint64_t)logn : 0);
}
constexpr bool scan_ws_fits(int logn) {   // ... for every size up to 2^logn, and one block scans the top level
    return logn < 1 || (scan_ws_words(logn, true) <= 1ull << logn && scan_plan(1ull << logn, nullptr).tiles2 <= NTT_FOLD_TILE &&
                        scan_ws_fits(logn - 1));
}
static_assert(scan_ws_fits(NTT_MAX_LOG), "the handle's scratch (n words) holds every level of a scan and a weighted scan's powers");

struct ScanLevel {   // 0 = the wire (a -> dst), 1 = the totals, 2 = the totals of the totals (both in place)
    int level; NttVecArg src; uint32_t* dst; uint64_t count;
    dim3 grid() const { return dim3((unsigned)((count + NTT_FOLD_TILE - 1) / NTT_FOLD_TILE)); }   // a block per tile
};
// up(wire, level, totals): one total per tile of the level;  down(wire, level, carry): the level's scan, carry nullable.
// `wire` is std::true_type at level 0 and std::false_type above: the kernels' WIRE.
template <class Up, class Down>
void scan_ladder(const ScanPlan& p, uint32_t* dst, NttVecArg a, uint64_t n, Up&& up, Down&& down) {
    constexpr std::true_type wire{};
    constexpr std::false_type totals{};
    const uint32_t* const none = nullptr;
    const ScanLevel l0{0, a, dst, n}, l1{1, {p.t1, ~0ull}, p.t1, p.tiles}, l2{2, {p.t2, ~0ull}, p.t2, p.tiles2};
    if (p.tiles == 1) return down(wire, l0, none);
    up(wire, l0, p.t1);
    if (p.tiles2 != 0) {
        up(totals, l1, p.t2);
        down(totals, l2, none);
    }
    down(totals, l1, p.tiles2 != 0 ? (const uint32_t*)p.t2 : none);
    down(wire, l0, (const uint32_t*)p.t1);
}

template <class Fr, int OP>
void scan_launch(hipStream_t st, uint32_t* dst, NttVecArg a, uint64_t n, uint32_t exclusive, uint32_t* total, uint32_t* ws) {
    const dim3 thr(VEC_THREADS);
    scan_ladder(
        scan_plan(n, ws), dst, a, n,
        [&](auto wire, const ScanLevel& l, uint32_t* totals) {
            hipLaunchKernelGGL((k_fold_scan_up<Fr, OP, decltype(wire)::value>), l.grid(), thr, 0, st, totals, l.src, l.count);
        },
        [&](auto wire, const ScanLevel& l, const uint32_t* carry) {   // the levels above the wire: exclusive, no total
            hipLaunchKernelGGL((k_fold_scan_down<Fr, OP, decltype(wire)::value>), l.grid(), thr, 0, st, l.dst, l.src, carry, l.count,
                               l.level ? 1u : exclusive, l.level ? nullptr : total);
        });
}

template <class Fr>
int ntt_vec_scan_t(hipStream_t st, int op, uint32_t flags, uint32_t* dst, NttVecArg a, uint64_t n, uint32_t* total, uint32_t* ws) {
    const uint32_t exclusive = flags & 1u;
    switch (op) {
        case SCAN_SUM: scan_launch<Fr, SCAN_SUM>(st, dst, a, n, exclusive, total, ws); break;
        case SCAN_PROD: scan_launch<Fr, SCAN_PROD>(st, dst, a, n, exclusive, total, ws); break;
        default: return fail(BLZ_ERR_INVALID_PARAM, "unknown scan %d", op);
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
