// Round polynomials on resident tables (blz_ntt_vec_mle_round, blz_ntt_sumcheck_step): ONE kernel, k_sc_round, over a pair source
// and a gate.  Same house rules as ntt_mle.hip.hpp: 256 lanes, the 8 x 32-bit arithmetic of field.hip.hpp through vec_canon, no
// atomics, no flags, no allocation, every dependency between blocks is a launch.
//
// ROUND  out[t] = sum over the pairs of G(..., lo_j + t (hi_j - lo_j), ...), t < points <= 4, one accumulator per point.
//   The grid of k_fold_part: lane g of S = blocks x 256 owns the work items g, g + S, ...  Per item the source yields (value,
//   difference) per table, ONE TABLE AT A TIME - only that pair of a table stays in registers -, then the gate is evaluated at
//   `points` points: the loop over t is unrolled to 4 and predicated on `points`, which is wave-uniform, and t advances by ONE
//   addition per table.
//
// GATES  PRODUCT  G = a, a b or a b c      (K = 1 .. 3 tables)   points x (K - 1) products per item
//        R1CS     G = a (b c - d)          (K = 4: eq, Az, Bz, Cz)   2 + 2 points products per item
//   Montgomery factors: each raw product leaves a factor 1 / R.  PRODUCT carries R^-(K-1) on every term of a sum.  R1CS: d's pair
//   (value and difference) is scaled by 1 / R ONCE per item (two products by the integer 1), so b c / R - d / R is one subtraction
//   and a times it carries R^-2 on every term - the stray power of a K = 3 product.  Either way the power comes off ONCE, where
//   the final word is made (mle_round_close: K - 1 products by R^2, DOT's rule), so one finish kernel serves every gate.
//
// SOURCES
//   ScPairs<LOW>  (no r: vec_mle_round, a sumcheck's first round)  the item is the pair p of len / 2: mle_pair's (p, p + len / 2),
//     or (2p, 2p + 1) with LOW; 2 loads through vec_canon per table, tables may be periodic, nothing is written to a table.
//     Products per pair at PRODUCT: none at K = 1, 3 at K = 2 with 3 points, 8 at K = 3 with 4.
//   ScQuads  (r: bind the top variable of every table IN PLACE and take the next round in the same pass)  the item is the quad q of
//     Q = len / 4.  Per table it loads the words q, q + Q, q + 2Q, q + 3Q, makes the two folded words lo' = w0 + r (w2 - w0) and
//     hi' = w1 + r (w3 - w1) - r in Montgomery form once per lane, as in k_mle_fold: one product per folded word, plain already -
//     and stores them canonical at q and q + Q.  No other lane reads or writes those four positions, which is why in place is
//     free.  (q, q + Q) of the folded table of length len / 2 is exactly the pair a round would read, so the folded words never
//     come back from memory: the unfused sequence (a k_mle_fold per table, then a round over the halves) moves 1.5 len words per
//     table and reads len / 2 per table again; the step moves 1.5 len per table and nothing more, in one op.
//     Products per quad: 2 K for the fold plus the gate's - PRODUCT K = 1: 2;  K = 2, 3 points: 7;  K = 3, 4 points: 14;  R1CS,
//     4 points: 8 + 2 + 8 = 18 against 20 for the six ops it replaces (8 in the four folds, 8 in round(eq, Az, Bz; 4), 4 in
//     round(eq, Cz; 4)).
//     Registers: four accumulators, the tables' (value, difference) pairs and r are 8 (2 K + 5) VGPRs live across the gate - 104
//     at R1CS before a product's own temporaries.  The compiler reports 192 - 201 VGPRs for the R1CS bind and 167 - 170 at K = 3
//     (two waves per SIMD), no scratch; asked for three waves (168) it spills 44 and 12 bytes per lane, so it is not asked.
//
// BIND ONLY  (points == 0: a sumcheck's last variable) K launches of k_mle_fold, in place, in the one enqueue (sc_bind_only).
//
// REDUCTION and launch geometry, of k_sc_round and of k_gate_round (ntt_gate.hip.hpp) alike: sc_plan and sc_finish.  One
//   fold_block_tree per point.  A call whose items fit one block - len <= 1024 with r, len <= 512 without - closes the sums there
//   and writes d_out itself: no workspace, which small handles do not have (4 words need n >= 4).  Any other writes one partial per
//   block and point, word t x blocks + block of the handle's scratch, and k_mle_round_fin, one block, folds and closes them.
//   Workspace: blocks x points words with blocks = min(len / 1024, 2048) (len / 512 without r) >= 2 and points <= 6 (a caller's
//   gate; 4 here): at most 6 len / 512 < len <= n.
#pragma once
#include <algorithm>

#include "ntt_mle.hip.hpp"

namespace blz {

enum { SC_GATE_PRODUCT = 0, SC_GATE_R1CS = 1 };   // BLZ_GATE_PRODUCT, BLZ_GATE_R1CS
constexpr int SC_MAX_TABLES = 4;
// a call's tables; the slots past the gate's K are not looked at.  ScQuads writes through p: at least len words each
struct ScOperands { NttVecArg t[SC_MAX_TABLES]; };

// the stray power of 1 / R on a gate's terms, as a number of operands of a product
template <int GATE, int K>
constexpr int sc_close_k() { return GATE == SC_GATE_R1CS ? 3 : K; }

// A pair source: pair() yields one table's value at t = 0 and its difference for work item i of `work`; BINDS: it takes r
template <bool LOW>
struct ScPairs {
    static constexpr bool BINDS = false;
    template <class Fr>
    static BLZ_DEV void pair(Fp<Fr>& lo, Fp<Fr>& diff, NttVecArg a, uint64_t p, uint64_t half, const Fp<Fr>&) {
        mle_pair<Fr, LOW>(lo, diff, a, p, half);
    }
};

// One quad of one table, folded in place: lo = the new word q, diff = the new word q + Q minus it
struct ScQuads {
    static constexpr bool BINDS = true;
    template <class Fr>
    static BLZ_DEV void pair(Fp<Fr>& lo, Fp<Fr>& diff, NttVecArg a, uint64_t q, uint64_t quarter, const Fp<Fr>& rm) {
        uint32_t* const t = const_cast<uint32_t*>(a.p);
        Fp<Fr> hi, w;
        fp_load(lo, t + q * 8);
        fp_load(w, t + (q + 2 * quarter) * 8);
        vec_canon(lo);
        vec_canon(w);
        fp_sub(w, w, lo);
        fp_mul(w, w, rm);
        fp_add(lo, lo, w);
        fp_reduce(lo);
        fp_load(hi, t + (q + quarter) * 8);
        fp_load(w, t + (q + 3 * quarter) * 8);
        vec_canon(hi);
        vec_canon(w);
        fp_sub(w, w, hi);
        fp_mul(w, w, rm);
        fp_add(hi, hi, w);
        fp_reduce(hi);
        fp_store(t + q * 8, lo);
        fp_store(t + (q + quarter) * 8, hi);
        fp_sub(diff, hi, lo);
    }
};

// acc[t] += G at t = 0 .. points - 1; v0: the tables' values at t = 0, d: their differences (R1CS: d's pair scaled by 1 / R).
// t advances on a copy of the values, not through the reference: advancing the kernel's own array costs the K = 1 pair rounds 3 - 4
// VGPRs, and BN254's with LOW (77) would cross 80, a wave per SIMD
template <class Fr, int GATE, int K>
BLZ_DEV void sc_gate_points(Fp<Fr> (&acc)[MLE_MAX_POINTS], const Fp<Fr> (&v0)[K], const Fp<Fr> (&d)[K], uint32_t points) {
    using E = Fp<Fr>;
    E v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = v0[j];
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) {
        if (t < (int)points) {
            E pr;
            if constexpr (GATE == SC_GATE_R1CS) {
                fp_mul(pr, v[1], v[2]);
                fp_sub(pr, pr, v[3]);
                fp_mul(pr, v[0], pr);
            } else {
                pr = v[0];
#pragma unroll
                for (int j = 1; j < K; ++j) fp_mul(pr, pr, v[j]);
            }
            fp_add(acc[t], acc[t], pr);
            if (t + 1 < MLE_MAX_POINTS) {
#pragma unroll
                for (int j = 0; j < K; ++j) fp_add(v[j], v[j], d[j]);
            }
        }
    }
}

// x R^-(K-1) -> x, canonical: K - 1 products by R^2
template <class Fr>
BLZ_DEV void mle_round_close(Fp<Fr>& x, int k) {
#pragma unroll 1
    for (int j = 1; j < k; ++j) fp_to_mont(x, x);
    fp_reduce(x);
}

// The block's accumulators: direct != 0 (one block): out = d_out, `points` canonical words; else out = the workspace, word
// t * gridDim.x + block = the block's partial of point t, with the stray power of 1 / R
template <class Fr, int NP>
BLZ_DEV void sc_block_sums(uint32_t* x, uint32_t* out, const Fp<Fr> (&acc)[NP], uint32_t points, uint32_t direct, int close_k) {
    using E = Fp<Fr>;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
        if (t < (int)points) {
            fold_block_tree<Fr>(x, acc[t], [](E& l, const E& r, int) { fp_add(l, l, r); });
            if (direct) {
                if (threadIdx.x == 0) {
                    E s;
                    fp_load(s, x);
                    mle_round_close(s, close_k);
                    fp_store(out + t * 8, s);
                }
            } else {
                vec_copy32(out + ((size_t)t * gridDim.x + blockIdx.x) * 8, x);
            }
            __syncthreads();   // x is the next point's
        }
    }
}

// r: one device word, read only where the source binds; work: the pairs (quads) of the call
template <class Fr, class Source, int GATE, int K>
__global__ __launch_bounds__(VEC_THREADS) void k_sc_round(uint32_t* out, ScOperands tb, const uint32_t* r, uint64_t work, int log_stride,
                                                           uint32_t points, uint32_t direct) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint64_t stride = 1ull << log_stride;   // gridDim.x * VEC_THREADS, a power of two
    E rm;
    if constexpr (Source::BINDS) {
        fp_load(rm, r);
        fp_to_mont(rm, rm);
    }
    E acc[MLE_MAX_POINTS];
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) fp_zero(acc[t]);
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; i < work; i += stride) {
        E v[K], d[K];
#pragma unroll
        for (int j = 0; j < K; ++j) Source::template pair<Fr>(v[j], d[j], tb.t[j], i, work, rm);
        if constexpr (GATE == SC_GATE_R1CS) {
            vec_strip_mont(v[3]);
            vec_strip_mont(d[3]);
        }
        sc_gate_points<Fr, GATE, K>(acc, v, d, points);
    }
    sc_block_sums<Fr>(x, out, acc, points, direct, sc_close_k<GATE, K>());
}

// out[t] = the fold of the `count` partials of point t (a power of two, <= VEC_MAX_BLOCKS), closed; one block
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_mle_round_fin(uint32_t* out, const uint32_t* partial, uint32_t count, uint32_t points, int k) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
#pragma unroll 1
    for (uint32_t t = 0; t < points; ++t) {
        E acc;
        fp_zero(acc);
#pragma unroll 1
        for (uint32_t e = threadIdx.x; e < count; e += VEC_THREADS) {
            E v;
            fp_load(v, partial + ((size_t)t * count + e) * 8);
            fp_add(acc, acc, v);
        }
        fold_block_tree<Fr>(x, acc, [](E& l, const E& r, int) { fp_add(l, l, r); });
        if (threadIdx.x == 0) {
            E s;
            fp_load(s, x);
            mle_round_close(s, k);
            fp_store(out + t * 8, s);
        }
        __syncthreads();
    }
}

using ScRoundKernel = void (*)(uint32_t*, ScOperands, const uint32_t*, uint64_t, int, uint32_t, uint32_t);

// the gate's instantiation for the call's source: quads with r, else pairs - MLE_LOW's only for PRODUCT
template <class Fr, int GATE, int K>
ScRoundKernel sc_round_kernel(bool bind, bool low) {
    if (bind) return &k_sc_round<Fr, ScQuads, GATE, K>;
    if constexpr (GATE == SC_GATE_PRODUCT)
        if (low) return &k_sc_round<Fr, ScPairs<true>, GATE, K>;
    return &k_sc_round<Fr, ScPairs<false>, GATE, K>;
}

// The launch of a round kernel over a call's items: work quads (bind) or pairs, blocks a power of two as work is, direct: one
// block, which writes d_out itself
struct ScPlan {
    uint64_t work; unsigned blocks; int log_stride; uint32_t direct;
    uint32_t* sums(uint32_t* out, uint32_t* ws) const { return direct ? out : ws; }   // where the round kernel writes
};
inline ScPlan sc_plan(bool bind, uint64_t len) {
    const uint64_t work = bind ? len >> 2 : len >> 1;
    const uint64_t blocks = std::min<uint64_t>((work + VEC_THREADS - 1) / VEC_THREADS, VEC_MAX_BLOCKS);
    return {work, (unsigned)blocks, fold_log2(blocks) + FOLD_LOG_THREADS, blocks == 1 ? 1u : 0u};
}

// the bind alone: each of the k tables folded in place by vec_mle_fold's launcher
template <class Fr>
int sc_bind_only(hipStream_t st, int k, const NttVecArg* t, const uint32_t* r, uint64_t len) {
    for (int j = 0; j < k; ++j) BLZ_TRY(ntt_vec_mle_fold_t<Fr>(st, 0, const_cast<uint32_t*>(t[j].p), t[j], r, len));
    return BLZ_OK;
}

// behind the round kernel's launch: the partials in ws folded and closed into out unless the one block has done it
template <class Fr>
int sc_finish(hipStream_t st, const ScPlan& p, uint32_t* out, const uint32_t* ws, uint32_t points, int close_k) {
    if (!p.direct) hipLaunchKernelGGL(k_mle_round_fin<Fr>, dim3(1), dim3(VEC_THREADS), 0, st, out, ws, (uint32_t)p.blocks, points, close_k);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

// t: the gate's k tables (PRODUCT 1 .. 3, R1CS 4).  r != nullptr: every table holds at least len words, no two overlap, and
// their first len / 2 words are written; points == 0: bind only (len >= 2), else len >= 4.  r == nullptr: round only, tables
// may be periodic, 1 <= points; flags: MLE_LOW, honoured for PRODUCT without r alone.  out: `points` words; ws: the handle's scratch
template <class Fr>
int ntt_sumcheck_step_t(hipStream_t st, uint32_t gate, uint32_t flags, int k, const NttVecArg* t, const uint32_t* r, uint32_t points, uint64_t len,
                        uint32_t* out, uint32_t* ws) {
    if (r && points == 0) return sc_bind_only<Fr>(st, k, t, r, len);
    const ScPlan p = sc_plan(r != nullptr, len);
    const bool low = (flags & MLE_LOW) != 0;
    ScOperands tb{};
    for (int j = 0; j < k && j < SC_MAX_TABLES; ++j) tb.t[j] = t[j];
    ScRoundKernel kernel;
    if (gate == SC_GATE_R1CS) {
        kernel = sc_round_kernel<Fr, SC_GATE_R1CS, 4>(r != nullptr, false);
    } else {
        switch (k) {
            case 1: kernel = sc_round_kernel<Fr, SC_GATE_PRODUCT, 1>(r != nullptr, low); break;
            case 2: kernel = sc_round_kernel<Fr, SC_GATE_PRODUCT, 2>(r != nullptr, low); break;
            case 3: kernel = sc_round_kernel<Fr, SC_GATE_PRODUCT, 3>(r != nullptr, low); break;
            default: return fail(BLZ_ERR_INVALID_PARAM, "a product gate takes 1 to %d tables", MLE_MAX_OPERANDS);
        }
    }
    hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(VEC_THREADS), 0, st, p.sums(out, ws), tb, r, p.work, p.log_stride, points, p.direct);
    return sc_finish<Fr>(st, p, out, ws, points, gate == SC_GATE_R1CS ? 3 : k);
}

}  // namespace blz
