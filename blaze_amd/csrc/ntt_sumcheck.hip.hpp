// A sumcheck step on resident tables (blz_ntt_sumcheck_step): bind the top variable of every table to r IN PLACE and take the
// next round polynomial of a gate over the folded tables in the same pass.  The fold's output is the next round's input, so the
// folded words never come back from memory: per round at live length len the unfused sequence (a k_mle_fold per table, then
// k_mle_round_part over the halves) moves 1.5 len words per table and reads len / 2 per table again; the step moves 1.5 len per
// table and nothing more, in one op.  Same house rules as ntt_mle.hip.hpp: 256 lanes, the 8 x 32-bit arithmetic of
// field.hip.hpp through vec_canon, no atomics, no flags, no allocation, every dependency between blocks is a launch.
//
// GATES  PRODUCT  G = a, a b or a b c      (K = 1 .. 3 tables)
//        R1CS     G = a (b c - d)          (K = 4: eq, Az, Bz, Cz)
//
// BIND + ROUND  k_sc_bind<Fr, GATE, K>: the grid of k_fold_part over the QUADS - lane g of S = blocks x 256 owns the quads
//   g, g + S, ... of Q = len / 4.  Per table it loads the words q, q + Q, q + 2Q, q + 3Q, makes the two folded words
//   lo' = w0 + r (w2 - w0) and hi' = w1 + r (w3 - w1) - r in Montgomery form once per lane, as in k_mle_fold: one product per
//   folded word, plain already - and stores them canonical at q and q + Q.  No other lane reads or writes those four positions,
//   which is why in place is free.  One table at a time: only (lo', hi' - lo') of a table stays in registers.  The pair (q, q + Q)
//   of the folded table of length len / 2 is exactly the pair vec_mle_round would read, so the gate is evaluated on it at
//   `points` <= 4 points (the loop over t unrolled to 4 and predicated on the wave-uniform `points`, t advancing by ONE addition
//   per table), one accumulator per point.
//   Montgomery factors: each raw product leaves a factor 1 / R.  PRODUCT carries R^-(K-1) on every term, as the round does.
//   R1CS: d's pair (value and difference) is scaled by 1 / R ONCE per quad (two products by the integer 1), so b c / R - d / R
//   is one subtraction and a times it carries R^-2 on every term - the stray power of a K = 3 product.  Either way the power
//   comes off once, where the final word is made (mle_round_close), and k_mle_round_fin is reused unchanged.
//   Products per quad: 2 K for the fold, plus points x (K - 1) for PRODUCT, 2 + 2 points for R1CS -
//     PRODUCT K = 1: 2;  K = 2, 3 points: 4 + 3 = 7;  K = 3, 4 points: 6 + 8 = 14;  R1CS, 4 points: 8 + 2 + 8 = 18
//   against 20 for the six ops the R1CS step replaces (8 in the four folds, 8 in round(eq, Az, Bz; 4), 4 in round(eq, Cz; 4)).
//   Registers: four accumulators, the tables' (value, difference) pairs and r are 8 (2 K + 5) VGPRs live across the gate - 104
//   at R1CS before a product's own temporaries.  The compiler reports 192 - 201 VGPRs for the R1CS bind and 167 - 170 at K = 3
//   (two waves per SIMD), no scratch; asked for three waves (168) it spills 44 and 12 bytes per lane, so it is not asked.
//
// ROUND ONLY  (no r: a sumcheck's first round) PRODUCT is vec_mle_round and goes to its launcher.  k_sc_round_r1cs<Fr> is
//   k_mle_round_part's loop over the pairs (p, p + len / 2) with the R1CS gate: 8 loads through vec_canon, 2 + 2 points products
//   per pair; tables may be periodic; nothing is written to a table.
//
// BIND ONLY  (points == 0: a sumcheck's last variable) K launches of k_mle_fold, in place, in the one enqueue.
//
// REDUCTION  one fold_block_tree per point.  A call whose quads (pairs) fit one block - len <= 1024 with r, len <= 512 without -
//   closes the sums there and writes d_out itself: no workspace.  Any other writes one partial per block and point, word
//   t x blocks + block of the handle's scratch, and k_mle_round_fin, one block, folds and closes them.
//   Workspace: blocks x points words with blocks = min(len / 1024, 2048) (len / 512 without r): at most 4 len / 512 < len <= n.
#pragma once
#include "ntt_mle.hip.hpp"

namespace blz {

enum { SC_GATE_PRODUCT = 0, SC_GATE_R1CS = 1 };   // BLZ_GATE_PRODUCT, BLZ_GATE_R1CS
constexpr int SC_MAX_TABLES = 4;
struct ScTables { uint32_t* p[SC_MAX_TABLES]; };   // the tables a bind writes: at least len words each

// the stray power of 1 / R on a gate's terms, as a number of operands of a product
template <int GATE, int K>
constexpr int sc_close_k() { return GATE == SC_GATE_R1CS ? 3 : K; }

// One quad of one table, folded in place: lo = the new word q, diff = the new word q + Q minus it
template <class Fr>
BLZ_DEV void sc_fold_quad(Fp<Fr>& lo, Fp<Fr>& diff, uint32_t* t, uint64_t q, uint64_t quarter, const Fp<Fr>& rm) {
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

// acc[t] += G at t = 0 .. points - 1; v: the tables' values at t = 0, d: their differences (R1CS: d's pair scaled by 1 / R)
template <class Fr, int GATE, int K>
BLZ_DEV void sc_gate_points(Fp<Fr> (&acc)[MLE_MAX_POINTS], Fp<Fr> (&v)[K], const Fp<Fr> (&d)[K], uint32_t points) {
    using E = Fp<Fr>;
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

// The block's accumulators: direct != 0 (one block): out = d_out, `points` canonical words; else out = the workspace, word
// t * gridDim.x + block = the block's partial of point t, with the stray power of 1 / R
template <class Fr>
BLZ_DEV void sc_block_sums(uint32_t* x, uint32_t* out, const Fp<Fr> (&acc)[MLE_MAX_POINTS], uint32_t points, uint32_t direct, int close_k) {
    using E = Fp<Fr>;
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) {
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

template <class Fr, int GATE, int K>
__global__ __launch_bounds__(VEC_THREADS) void k_sc_bind(uint32_t* out, ScTables tb, const uint32_t* r, uint64_t quarter, int log_stride,
                                                          uint32_t points, uint32_t direct) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint64_t stride = 1ull << log_stride;   // gridDim.x * VEC_THREADS, a power of two
    E rm;
    fp_load(rm, r);
    fp_to_mont(rm, rm);
    E acc[MLE_MAX_POINTS];
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) fp_zero(acc[t]);
#pragma unroll 1
    for (uint64_t q = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; q < quarter; q += stride) {
        E v[K], d[K];
#pragma unroll
        for (int j = 0; j < K; ++j) sc_fold_quad<Fr>(v[j], d[j], tb.p[j], q, quarter, rm);
        if constexpr (GATE == SC_GATE_R1CS) {
            vec_strip_mont(v[3]);
            vec_strip_mont(d[3]);
        }
        sc_gate_points<Fr, GATE, K>(acc, v, d, points);
    }
    sc_block_sums<Fr>(x, out, acc, points, direct, sc_close_k<GATE, K>());
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_sc_round_r1cs(uint32_t* out, NttVecArg a, NttVecArg b, NttVecArg c, NttVecArg dd, uint64_t half,
                                                                int log_stride, uint32_t points, uint32_t direct) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint64_t stride = 1ull << log_stride;
    E acc[MLE_MAX_POINTS];
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) fp_zero(acc[t]);
#pragma unroll 1
    for (uint64_t p = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; p < half; p += stride) {
        E v[4], d[4];
        mle_pair<Fr, false>(v[0], d[0], a, p, half);
        mle_pair<Fr, false>(v[1], d[1], b, p, half);
        mle_pair<Fr, false>(v[2], d[2], c, p, half);
        mle_pair<Fr, false>(v[3], d[3], dd, p, half);
        vec_strip_mont(v[3]);
        vec_strip_mont(d[3]);
        sc_gate_points<Fr, SC_GATE_R1CS, 4>(acc, v, d, points);
    }
    sc_block_sums<Fr>(x, out, acc, points, direct, sc_close_k<SC_GATE_R1CS, 4>());
}

template <class Fr, int GATE, int K>
void sc_bind_launch(hipStream_t st, dim3 grid, uint32_t* out, const NttVecArg* t, const uint32_t* r, uint64_t quarter, int ls, uint32_t points,
                    uint32_t direct) {
    ScTables tb{};
    for (int j = 0; j < K; ++j) tb.p[j] = const_cast<uint32_t*>(t[j].p);
    hipLaunchKernelGGL((k_sc_bind<Fr, GATE, K>), grid, dim3(VEC_THREADS), 0, st, out, tb, r, quarter, ls, points, direct);
}

// t: the gate's k tables (PRODUCT 1 .. 3, R1CS 4).  r != nullptr: every table holds at least len words, no two overlap, and
// their first len / 2 words are written; points == 0: bind only (len >= 2), else len >= 4.  r == nullptr: round only, tables
// may be periodic, 1 <= points.  out: `points` words; ws: the handle's scratch
template <class Fr>
int ntt_sumcheck_step_t(hipStream_t st, uint32_t gate, int k, const NttVecArg* t, const uint32_t* r, uint32_t points, uint64_t len, uint32_t* out,
                        uint32_t* ws) {
    if (r && points == 0) {
        for (int j = 0; j < k; ++j) BLZ_TRY(ntt_vec_mle_fold_t<Fr>(st, 0, const_cast<uint32_t*>(t[j].p), t[j], r, len));
        return BLZ_OK;
    }
    if (!r && gate == SC_GATE_PRODUCT) return ntt_vec_mle_round_t<Fr>(st, 0, out, k, t[0], t[k > 1 ? 1 : 0], t[k > 2 ? 2 : 0], points, len, ws);
    const uint64_t work = r ? len >> 2 : len >> 1;   // quads, or pairs
    uint64_t blocks = (work + VEC_THREADS - 1) / VEC_THREADS;   // a power of two: work is
    if (blocks > VEC_MAX_BLOCKS) blocks = VEC_MAX_BLOCKS;
    const int ls = fold_log2(blocks) + FOLD_LOG_THREADS;
    const uint32_t direct = blocks == 1 ? 1u : 0u;
    uint32_t* const part = direct ? out : ws;
    const dim3 grid((unsigned)blocks);
    int close_k = 3;
    if (!r) {
        hipLaunchKernelGGL(k_sc_round_r1cs<Fr>, grid, dim3(VEC_THREADS), 0, st, part, t[0], t[1], t[2], t[3], work, ls, points, direct);
    } else if (gate == SC_GATE_R1CS) {
        sc_bind_launch<Fr, SC_GATE_R1CS, 4>(st, grid, part, t, r, work, ls, points, direct);
    } else {
        close_k = k;
        switch (k) {
            case 1: sc_bind_launch<Fr, SC_GATE_PRODUCT, 1>(st, grid, part, t, r, work, ls, points, direct); break;
            case 2: sc_bind_launch<Fr, SC_GATE_PRODUCT, 2>(st, grid, part, t, r, work, ls, points, direct); break;
            case 3: sc_bind_launch<Fr, SC_GATE_PRODUCT, 3>(st, grid, part, t, r, work, ls, points, direct); break;
            default: return fail(BLZ_ERR_INVALID_PARAM, "a product gate takes 1 to %d tables", MLE_MAX_OPERANDS);
        }
    }
    if (!direct) hipLaunchKernelGGL(k_mle_round_fin<Fr>, dim3(1), dim3(VEC_THREADS), 0, st, out, (const uint32_t*)ws, (uint32_t)blocks, points, close_k);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
