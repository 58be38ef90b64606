// A zerocheck step (blz_ntt_zerocheck_gate): ntt_gate.hip.hpp's step for sum_p eq(tau, p) G(p) with the equality table taken out of
// the gate.  With top-variable pairing the round polynomial of round i factors,
//   s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X),   u_i(X) = sum_p W_i[p] G(X, p),   W_i = eq(tau_0 .. tau_{m-2-i}, .),
// and the weight W_i - half the live length, the same for every X - is all the device needs of eq:
//   * it multiplies the gate's sum ONCE per point, where a common eq table costs a product per point at one point more (s_i has
//     the degree of G plus one, u_i the degree of G; the caller multiplies the linear factor back in);
//   * it is not folded by r: eq(tau, 0) + eq(tau, 1) = 1, so W_{i+1}[q] = W_i[q] + W_i[q + Q] - no product - and both words
//     belong to the lane that owns quad q.
// One kernel, k_zc_round, over the two pair sources as k_gate_round is; the gate is the same DATA (NttGate by value) and the weight
// one more NttVecArg.  Phase 1 (gate_fold_quads), the pairs (gate_pair), the launch plan and the reduction (sc_plan, sc_block_sums,
// sc_finish) are ntt_gate.hip.hpp's and ntt_sumcheck.hip.hpp's, not copies; the term loop is k_gate_round's, written out here so
// that ntt_gate.hip.hpp and its six kernels' code stay as they are.  The house rules hold: 256 lanes, scalar control flow over the description, no atomics, no flags, no allocation, no scratch memory, every
// dependency between blocks is a launch.
//
// Per item i of `work`:
//   quads (with r)   the lane's two weight words, W[i] and W[i + work], are LOADED first and sit in flight under the table folds
//     of phase 1; then W[i] <- W[i] + W[i + work], canonical, is stored - exactly `work` = len / 4 words are written, no other
//     weight byte - and kept in registers for the item;
//   pairs (no r)     W[i & mask], canonical: the weight may be periodic, as the tables may;
//   then the terms, and acc[t] += W x (common_t x) sum[t].
// The weight is a plain word, so it adds one Montgomery power: the sums are closed with close_k + 1.
//
// PRODUCTS per item: ntt_gate.hip.hpp's count with `points` for the weight, at one point fewer than with common = eq.  R1CS
//   W (Az Bz - Cz) at 3 points: 6 + 3 + 2 + 3 = 14 (18 with eq at 4); the vanilla PLONK gate over its eight tables at 4 points:
//   16 + (4+2) + (4+2) + 8 + (4+2) + 4 + 4 = 50 (58 with eq at 5).  Traffic of the weight: len / 2 words read, len / 4 written.
#pragma once
#include "ntt_gate.hip.hpp"

namespace blz {

// wt: the weight; quads: at least 2 x work words, the first `work` are written; pairs: read at i & mask.  The rest as k_gate_round
template <class Fr, class Source>
__global__ __launch_bounds__(VEC_THREADS) void k_zc_round(uint32_t* out, NttGate g, NttVecArg wt, const uint32_t* r, uint64_t work, int log_stride,
                                                           uint32_t points, uint32_t direct) {
    using E = Fp<Fr>;
    constexpr int NP = NTT_GATE_MAX_POINTS;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint64_t stride = 1ull << log_stride;   // gridDim.x * VEC_THREADS, a power of two
    E rm;
    if constexpr (Source::BINDS) {
        fp_load(rm, r);
        fp_to_mont(rm, rm);
    }
    E acc[NP];
#pragma unroll
    for (int t = 0; t < NP; ++t) fp_zero(acc[t]);
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; i < work; i += stride) {
        E w;
        if constexpr (Source::BINDS) {
            uint32_t* const wp = const_cast<uint32_t*>(wt.p);
            E w2;
            fp_load(w, wp + i * 8);
            fp_load(w2, wp + (i + work) * 8);
            gate_fold_quads<Fr>(g, i, work, rm);
            vec_canon(w);
            vec_canon(w2);
            fp_add(w, w, w2);
            fp_reduce(w);
            fp_store(wp + i * 8, w);
        } else {
            fp_load(w, wt.p + (i & wt.mask) * 8);
            vec_canon(w);
        }
        E sum[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) fp_zero(sum[t]);
#pragma unroll 1
        for (uint32_t m = 0; m < g.nterms; ++m) {   // k_gate_round's terms, statement for statement
            const uint32_t tw = g.term[m];
            E prod[NP];
            {
                E d;
                gate_pair<Fr, Source>(prod[0], d, g.t[(tw >> 8) & 15u], i, work);
#pragma unroll 1
                for (uint32_t s = (tw >> 4) & 7u; s > 0; --s) {
                    vec_strip_mont(prod[0]);
                    vec_strip_mont(d);
                }
#pragma unroll
                for (int t = 1; t < NP; ++t)
                    if (t < (int)points) fp_add(prod[t], prod[t - 1], d);
            }
#pragma unroll 1
            for (uint32_t j = 1; j < (tw & 7u); ++j) {
                E v, d;
                gate_pair<Fr, Source>(v, d, g.t[(tw >> (8 + 4 * j)) & 15u], i, work);
#pragma unroll
                for (int t = 0; t < NP; ++t) {
                    if (t < (int)points) {
                        fp_mul(prod[t], prod[t], v);
                        if (t + 1 < NP) fp_add(v, v, d);
                    }
                }
            }
            if (tw & 8u) {
#pragma unroll
                for (int t = 0; t < NP; ++t)
                    if (t < (int)points) fp_sub(sum[t], sum[t], prod[t]);
            } else {
#pragma unroll
                for (int t = 0; t < NP; ++t)
                    if (t < (int)points) fp_add(sum[t], sum[t], prod[t]);
            }
        }
        if (g.common >= 0) {
            E v, d;
            gate_pair<Fr, Source>(v, d, g.t[g.common], i, work);
#pragma unroll
            for (int t = 0; t < NP; ++t) {
                if (t < (int)points) {
                    E pr;
                    fp_mul(pr, v, sum[t]);
                    fp_mul(pr, pr, w);
                    fp_add(acc[t], acc[t], pr);
                    if (t + 1 < NP) fp_add(v, v, d);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NP; ++t) {
                if (t < (int)points) {
                    E pr;
                    fp_mul(pr, sum[t], w);
                    fp_add(acc[t], acc[t], pr);
                }
            }
        }
    }
    sc_block_sums<Fr>(x, out, acc, points, direct, (int)g.close_k + 1);
}

// g, r, len, out, ws: as ntt_sumcheck_gate_t, with 1 <= points.  wt: the weight, device words.  r != nullptr: it holds at least
// len / 2 words, none of them in a table's first len words, and its first len / 4 are written; r == nullptr: it may be periodic
template <class Fr>
int ntt_zerocheck_gate_t(hipStream_t st, const NttGate& g, NttVecArg wt, const uint32_t* r, uint32_t points, uint64_t len, uint32_t* out, uint32_t* ws) {
    const ScPlan p = sc_plan(r != nullptr, len);
    const auto kernel = r ? &k_zc_round<Fr, ScQuads> : &k_zc_round<Fr, ScPairs<false>>;
    hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(VEC_THREADS), 0, st, p.sums(out, ws), g, wt, r, p.work, p.log_stride, points, p.direct);
    return sc_finish<Fr>(st, p, out, ws, points, (int)g.close_k + 1);
}

}  // namespace blz
