// A sumcheck step for a caller-defined gate (blz_ntt_sumcheck_gate): the round polynomial of
//   G = T[common] x sum_m (+/-) prod_{j < nfactors_m} T[factor_mj]          (common < 0: no common factor)
// over up to 12 tables, with or without the in-place bind of ntt_sumcheck.hip.hpp.  The gate is DATA: NttGate travels by value in
// the kernel arguments, so ONE kernel, k_gate_round, over the two pair sources (ScPairs<false>, ScQuads) serves every gate - six
// instantiations for the three scalar fields where a gate compiled into k_sc_round costs eleven per field.  House rules as
// there: 256 lanes, the arithmetic of field.hip.hpp through vec_canon, no atomics, no flags, no allocation, no scratch memory,
// every dependency between blocks is a launch.  Every index read from the description is wave-uniform: the loops over tables,
// terms and factors are scalar control flow and a table's (pointer, mask) comes from the kernel arguments by a scalar load.
//
// A register array of Fp cannot be indexed by a table number known only at run time (it would live in scratch), so a lane keeps
// NO table in registers across the gate.  Lane g of S = blocks x 256 owns the items g, g + S, ... as in k_sc_round, and per item:
//   PHASE 1 (ScQuads only, the bind)  for each of the ntables tables, rolled: the lane's quad is folded in place as ScQuads::pair
//     folds it - 2 products - and the two canonical words q and q + Q are stored.  Every table is folded, named by a term or
//     not.  The loop is pipelined by one table (gate_fold_quads): table j + 1's four words are in flight while table j is folded.
//   PHASE 2 (the gate)  for each term, for each factor: load the lane's own (lo, hi) of that table - on the quad source the two
//     words this lane has just stored: same thread, same addresses, so program order holds and they come from L1 / L2 - and
//     multiply the running prod[t] by lo + t (hi - lo), t < points, one addition per point.  After the last factor prod[t] is
//     added to or subtracted from sum[t]; after the last term acc[t] += common_t x sum[t] (or sum[t] alone).
//   A table named f times is loaded f times; that buys the rolled loops - 6 inlined products for a factor, 6 for the common
//   factor, 2 for a deficit, 2 for the fold - and 3 x 6 + 2 elements of registers whatever the gate.
//
// MONTGOMERY POWERS  The words are plain, so a raw product of f of them carries R^-(f-1).  Every term is brought to the power of
//   the gate's longest, F = max nfactors: the first factor's (lo, diff) of a term of f factors is multiplied by the integer 1
//   F - f times (vec_strip_mont, twice per missing power, ONCE per item - the points are lo + t diff of the stripped pair).  The
//   common factor adds one power.  The sums are closed once, where the final word is made (mle_round_close / k_mle_round_fin),
//   with close_k = F + (common >= 0): close_k - 1 products by R^2.  The host computes F and the deficits (ntt.hip).
//
// PRODUCTS per item: 2 ntables (quads) + sum_m (points (f_m - 1) + 2 (F - f_m)) + points (common >= 0).
//   R1CS as eq (+ Az Bz, - Cz) at 4 points: 8 + (4 + 2) + 4 = 18, the count of BLZ_GATE_R1CS.  The vanilla PLONK gate
//   eq (qL a + qR b + qM a b - qO c + qC), 9 tables, F = 3, at 5 points: 18 + (5+2) + (5+2) + 10 + (5+2) + 4 + 5 = 58 per quad.
//
// REDUCTION, launch geometry and workspace: ntt_sumcheck.hip.hpp's (sc_plan, sc_finish), with points <= 6.
#pragma once
#include "ntt_sumcheck.hip.hpp"

namespace blz {

static_assert(NTT_GATE_MAX_TABLES <= 16 && NTT_GATE_MAX_FACTORS == 4, "a term word holds four table indices of four bits");

// The lane's pair of one table for the gate: on the quad source the two words phase 1 stored, canonical already
template <class Fr, class Source>
BLZ_DEV void gate_pair(Fp<Fr>& lo, Fp<Fr>& diff, NttVecArg a, uint64_t i, uint64_t work) {
    if constexpr (Source::BINDS) {
        Fp<Fr> hi;
        fp_load(lo, a.p + i * 8);
        fp_load(hi, a.p + (i + work) * 8);
        fp_sub(diff, hi, lo);
    } else {
        mle_pair<Fr, false>(lo, diff, a, i, work);
    }
}

// Phase 1: the lane's quad of every table folded in place, as ScQuads::pair folds one - but the four words of table j + 1 are
// loaded BEFORE table j is folded and stored (no two tables overlap and no other lane touches this lane's positions, which the
// compiler cannot know), so a table's load latency hides behind the fold in front of it; prod and sum are dead here, the eight
// words in flight cost no register at the kernel's peak
template <class Fr>
BLZ_DEV void gate_fold_quads(const NttGate& g, uint64_t q, uint64_t quarter, const Fp<Fr>& rm) {
    using E = Fp<Fr>;
    E w[4], nx[4];
    {
        const uint32_t* const t = g.t[0].p;
#pragma unroll
        for (int k = 0; k < 4; ++k) fp_load(w[k], t + (q + k * quarter) * 8);
    }
#pragma unroll 1
    for (uint32_t j = 0; j < g.ntables; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) fp_zero(nx[k]);
        if (j + 1 < g.ntables) {
            const uint32_t* const t = g.t[j + 1].p;
#pragma unroll
            for (int k = 0; k < 4; ++k) fp_load(nx[k], t + (q + k * quarter) * 8);
        }
        uint32_t* const t = const_cast<uint32_t*>(g.t[j].p);
#pragma unroll
        for (int k = 0; k < 2; ++k) {   // word q + k Q = w[k] + r (w[k + 2] - w[k])
            vec_canon(w[k]);
            vec_canon(w[k + 2]);
            fp_sub(w[k + 2], w[k + 2], w[k]);
            fp_mul(w[k + 2], w[k + 2], rm);
            fp_add(w[k], w[k], w[k + 2]);
            fp_reduce(w[k]);
            fp_store(t + (q + k * quarter) * 8, w[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = nx[k];
    }
}

// r: one device word, read only where the source binds; work: the pairs (quads) of the call
template <class Fr, class Source>
__global__ __launch_bounds__(VEC_THREADS) void k_gate_round(uint32_t* out, NttGate g, const uint32_t* r, uint64_t work, int log_stride,
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
        if constexpr (Source::BINDS) gate_fold_quads<Fr>(g, i, work, rm);
        E sum[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) fp_zero(sum[t]);
#pragma unroll 1
        for (uint32_t m = 0; m < g.nterms; ++m) {
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
                    fp_add(acc[t], acc[t], pr);
                    if (t + 1 < NP) fp_add(v, v, d);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NP; ++t)
                if (t < (int)points) fp_add(acc[t], acc[t], sum[t]);
        }
    }
    sc_block_sums<Fr>(x, out, acc, points, direct, (int)g.close_k);
}

// g: the description as ntt.hip packs it; the rest as ntt_sumcheck_step_t.  r != nullptr: every table of g holds at least len
// words, no two overlap, and their first len / 2 words are written; points == 0: bind only.  r == nullptr: round only, tables
// may be periodic.  out: `points` <= 6 words; ws: the handle's scratch
template <class Fr>
int ntt_sumcheck_gate_t(hipStream_t st, const NttGate& g, const uint32_t* r, uint32_t points, uint64_t len, uint32_t* out, uint32_t* ws) {
    if (r && points == 0) return sc_bind_only<Fr>(st, (int)g.ntables, g.t, r, len);
    const ScPlan p = sc_plan(r != nullptr, len);
    const auto kernel = r ? &k_gate_round<Fr, ScQuads> : &k_gate_round<Fr, ScPairs<false>>;
    hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(VEC_THREADS), 0, st, p.sums(out, ws), g, r, p.work, p.log_stride, points, p.direct);
    return sc_finish<Fr>(st, p, out, ws, points, (int)g.close_k);
}

}  // namespace blz
