// A caller-defined gate evaluated position by position (blz_ntt_gate_eval): for p < len
//   dst[p] = T[common][p_c] x sum_m (+/-) prod_{j < nfactors_m} T[factor_mj][p_mj]      (common < 0: the sum alone)
// where table i is read at p_i = (p + rot[i]) & mask_i - the element-wise counterpart of ntt_gate.hip.hpp, over the same
// description.  The gate is DATA: NttGate travels by value in the kernel arguments with the rotations and the field's powers of R
// beside it (GevalArgs), so ONE kernel, k_geval, serves every gate, rotated or not.  House rules as in ntt_gate.hip.hpp: 256
// lanes, one position per lane per step, the grid-stride loop of k_vec_ew, the arithmetic of field.hip.hpp through vec_canon, no
// atomics, no LDS, no allocation, no scratch memory.  Every index read from the description is wave-uniform: the loops over terms
// and factors are scalar control flow, and a table's (pointer, mask, rotation) and a term's power of R come from the kernel
// arguments by scalar loads.
//
// A register array of Fp cannot be indexed by a table number known only at run time (it would live in scratch), so a lane keeps
// NO table in registers across the gate: a table named f times is loaded f times, from cache after the first.  The factors of
// the whole gate - term after term, the common factor last - form one sequence, and the NEXT factor's two 16-byte loads are
// issued before the product of the current one (as gate_fold_quads does for its tables): 4 elements of registers whatever the
// gate (the factor in hand, the one in flight, the term's product, the sum).
//
// MONTGOMERY POWERS  The words are plain, so a raw product of f of them carries R^-(f-1).  The power is folded into a constant per
//   term: the FIRST factor of a term of f >= 2 factors is multiplied by R^f mod m (one product, mont(x, R^f) = x R^(f-1)), after
//   which the f - 1 products of the chain leave the plain product; a term of one factor is its word, reduced.  The common factor
//   is brought to Montgomery form (one product) and multiplies the plain sum (one more): plain again.  Nothing is closed at the
//   end.  The constants R^2, R^3, R^4 are computed at compile time (GevalPow) and handed over in the kernel arguments.
//
// PRODUCTS per position: sum over the terms with f_m >= 2 of f_m, + 2 (common >= 0).  Reusing NttGate's deficits and close_k
//   instead would cost (nterms + 1) (F - 1) (+ 1 + 1 with a common factor), never less.  The vanilla PLONK gate
//   qL a + qR b + qM a b - qO c + qC (terms of 2, 2, 3, 2, 1 factors, no common factor): 2 + 2 + 3 + 2 = 9 (12 the other way);
//   under a common factor eq: 11.  A linear combination sum_{j < 6} c_j f_j: 12.
//
// WHY EVERY INTERMEDIATE FITS  mont(a, b) = (a b + q m) / R < a b / R + m, and a raw word is below R = 2^256.
//   first factor   x raw, the constant c < m:  below m x / R + m < 2m.
//   chain          prod < 2m (below m in the strict field), v raw:  below prod v / R + m < prod + m.
//   strict field (BLS12-381, 4m > R): fp_mul subtracts m once where the value (the word above the eight counted in) is not
//     below m, so a product with one operand below m is below m - canonical - whatever 256-bit word the other is: the first
//     factor's, and by induction every product of the chain.  2^256 - 1 in every position of a four-factor term is no exception.
//   lazy fields (BLS12-377, BN254: 4m < R): the product does not subtract, so geval_mul takes m off once: prod + m < 3m -> below
//     2m again, inside the representation fp_add / fp_sub / fp_mul expect ([0, 2m]); 3m < R: no ninth word.
//   sums           fp_add / fp_sub keep [0, 2m] (strict: [0, m)); a one-factor term enters through vec_canon: below m.
//   common factor  mont(c raw, R^2) below 2m (strict: below m), times the sum: below 4 m^2 / R + m < 2m (strict: below m).
//   The word stored goes through fp_reduce: canonical.
//
// IN PLACE  dst may be a table that starts where dst starts, with rotation 0 and at least len words (ntt.hip refuses every other
//   meeting): a lane has loaded every factor of its position before it stores, and no other lane touches that position.
#pragma once
#include "ntt_vec.hip.hpp"

namespace blz {

// R^2, R^3, R^4 mod m as plain limbs: w[f - 2] closes a term of f factors.  Montgomery's product (CIOS) at compile time
template <class P>
struct GevalPow {
    uint32_t w[NTT_GATE_MAX_FACTORS - 1][P::N];
    static constexpr void mont(uint32_t (&r)[P::N], const uint32_t (&a)[P::N], const uint32_t (&b)[P::N]) {
        constexpr int N = P::N;
        uint32_t t[N + 2] = {};
        for (int i = 0; i < N; ++i) {
            uint64_t c = 0;
            for (int j = 0; j < N; ++j) {
                c += (uint64_t)t[j] + (uint64_t)a[j] * b[i];
                t[j] = (uint32_t)c;
                c >>= 32;
            }
            c += t[N];
            t[N] = (uint32_t)c;
            t[N + 1] = (uint32_t)(c >> 32);
            const uint32_t q = t[0] * P::N0;
            c = ((uint64_t)t[0] + (uint64_t)q * P::MOD[0]) >> 32;
            for (int j = 1; j < N; ++j) {
                c += (uint64_t)t[j] + (uint64_t)q * P::MOD[j];
                t[j - 1] = (uint32_t)c;
                c >>= 32;
            }
            c += t[N];
            t[N - 1] = (uint32_t)c;
            t[N] = t[N + 1] + (uint32_t)(c >> 32);
        }
        uint32_t u[N] = {};
        uint64_t br = 0;
        for (int j = 0; j < N; ++j) {   // canonical operands: t < 2m
            const uint64_t d = (uint64_t)t[j] - P::MOD[j] - br;
            u[j] = (uint32_t)d;
            br = (d >> 32) & 1u;
        }
        const bool keep = t[N] == 0 && br != 0;
        for (int j = 0; j < N; ++j) r[j] = keep ? t[j] : u[j];
    }
    constexpr GevalPow() : w{} {
        for (int i = 0; i < P::N; ++i) w[0][i] = P::R2[i];
        for (int k = 1; k < NTT_GATE_MAX_FACTORS - 1; ++k) mont(w[k], w[k - 1], P::R2);
    }
};

// The kernel's description of the call, by value: the gate as ntt.hip packs it (deficits and close_k are not looked at), the
// rotations beside it, and the field's closing constants
struct GevalArgs {
    NttGate g;
    uint64_t rot[NTT_GATE_MAX_TABLES];
    uint32_t pw[NTT_GATE_MAX_FACTORS - 1][8];
};
static_assert(sizeof(GevalArgs) <= 1024, "the description travels in the kernel arguments");

// table i's word for position p
template <class Fr>
BLZ_DEV void geval_load(Fp<Fr>& x, const GevalArgs& a, uint32_t i, uint64_t p) {
    fp_load(x, a.g.t[i].p + ((p + a.rot[i]) & a.g.t[i].mask) * 8);
}

// prod = prod v for a raw word v; prod stays below 2m (strict field: below m) - the head comment's chain
template <class Fr>
BLZ_DEV void geval_mul(Fp<Fr>& prod, const Fp<Fr>& v) {
    fp_mul(prod, prod, v);
    if constexpr (Fr::LAZY) fp_csub_const<Fr, Fr::MOD>(prod);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_geval(uint32_t* dst, GevalArgs a, uint64_t len) {
    using E = Fp<Fr>;
    static_assert(Fr::N == 8, "GevalArgs::pw holds eight limbs");
    const NttGate& g = a.g;
    const uint64_t stride = (uint64_t)gridDim.x * VEC_THREADS;
#pragma unroll 1
    for (uint64_t p = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; p < len; p += stride) {
        E sum, cur;
        fp_zero(sum);
        geval_load<Fr>(cur, a, (g.term[0] >> 8) & 15u, p);
#pragma unroll 1
        for (uint32_t m = 0; m < g.nterms; ++m) {
            const uint32_t tw = g.term[m], f = tw & 7u;
            // what follows this term's last factor: the next term's first, the common factor, or nothing (-1)
            const int32_t after = m + 1 < g.nterms ? (int32_t)((g.term[m + 1] >> 8) & 15u) : g.common;
            E prod;
#pragma unroll 1
            for (uint32_t j = 0; j < f; ++j) {
                const int32_t next = j + 1 < f ? (int32_t)((tw >> (12 + 4 * j)) & 15u) : after;
                E nx;
                fp_zero(nx);
                if (next >= 0) geval_load<Fr>(nx, a, (uint32_t)next, p);
                if (j > 0) {
                    geval_mul<Fr>(prod, cur);
                } else if (f > 1) {
                    E c;
#pragma unroll
                    for (int i = 0; i < Fr::N; ++i) c.v[i] = a.pw[f - 2][i];
                    fp_mul(prod, cur, c);
                } else {
                    prod = cur;
                    vec_canon(prod);
                }
                cur = nx;
            }
            if (tw & 8u) fp_sub(sum, sum, prod); else fp_add(sum, sum, prod);
        }
        if (g.common >= 0) {   // cur holds the common factor's word
            fp_to_mont(cur, cur);
            fp_mul(sum, sum, cur);
        }
        fp_reduce(sum);
        fp_store(dst + p * 8, sum);
    }
}

// g: the description as ntt.hip packs it, its tables resolved; rot: one rotation per table; dst: len words, 1 <= len.  A table
// may be dst itself under the rule of the head comment
template <class Fr>
int ntt_gate_eval_t(hipStream_t st, uint32_t* dst, const NttGate& g, const uint64_t* rot, uint64_t len) {
    static constexpr GevalPow<Fr> POW{};
    GevalArgs a{};
    a.g = g;
    for (uint32_t i = 0; i < g.ntables; ++i) a.rot[i] = rot[i];
    for (int k = 0; k < NTT_GATE_MAX_FACTORS - 1; ++k)
        for (int i = 0; i < Fr::N; ++i) a.pw[k][i] = POW.w[k][i];
    const uint64_t blocks = (len + VEC_THREADS - 1) / VEC_THREADS;
    hipLaunchKernelGGL(k_geval<Fr>, dim3((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), dim3(VEC_THREADS), 0, st, dst, a, len);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
