// A gate whose factors may be LINEAR FORMS over the tables, evaluated position by position (blz_ntt_gate_eval_lin): for p < len
//   dst[p] = C(p) x sum_m (+/-) prod_{j < nfactors_m} F_mj(p)                                     (common < 0: the sum alone)
//   F, C   = a table word T[i][p_i], p_i = (p + rot[i]) & mask_i, or the value of a form
//   L_k(p) = sum_{s < nsummands_k} (+/-) [ T[coef_s][p_coef] x ] T[table_s][p_table]
// - products of sums, where ntt_geval.hip.hpp has products of words: the permutation argument's quotient term, the numerator and
// denominator columns behind Z, the logUp denominator, (Z - 1) L_1.  The gate is DATA: NttLinGate travels by value in the kernel
// arguments with the rotations and the field's powers of R beside it (LinevalArgs), so ONE kernel, k_lineval, serves every
// gate.  House rules as in ntt_geval.hip.hpp: 256 lanes, one position per lane per step, the grid-stride loop of k_vec_ew, the
// arithmetic of field.hip.hpp through vec_canon, nothing but loads, products and one store per position, no scratch memory.
// Every index read from the description is wave-uniform: the walk over terms, factors and summands (LinCursor) is scalar
// control flow, and a table's (pointer, mask, rotation) and a term's power of R come from the kernel arguments by scalar loads.
//
// WORDS IN SEQUENCE  A lane keeps NO table in registers across the gate (a register array cannot be indexed by a number known
//   only at run time): a table named f times is loaded f times, from cache after the first.  The words of the whole gate - term
//   after term, factor after factor, within a form summand after summand (a coefficient longer than one word ahead of its
//   table's word), the common factor last - form ONE sequence of slots, and the NEXT slot's two 16-byte loads are issued before
//   the current slot is worked on.  Seven elements of registers whatever the gate: the word in hand, the one in flight, a
//   coefficient, the form, the term's product, the sum (and the product's own columns).
//
// ONE-WORD COEFFICIENTS  The one departure from ntt_geval.hip.hpp.  A coefficient is usually a scalar - beta, gamma^j, alpha, a
//   one-word table - and its Montgomery form c R does not depend on the position.  Ahead of the loop lane i of every block
//   brings table i to Montgomery form if it is one word long and a form that is evaluated names it as a coefficient
//   (NttLinGate::coef_tables), and leaves it in LDS: 16 x 32 bytes.  EVERY lane reaches the barrier behind that, the lanes of a
//   block whose positions all lie at or above len included: nothing returns early.  In the loop the coefficient is read back by a
//   broadcast read (one address for the wave) and c x is ONE product that lands plain.  A longer coefficient is a slot of its
//   own: its word is brought to Montgomery form per position, two products.
//
// MONTGOMERY POWERS  The words are plain.  A summand c x is mont(c R, x) = c x: plain, so a form's value is plain and enters a
//   term as a word does.  A raw product of f values carries R^-(f-1); as in k_geval the FIRST factor of a term of f >= 2 factors is
//   multiplied by R^f mod m (one product), after which the f - 1 products of the chain leave the plain product; a term of one
//   factor is its value, reduced.  The common factor - a word or a form's value - is brought to Montgomery form (one product)
//   and multiplies the plain sum (one more).  R^2 .. R^4 are GevalPow's, handed over in the kernel arguments.
//
// PRODUCTS per position: per summand with a coefficient 1 (a one-word table) or 2 (a longer one), none without; f per term of
//   f >= 2 factors; 2 for a common factor.  A form named twice is evaluated twice.  The three-wire permutation term
//   Z(wX) prod_j (w_j + beta sigma_j + gamma) - Z prod_j (w_j + (beta k_j) X + gamma): six forms with one scalar coefficient
//   each, two terms of four factors: 6 + 8 = 14.  The same through k_geval - six calls a + beta sigma + gamma (2 each), a
//   seventh of two four-factor terms (8): 20, and six temporaries.  beta + gamma f1 + gamma^2 f2 + gamma^3 f3: 3.
//
// WHY EVERY INTERMEDIATE FITS  mont(a, b) = (a b + q m) / R < a b / R + m, and a raw word is below R = 2^256.  "Strict" is
//   BLS12-381 (4m > R: values canonical, fp_mul subtracts m once where the value, the word above the eight counted in, is not
//   below m); "lazy" is BLS12-377 and BN254 (4m < R: values in [0, 2m], fp_mul does not subtract, lin_mul takes m off once).
//   coefficient    c raw: mont(c, R^2 mod m) < m c / R + m < 2m; strict: one operand below m, so below m.  LDS holds that.
//   summand c x    c R below 2m, x raw: below 2m x / R + m < 3m < R, less m: below 2m.  Strict: c R < m, so below 2m before and
//                  below m after the product's own subtraction, whatever 256-bit word x is.
//   summand x      through vec_canon: below m.
//   form           fp_add / fp_sub reduce at EVERY step: two values of [0, 2m] add to at most 4m < R and come back to [0, 2m]
//                  (strict: below m, sum below 2m < R, back below m).  Nothing is left to pile up: four summands unreduced would
//                  reach 8m, which is above R for BN254 (m about 0.19 R) and for BLS12-381.  The first summand is added to or
//                  taken from 0.  The value, below 2m (strict: below m), enters a chain as a raw word does - every bound
//                  below holds for any word below R.
//   first factor   v below R, the constant R^f mod m below m: below m v / R + m < 2m (strict: below m).
//   chain          prod below 2m, v below R: below prod v / R + m < 3m, less m: below 2m.  Strict: prod < m, so below m.
//   one factor     through vec_canon, a form's value too: below m.
//   sums           fp_add / fp_sub keep [0, 2m] (strict: [0, m)).
//   common factor  mont(v, R^2) below 2m for v below R (strict: below m), times the sum: below 4 m^2 / R + m < 2m (strict:
//                  below m).  The word stored goes through fp_reduce: canonical.
//
// IN PLACE  dst may be a table that starts where dst starts, with rotation 0 and at least len words (ntt.hip refuses every other
//   meeting), whatever names the table - a factor, a summand, a coefficient: a lane has loaded every word of its position
//   before it stores, and no other lane touches that position.  A one-word table can be dst only at len 1: one block, whose
//   lanes read the word ahead of the barrier and whose lane 0 stores behind it.
#pragma once
#include "ntt_geval.hip.hpp"

namespace blz {

// The kernel's description of the call, by value: the gate as ntt.hip packs it, its tables resolved, the rotations beside it,
// and the field's closing constants
struct LinevalArgs {
    NttLinGate g;
    uint64_t rot[NTT_LIN_MAX_TABLES];
    uint32_t pw[NTT_GATE_MAX_FACTORS - 1][8];
};
static_assert(sizeof(LinevalArgs) <= 1024, "the description travels in the kernel arguments");

// One slot of the gate's sequence of words.  Every field is wave-uniform
struct LinCursor {
    uint32_t m, j;    // the term (g.nterms: the common factor) and the factor in it
    uint32_t fac;     // that factor's byte: a table index, or NTT_LIN_FORM | k
    uint32_t s, sw;   // in a form: the summand and its word of NttLinGate::form
    uint32_t coef;    // in a form: 1 the slot is the summand's coefficient, a table of more than one word; 0 its table
};

// the summand's coefficient is a table of more than one word: a slot of its own
BLZ_DEV uint32_t lin_coef_slot(const LinevalArgs& a, uint32_t sw) {
    const uint32_t c = (sw >> 8) & 0xFFu;
    return c != NTT_LIN_NO_COEF && a.g.t[c & 15u].mask != 0 ? 1u : 0u;
}
// c.m, c.j name a factor: its first slot
BLZ_DEV void lin_enter(const LinevalArgs& a, LinCursor& c) {
    c.fac = c.m < a.g.nterms ? (a.g.term_fac[c.m & 7u] >> (8 * c.j)) & 0xFFu : (uint32_t)a.g.common & 0xFFu;
    c.s = 0;
    c.sw = 0;
    c.coef = 0;
    if (c.fac & NTT_LIN_FORM) {
        c.sw = a.g.form[c.fac & 7u][0];
        c.coef = lin_coef_slot(a, c.sw);
    }
}
// the slot after c; false: c was the last
BLZ_DEV bool lin_next(const LinevalArgs& a, LinCursor& c) {
    if (c.fac & NTT_LIN_FORM) {
        if (c.coef) {
            c.coef = 0;
            return true;
        }
        if (++c.s < a.g.form_n[c.fac & 7u]) {
            c.sw = a.g.form[c.fac & 7u][c.s & 3u];
            c.coef = lin_coef_slot(a, c.sw);
            return true;
        }
    }
    if (c.m >= a.g.nterms) return false;   // the common factor is the last
    if (++c.j == (a.g.term_hdr[c.m & 7u] & 7u)) {
        c.j = 0;
        if (++c.m == a.g.nterms && a.g.common < 0) return false;
    }
    lin_enter(a, c);
    return true;
}
// the table whose word the slot reads
BLZ_DEV uint32_t lin_table(const LinCursor& c) {
    return ((c.fac & NTT_LIN_FORM) ? (c.coef ? c.sw >> 8 : c.sw) : c.fac) & 15u;
}
template <class Fr>
BLZ_DEV void lin_load(Fp<Fr>& x, const LinevalArgs& a, uint32_t i, uint64_t p) {
    fp_load(x, a.g.t[i].p + ((p + a.rot[i]) & a.g.t[i].mask) * 8);
}
// r = x y R^-1 for x below 2m (strict field: below m) and any word y; r below 2m (below m) - the head comment's products
template <class Fr>
BLZ_DEV void lin_mul(Fp<Fr>& r, const Fp<Fr>& x, const Fp<Fr>& y) {
    fp_mul(r, x, y);
    if constexpr (Fr::LAZY) fp_csub_const<Fr, Fr::MOD>(r);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_lineval(uint32_t* dst, LinevalArgs a, uint64_t len) {
    using E = Fp<Fr>;
    static_assert(Fr::N == 8, "LinevalArgs::pw and the LDS rows hold eight limbs");
    __shared__ uint32_t coefm[NTT_LIN_MAX_TABLES][8];   // table i's one word in Montgomery form, where coef_tables names it
    const NttLinGate& g = a.g;
    {
        const uint32_t* src = nullptr;
#pragma unroll 1
        for (uint32_t i = 0; i < g.ntables; ++i)
            if (((g.coef_tables >> i) & 1u) && g.t[i].mask == 0 && threadIdx.x == i) src = g.t[i].p;
        if (src) {
            E c;
            fp_load(c, src);
            fp_to_mont(c, c);
#pragma unroll
            for (int i = 0; i < Fr::N; ++i) coefm[threadIdx.x & 15u][i] = c.v[i];
        }
    }
    __syncthreads();   // every lane of every block: nothing above returns
    const uint64_t stride = (uint64_t)gridDim.x * VEC_THREADS;
#pragma unroll 1
    for (uint64_t p = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; p < len; p += stride) {
        E sum, prod, form, coef, cur;
        fp_zero(sum);
        fp_zero(prod);
        fp_zero(form);
        fp_zero(coef);
        LinCursor c{};
        lin_enter(a, c);
        lin_load<Fr>(cur, a, lin_table(c), p);
        bool more = true;
#pragma unroll 1
        while (more) {
            LinCursor nc = c;
            more = lin_next(a, nc);
            E nx;
            fp_zero(nx);
            if (more) lin_load<Fr>(nx, a, lin_table(nc), p);
            bool value = true;   // cur is a factor's value: a table's word, or a form's after its last summand
            if (c.fac & NTT_LIN_FORM) {
                if (c.coef) {   // a long coefficient's word: kept in Montgomery form for the slot that follows
                    fp_to_mont(coef, cur);
                    value = false;
                } else {
                    const uint32_t ct = (c.sw >> 8) & 0xFFu;
                    if (ct == NTT_LIN_NO_COEF) {
                        vec_canon(cur);
                    } else {
                        if (g.t[ct & 15u].mask == 0) {
#pragma unroll
                            for (int i = 0; i < Fr::N; ++i) coef.v[i] = coefm[ct & 15u][i];
                        }
                        lin_mul<Fr>(cur, coef, cur);
                    }
                    if (c.s == 0) fp_zero(form);
                    if ((c.sw >> 16) & 1u) fp_sub(form, form, cur); else fp_add(form, form, cur);
                    if (c.s + 1 < g.form_n[c.fac & 7u]) value = false; else cur = form;
                }
            }
            if (value) {
                if (c.m == g.nterms) {   // the common factor
                    fp_to_mont(cur, cur);
                    fp_mul(sum, sum, cur);
                } else {
                    const uint32_t hdr = g.term_hdr[c.m & 7u], f = hdr & 7u;
                    if (c.j > 0) {
                        lin_mul<Fr>(prod, prod, cur);
                    } else if (f > 1) {
                        E k;
#pragma unroll
                        for (int i = 0; i < Fr::N; ++i) k.v[i] = a.pw[f - 2][i];
                        fp_mul(prod, cur, k);
                    } else {
                        prod = cur;
                        vec_canon(prod);
                    }
                    if (c.j + 1 == f) {
                        if (hdr & 8u) fp_sub(sum, sum, prod); else fp_add(sum, sum, prod);
                    }
                }
            }
            cur = nx;
            c = nc;
        }
        fp_reduce(sum);
        fp_store(dst + p * 8, sum);
    }
}

// g: the description as ntt.hip packs it, its tables resolved; rot: one rotation per table; dst: len words, 1 <= len.  A table
// may be dst itself under the rule of the head comment
template <class Fr>
int ntt_gate_eval_lin_t(hipStream_t st, uint32_t* dst, const NttLinGate& g, const uint64_t* rot, uint64_t len) {
    static constexpr GevalPow<Fr> POW{};
    LinevalArgs a{};
    a.g = g;
    for (uint32_t i = 0; i < g.ntables; ++i) a.rot[i] = rot[i];
    for (int k = 0; k < NTT_GATE_MAX_FACTORS - 1; ++k)
        for (int i = 0; i < Fr::N; ++i) a.pw[k][i] = POW.w[k][i];
    const uint64_t blocks = (len + VEC_THREADS - 1) / VEC_THREADS;
    hipLaunchKernelGGL(k_lineval<Fr>, dim3((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), dim3(VEC_THREADS), 0, st, dst, a, len);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
