// The small rounds of a GKR argument over a FRACTION tree (blz_ntt_gkr_prove_frac, logUp-GKR) in ONE block: k_fgkr_tail is
// k_gkr_tail's two jobs (ntt_gkr.hip.hpp) over four tables.  A fraction tree over 2^m leaves (P, Q) is proven by m layers and
// m (m - 1) / 2 sumcheck rounds, as a product tree is, but a layer has four tables - the halves of the numerators and of the
// denominators - and a batching challenge lambda.  The transcript helpers and the Keccak lane layout are that header's.
//
// THE GATE WITHOUT THE SCALAR  Under lambda the layer identity is
//     P(tau) + lambda Q(tau) = sum_p eq(tau, p) [ P_lo Q_hi + P_hi Q_lo + lambda Q_lo Q_hi ] = sum_p eq(tau, p) [ P_lo Q_hi + Q_lo T ],
//   T = P_hi + lambda Q_hi.  T is linear in the tables, so binding a variable commutes with it: fold(T) = fold(P_hi) + lambda
//   fold(Q_hi).  T stands where P_hi stood and is folded like a table; the gate is two products a point where the lambda form
//   has four, and at the end P_hi at the challenges is T_f - lambda Q_hi_f, one product.
//
// LAYERS  Layer j, 0 <= j < m, has the tables P_lo, P_hi, Q_lo, Q_hi: the halves of layer m - 1 - j of the two trees (of the
//   leaves for j = m - 1), 2^j words each; its weight is W = eq(tau_0 .. tau_{j-2}) over row j - 1 of the points, 2^(j-1) words.
//
// ONE BODY, TWO JOBS
//   the tail of a large layer (tail != 0, 2^j > FGKR_TAIL_LEN)  The chain of launches has written lambda_j, has written T over
//     P_hi, has brought the live length down to FGKR_TAIL_LEN = 256 and has written, but not absorbed, the current row.  The block
//     loads the 256 live words of the four tables, the 128 of W and lambda_j, and loops: absorb the row -> the challenge; fold the
//     four tables, sum the weight and - while a pair is left - make the next row.  Then the claims and their transcript step.
//   whole small layers (2^j <= FGKR_TAIL_LEN)  The lambda step (count 0: the digest of the state alone) is run, W R^2 is built in
//     LDS by doubling, P_lo, Q_lo, Q_hi are loaded AS STORED and T is formed in LDS - lambda brought to Montgomery form once, one
//     product a word -, round 0 is made, then the same loop.  The launch goes on to the next layer while it fits: a tree with
//     m <= 9 is one launch.  Layer 0 has no lambda and no sumcheck: its claims are the root's four children as stored.
//   Nothing is written to the trees, the leaves or the weight: the folded words live in LDS and only four words a layer leave.
//
// LANES  256.  bind: an item is one folded word of one of the four tables, 2 x live items over the lanes (two each at 256); the
//   lanes from the top sum the weight.  round: wave t < 3 evaluates point t, lane l takes the pairs l, l + 64, ... and adds
//   W (P_lo,t Q_hi,t + Q_lo,t T_t): two products, one sum, the weight's product; the wave's sum is reduced by __shfl_down and its
//   lane 0 stores u(t).  The round runs in two passes over the lane's pairs - the sums of two products into the lane's own words
//   of LDS, then their products with the weight into the accumulator - so that three field elements, not four, are live across a
//   product: in one pass the compiler reports 129 - 131 VGPRs, in two 124 - 126.  Three barriers a round, as in k_gkr_tail.
//
// TRANSCRIPT  blz_ntt_fs_challenge's function.  lambda_j: gkr_absorb with count 0.  A row: gkr_absorb with count 3.  The claims
//   are FOUR words: with the state 160 bytes, two blocks of the 136-byte rate.  fgkr_absorb2 keeps gkr_absorb's lane layout and
//   runs the permutation twice: message lanes 0 .. 16 (the state, claims 0 .. 2 and the first 64 bits of claim 3) go into block
//   one, message lanes 17 .. 19 with the padding (0x06 in lane 3, the top bit of lane 16) into block two.
//
// WHAT IS STORED IS CANONICAL  A row word, a folded word, T, a summed weight and a claim go through fp_reduce: the chain of
//   launches and this kernel agree byte for byte because a field element has one canonical word.  Layer 0's claims are copies.
//
// MONTGOMERY POWERS  As in k_gkr_tail the weight is kept as W R^2.  mont(P_lo,t, Q_hi,t) + mont(Q_lo,t, T_t) carries 1 / R as a
//   whole, and mont(that, W R^2) is the plain term.  lambda is kept as lambda R: mont(Q_hi, lambda R) is plain.
//
// WHY EVERY INTERMEDIATE FITS  (lazy fields keep [0, 2m], the strict field [0, m); field.hip.hpp)
//   a table word goes through vec_canon before the first subtraction or product: [0, m).  T: lambda R < 2m, mont(Q_hi, lambda R)
//   is below 2m (the strict field: below m), plus P_hi in [0, m) by fp_add: its range; fp_reduce -> [0, m).  bind: hi - lo in
//   [0, 2m], times r R (< 2m) below 2m, plus lo: fp_add's range; fp_reduce.  points: lo + t d by fp_add, in range for any t.
//   THE SUM OF TWO PRODUCTS: each of mont(P_lo,t, Q_hi,t) and mont(Q_lo,t, T_t) has operands <= 2m and is below 2m (lazy: 4 m^2 /
//   R + m < 2m as 4m < R; strict: reduced below m by the product); fp_add brings their sum, at most 4m < R before its
//   conditional subtraction of 2m, back into [0, 2m] (strict: below 2m, one subtraction of m, [0, m)): an operand <= 2m for the
//   weight's product, whose other operand W R^2 is in [0, m).  A sum of terms in a lane and across a wave by fp_add stays in
//   fp_add's range whatever their number; fp_reduce makes the row word canonical.  The claim P_hi_f: T_f in [0, m) minus
//   mont(Q_hi_f, lambda R) < 2m by fp_sub: [0, 2m]; fp_reduce.  The weight by doubling: as in k_gkr_tail.
//
// HOUSE RULES  No atomics, no allocation, no scratch memory, no spinning on memory.  The block synchronises with __syncthreads
//   alone; every loop bound around a barrier is block-uniform (the arguments, the layer, the live length) and nothing returns, so
//   every lane reaches every barrier.  LDS: 4 x 8 KiB of tables, 4 KiB of weight - 36 KiB -, 12 KiB for the round's sums of two
//   products (3 waves x 128 pairs), under 2 KiB for the row, the challenge, lambda, the point row and its Montgomery forms:
//   under 50 KiB, static, below the 64 KiB a static allocation may have - which is why the largest live length is 256 and not
//   512 (72 KiB of tables and weight alone).
#pragma once
#include "ntt_gkr.hip.hpp"

namespace blz {

// (FGKR_TAIL_LEN = 256, the largest live length the block takes, stands in ntt_engine.hpp: the entry point plans by it)
static_assert(FGKR_TAIL_LEN == (uint32_t)VEC_THREADS, "a load is one word of each table per lane");
static_assert(4 * FGKR_TAIL_LEN * 32 + FGKR_TAIL_LEN / 2 * 32 == 36 * 1024, "four tables and a weight are 36 KiB");

// Keccak-f[1600] on gkr_absorb's lane layout: lane x + 5 y < 25 holds A[x, y]
BLZ_DEV uint64_t fgkr_permute(const GkrKeccakLane& k, uint64_t a) {
#pragma unroll 1
    for (int round = 0; round < 24; ++round) {
        const uint64_t c = a ^ __shfl(a, k.col1) ^ __shfl(a, k.col2) ^ __shfl(a, k.col3) ^ __shfl(a, k.col4);
        const uint64_t cr = __shfl(c, k.right);
        a ^= __shfl(c, k.left) ^ (cr << 1 | cr >> 63);
        a = a << k.rot | a >> ((64 - k.rot) & 63);
        a = __shfl(a, k.pi_src);
        a ^= ~__shfl(a, k.right) & __shfl(a, k.right2);
        if (k.lane == 0) a ^= GKR_KECCAK_RC[round];
    }
    return a;
}

// One transcript step over FOUR words by ONE whole wave: st: lanes 0 .. 3 hold the state; w: lane i < 4 holds word i as 4 x 64
// bits.  The message is 20 lanes, the rate 17: two blocks.  Returns the lane's 64 bits of the state: lanes 0 .. 3 the digest
BLZ_DEV uint64_t fgkr_absorb2(const GkrKeccakLane& k, uint64_t st, const uint64_t (&w)[4]) {
    const uint64_t x0 = __shfl(w[0], k.msg_src), x1 = __shfl(w[1], k.msg_src), x2 = __shfl(w[2], k.msg_src), x3 = __shfl(w[3], k.msg_src);
    const uint64_t y1 = __shfl(w[1], 3), y2 = __shfl(w[2], 3), y3 = __shfl(w[3], 3);   // message lanes 17, 18, 19
    const int q = k.lane & 3;
    uint64_t a = q == 0 ? x0 : q == 1 ? x1 : q == 2 ? x2 : x3;
    if (k.lane < 4) a = st;
    else if (k.lane > 16) a = 0;   // the capacity
    a = fgkr_permute(k, a);
    if (k.lane == 0) a ^= y1;
    if (k.lane == 1) a ^= y2;
    if (k.lane == 2) a ^= y3;
    if (k.lane == 3) a ^= 0x06;
    if (k.lane == 16) a ^= 0x8000000000000000ull;   // the last lane of the rate
    return fgkr_permute(k, a);
}

// where layer j's tables start in one of the trees: the halves of layer m - 1 - j, of the leaves for j = m - 1; hi = lo + 2^j words
BLZ_DEV const uint32_t* fgkr_layer(const uint32_t* tree, const uint32_t* a, uint32_t m, uint32_t j) {
    return j + 1 == m ? a : tree + ((1ull << m) - (4ull << j)) * 8;
}

// Bind the top variable of the four tables in LDS, in place, and sum the weight: `live` words in each table, live / 2 come out.
// tb: the four tables back to back, FGKR_TAIL_LEN words each
template <class Fr>
BLZ_DEV void fgkr_bind(uint32_t* tb, uint32_t* wt, uint32_t live, const Fp<Fr>& rm) {
    const uint32_t half = live >> 1, quarter = live >> 2;
#pragma unroll 1
    for (uint32_t item = threadIdx.x; item < 2 * live; item += VEC_THREADS) {
        uint32_t* const x0 = tb + ((size_t)(item / half) * FGKR_TAIL_LEN + item % half) * 8;
        Fp<Fr> x, y;
        fp_load(x, x0);
        fp_load(y, x0 + half * 8);
        vec_canon(x);
        vec_canon(y);
        fp_sub(y, y, x);
        fp_mul(y, y, rm);
        fp_add(x, x, y);
        fp_reduce(x);
        fp_store(x0, x);
    }
    const uint32_t q = VEC_THREADS - 1 - threadIdx.x;   // from the top: the lanes the fold leaves idle below 256
    if (q < quarter) {
        Fp<Fr> w, w2;
        fp_load(w, wt + q * 8);
        fp_load(w2, wt + (q + quarter) * 8);
        fp_add(w, w, w2);
        fp_reduce(w);
        fp_store(wt + q * 8, w);
    }
}

// table x at point `wave` of pair p: x[p] + wave (x[p + pairs] - x[p])
template <class Fr>
BLZ_DEV void fgkr_point(Fp<Fr>& a, const uint32_t* x, uint32_t p, uint32_t pairs, uint32_t wave) {
    Fp<Fr> d;
    fp_load(a, x + p * 8);
    fp_load(d, x + (p + pairs) * 8);
    vec_canon(a);
    vec_canon(d);
    fp_sub(d, d, a);
    if (wave >= 1) fp_add(a, a, d);
    if (wave >= 2) fp_add(a, a, d);
}

// The round polynomial over `pairs` pairs of the four tables: wave t < 3 makes u(t) = sum_p W[p] (P_lo,t Q_hi,t + Q_lo,t T_t),
// canonical, into word t of `out` (d_rounds) and of `row` (LDS).  wt holds W R^2.  Every lane calls it
template <class Fr>
BLZ_DEV void fgkr_round(const uint32_t* tb, const uint32_t* wt, uint32_t* sm, uint32_t pairs, uint32_t* row, uint32_t* out) {
    using E = Fp<Fr>;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t *pl = tb, *tt = tb + FGKR_TAIL_LEN * 8, *ql = tb + 2 * FGKR_TAIL_LEN * 8, *qh = tb + 3 * FGKR_TAIL_LEN * 8;
    if (wave < (uint32_t)GKR_POINTS) {
        // two passes, so that no more than three field elements are live across a product: the gate's sums of two products go
        // through the wave's own words of `sm`, each written and read back by the same lane
        uint32_t* const mine = sm + wave * (FGKR_TAIL_LEN / 2) * 8;
#pragma unroll 1
        for (uint32_t p = lane; p < pairs; p += 64) {
            E a, b, c;
            fgkr_point<Fr>(a, pl, p, pairs, wave);
            fgkr_point<Fr>(b, qh, p, pairs, wave);
            fp_mul(a, a, b);
            fgkr_point<Fr>(c, ql, p, pairs, wave);
            fgkr_point<Fr>(b, tt, p, pairs, wave);
            fp_mul(c, c, b);
            fp_add(a, a, c);
            fp_store(mine + p * 8, a);
        }
        E acc;
        fp_zero(acc);
#pragma unroll 1
        for (uint32_t p = lane; p < pairs; p += 64) {
            E a, b;
            fp_load(a, mine + p * 8);
            fp_load(b, wt + p * 8);
            fp_mul(a, a, b);
            fp_add(acc, acc, a);
        }
#pragma unroll 1
        for (int off = 32; off >= 1; off >>= 1) {
            E o;
#pragma unroll
            for (int k = 0; k < Fr::N; ++k) o.v[k] = __shfl_down(acc.v[k], (unsigned)off);
            fp_add(acc, acc, o);
        }
        if (lane == 0) {
            fp_reduce(acc);
            fp_store(row + wave * 8, acc);
            fp_store(out + wave * 8, acc);
        }
    }
}

// g: NttFgkrTail (ntt_engine.hpp).  One block of VEC_THREADS lanes
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_fgkr_tail(NttFgkrTail g) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t tb[4 * FGKR_TAIL_LEN * 8];   // P_lo, T (layer 0: P_hi), Q_lo, Q_hi
    __shared__ __attribute__((aligned(16))) uint32_t wt[FGKR_TAIL_LEN / 2 * 8];
    __shared__ __attribute__((aligned(16))) uint32_t sm[GKR_POINTS * FGKR_TAIL_LEN / 2 * 8];   // a point's sums of two products, per wave
    __shared__ __attribute__((aligned(16))) uint32_t row[GKR_POINTS * 8];      // the round polynomial, from the waves that made it to wave 0
    __shared__ __attribute__((aligned(16))) uint32_t chal[8];                 // the round's challenge, for every lane
    __shared__ __attribute__((aligned(16))) uint32_t lam[8];                  // the layer's lambda
    __shared__ __attribute__((aligned(16))) uint32_t pt[32 * 8];               // the point row: read for W, then rewritten by the layer
    __shared__ __attribute__((aligned(16))) uint32_t tm[FGKR_TAIL_LOG * 8];    // tau R of the weight's variables
    const uint32_t t = threadIdx.x;
    const bool wave0 = t < 64;
    const GkrKeccakLane kl = gkr_keccak_lane();
    uint32_t* const tt = tb + FGKR_TAIL_LEN * 8;
    uint32_t* const qh = tb + 3 * FGKR_TAIL_LEN * 8;
    uint64_t st = 0;
    if (t < 4) st = reinterpret_cast<const uint64_t*>(g.state)[t];
    // a launch that starts with a whole layer below the root takes that layer's point from memory; later layers find it in pt
    if (!g.tail && t < g.first) {
        const uint32_t* const src = g.points + ((size_t)(g.first - 1) * g.first / 2 + t) * 8;
        reinterpret_cast<uint4*>(pt + t * 8)[0] = reinterpret_cast<const uint4*>(src)[0];
        reinterpret_cast<uint4*>(pt + t * 8)[1] = reinterpret_cast<const uint4*>(src)[1];
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = g.first; j < g.last; ++j) {
        const uint32_t* const gp = fgkr_layer(g.tree_p, g.a_p, g.m, j);
        const uint32_t* const gq = fgkr_layer(g.tree_q, g.a_q, g.m, j);
        const size_t hi = (size_t)8 << j;   // where a layer's hi half starts
        uint32_t* const rows = g.rounds + (size_t)GKR_POINTS * (j * (j - 1u) / 2) * 8;             // layer j's rounds
        uint64_t* const prow = reinterpret_cast<uint64_t*>(g.points) + (size_t)(j * (j + 1u) / 2) * 4;   // row j of the points
        uint64_t* const pt64 = reinterpret_cast<uint64_t*>(pt);
        uint32_t live, i;
        bool made_here;   // the current row is in `row`; else the chain's last step left it in d_rounds
        // lambda_j: the chain has written it (a tail), or it is made here - the digest of the state alone
        if (j >= 1) {
            if (wave0) {
                if (g.tail) {
                    if (t < 4) reinterpret_cast<uint64_t*>(lam)[t] = reinterpret_cast<const uint64_t*>(g.lambdas + (size_t)j * 8)[t];
                } else {
                    const uint64_t none[4] = {0, 0, 0, 0};
                    st = gkr_absorb(kl, st, none, 0);
                    if (t < 4) {
                        const uint64_t c = gkr_challenge(st, t, g.keep_bits);
                        reinterpret_cast<uint64_t*>(g.lambdas + (size_t)j * 8)[t] = c;
                        reinterpret_cast<uint64_t*>(lam)[t] = c;
                    }
                }
            }
            __syncthreads();
        }
        if (g.tail) {
            live = FGKR_TAIL_LEN, i = j - FGKR_TAIL_LOG, made_here = false;
#pragma unroll 1
            for (uint32_t k = 0; k < 4; ++k) {   // T stands over P_hi
                E x;
                fp_load(x, ((k & 2u) ? gq : gp) + ((k & 1u) ? hi : 0) + (size_t)t * 8);
                fp_store(tb + ((size_t)k * FGKR_TAIL_LEN + t) * 8, x);
            }
            if (t < FGKR_TAIL_LEN / 2) {
                E w;   // the weight as the steps left it, plain: W R^2 from here on
                fp_load(w, g.weight + (size_t)t * 8);
                fp_to_mont(w, w);
                fp_to_mont(w, w);
                fp_reduce(w);
                fp_store(wt + t * 8, w);
            }
            __syncthreads();
        } else {
            live = 1u << j, i = 0, made_here = true;
            if (t < live) {
                E x, y;
                fp_load(x, gp + (size_t)t * 8);
                fp_store(tb + t * 8, x);
                fp_load(x, gq + (size_t)t * 8);
                fp_store(tb + (2 * FGKR_TAIL_LEN + t) * 8, x);
                fp_load(y, gq + hi + (size_t)t * 8);
                fp_store(qh + t * 8, y);
                fp_load(x, gp + hi + (size_t)t * 8);
                if (j >= 1) {   // T = P_hi + lambda Q_hi, canonical
                    E lm;
                    fp_load(lm, lam);
                    fp_to_mont(lm, lm);
                    vec_canon(x);
                    vec_canon(y);
                    fp_mul(y, y, lm);
                    fp_add(x, x, y);
                    fp_reduce(x);
                }
                fp_store(tt + t * 8, x);
            }
            if (j >= 1) {
                // W R^2 = eq(tau_0 .. tau_{j-2}) R^2 by doubling: k_mle_eq's top level, seeded with R^2 where that seeds with 1
                const uint32_t nv = j - 1;
                if (t < nv) {
                    E w;
                    fp_load(w, pt + t * 8);
                    fp_to_mont(w, w);
                    fp_store(tm + t * 8, w);
                }
                if (t == 0) {
                    E seed;
#pragma unroll
                    for (int k = 0; k < Fr::N; ++k) seed.v[k] = Fr::R2[k];
                    fp_store(wt, seed);
                }
                __syncthreads();
#pragma unroll 1
                for (uint32_t s = 0; s < nv; ++s) {
                    const uint32_t size = 1u << s;
                    if (t < size) {
                        E w, old, up;
                        fp_load(w, tm + s * 8);
                        fp_load(old, wt + t * 8);
                        fp_mul(up, old, w);
                        fp_sub(old, old, up);
                        fp_store(wt + t * 8, old);
                        fp_store(wt + (t + size) * 8, up);
                    }
                    __syncthreads();
                }
                if (t < (1u << nv)) {
                    E w;
                    fp_load(w, wt + t * 8);
                    fp_reduce(w);
                    fp_store(wt + t * 8, w);
                }
                __syncthreads();
                // round 0 over the pairs of the tables
                fgkr_round<Fr>(tb, wt, sm, live >> 1, row, rows);
            }
            __syncthreads();
        }
        // one pass per variable: absorb the row, bind the top variable, make the next row while a pair is left
#pragma unroll 1
        while (j >= 1 && live >= 2) {
            if (wave0) {
                E u;
                fp_zero(u);
                if (t < (uint32_t)GKR_POINTS) fp_load(u, made_here ? row + t * 8 : rows + ((size_t)i * GKR_POINTS + t) * 8);
                uint64_t w4[4];
                gkr_pack<Fr>(w4, u);
                st = gkr_absorb(kl, st, w4, GKR_POINTS);
                if (t < 4) {
                    const uint64_t c = gkr_challenge(st, t, g.keep_bits);
                    prow[(size_t)(j - 1 - i) * 4 + t] = c;   // backwards: the row ends up in bit order
                    pt64[(j - 1 - i) * 4 + t] = c;
                    reinterpret_cast<uint64_t*>(chal)[t] = c;
                }
            }
            __syncthreads();
            E rm;
            fp_load(rm, chal);
            fp_to_mont(rm, rm);
            fgkr_bind<Fr>(tb, wt, live, rm);
            live >>= 1, ++i, made_here = true;
            __syncthreads();
            if (live >= 2) {
                fgkr_round<Fr>(tb, wt, sm, live >> 1, row, rows + (size_t)i * GKR_POINTS * 8);
                __syncthreads();
            }
        }
        // the claims - the four tables at the challenges, P_hi's as T_f - lambda Q_hi_f; layer 0: the root's four children as
        // stored - and their transcript step, two blocks
        if (wave0) {
            E cw;
            fp_zero(cw);
            if (t < 4) fp_load(cw, tb + (size_t)t * FGKR_TAIL_LEN * 8);
            if (j >= 1) {
                E tf, q, lm;
                fp_load(tf, tt);
                fp_load(q, qh);
                fp_load(lm, lam);
                fp_to_mont(lm, lm);
                fp_mul(q, q, lm);
                fp_sub(tf, tf, q);
                fp_reduce(tf);
                if (t == 1) cw = tf;
            }
            if (t < 4) fp_store(g.claims + ((size_t)4 * j + t) * 8, cw);
            uint64_t w4[4];
            gkr_pack<Fr>(w4, cw);
            st = fgkr_absorb2(kl, st, w4);
            if (t < 4) {
                const uint64_t c = gkr_challenge(st, t, g.keep_bits);
                prow[(size_t)j * 4 + t] = c;
                pt64[j * 4 + t] = c;
            }
        }
        __syncthreads();
    }
    if (t < 4) reinterpret_cast<uint64_t*>(g.state)[t] = st;
}

// The claims of layer g.first alone, for the chain of launches: word 0 of the four tables into row g.first of the claims; below
// the root the second is T's and P_hi_f = T_f - lambda Q_hi_f goes out, canonical.  One wave
template <class Fr>
__global__ __launch_bounds__(64) void k_fgkr_claims(NttFgkrTail g) {
    using E = Fp<Fr>;
    const uint32_t t = threadIdx.x, j = g.first;
    const uint32_t* const gp = fgkr_layer(g.tree_p, g.a_p, g.m, j);
    const uint32_t* const gq = fgkr_layer(g.tree_q, g.a_q, g.m, j);
    const size_t hi = (size_t)8 << j;
    if (t < 4) {
        E cw;
        fp_load(cw, ((t & 2u) ? gq : gp) + ((t & 1u) ? hi : 0));
        if (j >= 1 && t == 1) {
            E q, lm;
            fp_load(q, gq + hi);
            fp_load(lm, g.lambdas + (size_t)j * 8);
            fp_to_mont(lm, lm);
            vec_canon(cw);
            vec_canon(q);
            fp_mul(q, q, lm);
            fp_sub(cw, cw, q);
            fp_reduce(cw);
        }
        fp_store(g.claims + ((size_t)4 * j + t) * 8, cw);
    }
}

// g.claims_only: k_fgkr_claims for layer g.first; else k_fgkr_tail over the layers [g.first, g.last).  The caller has checked every
// pointer and that the layers fit: tail != 0 takes ONE layer with 2^first > FGKR_TAIL_LEN, else 2^(last - 1) <= FGKR_TAIL_LEN
template <class Fr>
int ntt_fgkr_tail_t(hipStream_t st, const NttFgkrTail& g) {
    if (g.claims_only) hipLaunchKernelGGL(k_fgkr_claims<Fr>, dim3(1), dim3(64), 0, st, g);
    else hipLaunchKernelGGL(k_fgkr_tail<Fr>, dim3(1), dim3(VEC_THREADS), 0, st, g);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
