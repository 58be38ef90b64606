// Multilinear tables on resident buffers (blz_ntt_vec_mle_fold, blz_ntt_vec_mle_round, blz_ntt_vec_mle_eq): the three steps a
// sumcheck prover repeats log n times, templated on the scalar field like the other ops whose operands, wire format and
// 8 x 32-bit arithmetic (field.hip.hpp, vec_canon) they share.  A multilinear polynomial in m variables is its 2^m values on
// the hypercube by buffer position p = sum x_i 2^i; len = 2^m is the live length of a call and may be far below the handle's
// n, so every kernel is sized by len: nothing past the words an op owns is read or written.  Blocks never wait for one
// another - every dependency between blocks is a launch -, no atomics, no allocation.
//
// FOLD   dst[p] = lo + r (hi - lo), p < len / 2; (lo, hi) = (a[p], a[p + len / 2]), or (a[2p], a[2p + 1]) with LOW.
//   k_mle_fold has the shape of k_vec_ew.  r goes to Montgomery form once per lane (one product ahead of the grid-stride
//   loop), so the ONE product per output word, mont(hi - lo, r R), is plain already: 1 product, 2 canons, 1 sub, 1 add per word.
//   Without LOW dst may be a's words: a lane reads p and p + len / 2 before it writes p, and no other lane touches either.
//   With LOW lane p writes a word lane p / 2 reads: in place goes through the handle's scratch and a copy (ntt.hip).
//
// ROUND  out[t] = sum_{p < len / 2} prod_{j < K} (lo_j + t (hi_j - lo_j)), t < points <= 4, K <= 3 operands.
//   k_mle_round_part: the grid of k_fold_part - lane g of S = blocks x 256 owns the pairs g, g + S, ... - with `points`
//   accumulators per lane.  Per pair: 2 K loads through vec_canon, value and difference per operand; per point K - 1 raw
//   Montgomery products (the value of operand 0 times the others') and one addition into the point's accumulator, then t advances
//   by ONE addition per operand.  The loop over t is unrolled to 4 and predicated on `points`, which is wave-uniform.
//   Products per pair: points x (K - 1) - none at K = 1, 3 at K = 2 with 3 points, 8 at K = 3 with 4.
//   Each raw product leaves a factor 1 / R: every term of a sum carries the same R^-(K-1), which comes off ONCE, where the
//   final word is made (K - 1 products by R^2: DOT's rule).  One fold_block_tree per point; a call whose pairs fit one block
//   (len <= 512) finishes there and writes d_out itself - no workspace, which small handles do not have: 4 words need n >= 4 -,
//   any other writes one partial per block and point and k_mle_round_fin, one block, folds them.
//   Workspace: blocks x points words with blocks = len / 512 >= 2, so at most 4 len / 512 < len <= n words.
//
// EQ     dst[p] = prod_{i < m} (x_i tau_i + (1 - x_i)(1 - tau_i)), p < 2^m.
//   By doubling: the table of s variables becomes that of s + 1 by new[q + 2^s] = old[q] tau_s, new[q] = old[q] - new[q + 2^s]:
//   one product per PAIR.  The multiplier is tau_s R, so a table keeps the form of its seed: seeded with R it is in Montgomery
//   form, seeded with the integer 1 it is plain.  k_mle_eq works on tiles of 1024 words: a block builds the table of the level's
//   low (at most 10) variables in LDS - seeded with R, 1023 products, once -, then for each of its tiles (tile, tile + blocks, ...;
//   at most VEC_MAX_BLOCKS blocks) word q = mont(table[q], outer[tile]), where outer is the PLAIN table over the remaining
//   variables: the last product lands plain.  The outer table is built by the same kernel into the workspace, and its own outer
//   table likewise: variables [0, 10) | [10, 20) | [20, 27) at m = 27, three launches, top level first.  The top level has no
//   outer word: it seeds with the integer 1 and stores its table as it is.
//   Products per element: 1 for the outer word, and (1023 + 10 for tau R) / 1024 for the block's table divided by its tiles - two
//   while every block has one tile (m <= 21), 1 + 1 / 64 at m = 27; the upper levels add under 2 / 1024.  The longest serial
//   chain is a level's own doublings and one outer product per level above it: 10 + 1 from m = 11 on, never more than m.
//   Workspace: 2^(m - 10) + 2^(m - 20) words (at most 2^17 + 2^7), none for m <= 10.
#pragma once
#include "ntt_fold.hip.hpp"

namespace blz {

constexpr uint32_t MLE_LOW = 1u;       // BLZ_MLE_LOW
constexpr int MLE_MAX_POINTS = 4;
constexpr int MLE_MAX_OPERANDS = 3;
constexpr int MLE_EQ_LOG_TILE = 10;    // variables per level of the equality table: a tile of 1024 words, 32 KiB of LDS
constexpr uint32_t MLE_EQ_TILE = 1u << MLE_EQ_LOG_TILE;
static_assert(NTT_MAX_LOG <= 3 * MLE_EQ_LOG_TILE, "three levels build the largest equality table");

// the pair of output position p: canonical lo and hi - lo
template <class Fr, bool LOW>
BLZ_DEV void mle_pair(Fp<Fr>& lo, Fp<Fr>& diff, NttVecArg a, uint64_t p, uint64_t half) {
    Fp<Fr> hi;
    fp_load(lo, a.p + ((LOW ? 2 * p : p) & a.mask) * 8);
    fp_load(hi, a.p + ((LOW ? 2 * p + 1 : p + half) & a.mask) * 8);
    vec_canon(lo);
    vec_canon(hi);
    fp_sub(diff, hi, lo);
}

template <class Fr, bool LOW>
__global__ __launch_bounds__(VEC_THREADS) void k_mle_fold(uint32_t* dst, NttVecArg a, const uint32_t* r, uint64_t half) {
    using E = Fp<Fr>;
    E rm;
    fp_load(rm, r);
    fp_to_mont(rm, rm);
    const uint64_t stride = (uint64_t)gridDim.x * VEC_THREADS;
    for (uint64_t p = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; p < half; p += stride) {
        E lo, d;
        mle_pair<Fr, LOW>(lo, d, a, p, half);
        fp_mul(d, d, rm);
        fp_add(d, lo, d);
        fp_reduce(d);
        fp_store(dst + p * 8, d);
    }
}

// x R^-(K-1) -> x, canonical: K - 1 products by R^2
template <class Fr>
BLZ_DEV void mle_round_close(Fp<Fr>& x, int k) {
#pragma unroll 1
    for (int j = 1; j < k; ++j) fp_to_mont(x, x);
    fp_reduce(x);
}

// direct != 0 (one block): out = d_out, `points` canonical words; else out = the workspace, word t * gridDim.x + block = the
// block's partial of point t, with the stray R^-(K-1)
template <class Fr, int K, bool LOW>
__global__ __launch_bounds__(VEC_THREADS) void k_mle_round_part(uint32_t* out, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t half,
                                                                 int log_stride, uint32_t points, uint32_t direct) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    const uint64_t stride = 1ull << log_stride;   // gridDim.x * VEC_THREADS, a power of two
    E acc[MLE_MAX_POINTS];
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) fp_zero(acc[t]);
#pragma unroll 1
    for (uint64_t p = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; p < half; p += stride) {
        E v[K], d[K];
        mle_pair<Fr, LOW>(v[0], d[0], a, p, half);
        if constexpr (K > 1) mle_pair<Fr, LOW>(v[1], d[1], b, p, half);
        if constexpr (K > 2) mle_pair<Fr, LOW>(v[2], d[2], c, p, half);
#pragma unroll
        for (int t = 0; t < MLE_MAX_POINTS; ++t) {
            if (t < (int)points) {
                E pr = v[0];
#pragma unroll
                for (int j = 1; j < K; ++j) fp_mul(pr, pr, v[j]);
                fp_add(acc[t], acc[t], pr);
                if (t + 1 < MLE_MAX_POINTS) {
#pragma unroll
                    for (int j = 0; j < K; ++j) fp_add(v[j], v[j], d[j]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MLE_MAX_POINTS; ++t) {
        if (t < (int)points) {
            fold_block_tree<Fr>(x, acc[t], [](E& l, const E& r, int) { fp_add(l, l, r); });
            if (direct) {
                if (threadIdx.x == 0) {
                    E s;
                    fp_load(s, x);
                    mle_round_close(s, K);
                    fp_store(out + t * 8, s);
                }
            } else {
                vec_copy32(out + ((size_t)t * gridDim.x + blockIdx.x) * 8, x);
            }
            __syncthreads();   // x is the next point's
        }
    }
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

// One level of the equality table: tile `tile` of `tiles` is the 2^lv words out[tile 2^lv ..] = eq over the variables
// [base, base + lv) (tau[base ..], lv <= 10) times outer[tile], canonical.  outer == nullptr: the top level, one tile, no product.
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_mle_eq(uint32_t* out, const uint32_t* tau, uint32_t base, uint32_t lv, const uint32_t* outer,
                                                         uint32_t tiles) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t tab[MLE_EQ_TILE * 8];
    __shared__ __attribute__((aligned(16))) uint32_t tm[MLE_EQ_LOG_TILE * 8];
    const uint32_t t = threadIdx.x;
    if (t < lv) {
        E w;
        fp_load(w, tau + (size_t)(base + t) * 8);
        fp_to_mont(w, w);
        fp_store(tm + t * 8, w);
    }
    if (t == 0) {
        E seed;
        if (outer) {
            fp_one(seed);
        } else {
            fp_zero(seed);
            seed.v[0] = 1u;
        }
        fp_store(tab, seed);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 0; s < lv; ++s) {
        const uint32_t size = 1u << s;
        E w;
        fp_load(w, tm + s * 8);
#pragma unroll 1
        for (uint32_t q = t; q < size; q += VEC_THREADS) {
            E old, hi;
            fp_load(old, tab + q * 8);
            fp_mul(hi, old, w);
            fp_sub(old, old, hi);
            fp_store(tab + q * 8, old);
            fp_store(tab + (q + size) * 8, hi);
        }
        __syncthreads();
    }
    // the block's tiles: tile, tile + gridDim.x, ... (one each up to VEC_MAX_BLOCKS tiles; the table above is built once)
    const uint32_t size = 1u << lv;
#pragma unroll 1
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        E o;
        if (outer) fp_load(o, outer + (size_t)tile * 8);
        uint32_t* const row = out + ((size_t)tile << lv) * 8;
#pragma unroll 1
        for (uint32_t q = t; q < size; q += VEC_THREADS) {
            E v;
            fp_load(v, tab + q * 8);
            if (outer) fp_mul(v, v, o);
            fp_reduce(v);
            fp_store(row + (size_t)q * 8, v);
        }
    }
}

// dst: len / 2 words; may be a.p without MLE_LOW
template <class Fr>
int ntt_vec_mle_fold_t(hipStream_t st, uint32_t flags, uint32_t* dst, NttVecArg a, const uint32_t* r, uint64_t len) {
    const uint64_t half = len >> 1;
    const uint64_t blocks = (half + VEC_THREADS - 1) / VEC_THREADS;
    const dim3 grid((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), thr(VEC_THREADS);
    if (flags & MLE_LOW) hipLaunchKernelGGL((k_mle_fold<Fr, true>), grid, thr, 0, st, dst, a, r, half);
    else hipLaunchKernelGGL((k_mle_fold<Fr, false>), grid, thr, 0, st, dst, a, r, half);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

template <class Fr, int K>
void mle_round_launch(hipStream_t st, bool low, dim3 grid, uint32_t* out, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t half, int ls,
                      uint32_t points, uint32_t direct) {
    if (low) hipLaunchKernelGGL((k_mle_round_part<Fr, K, true>), grid, dim3(VEC_THREADS), 0, st, out, a, b, c, half, ls, points, direct);
    else hipLaunchKernelGGL((k_mle_round_part<Fr, K, false>), grid, dim3(VEC_THREADS), 0, st, out, a, b, c, half, ls, points, direct);
}

// k operands (the ones not taken: any valid NttVecArg), 1 <= points <= 4; out: `points` words; ws: the handle's scratch
template <class Fr>
int ntt_vec_mle_round_t(hipStream_t st, uint32_t flags, uint32_t* out, int k, NttVecArg a, NttVecArg b, NttVecArg c, uint32_t points,
                        uint64_t len, uint32_t* ws) {
    const uint64_t half = len >> 1;
    uint64_t blocks = (half + VEC_THREADS - 1) / VEC_THREADS;   // a power of two: half is
    if (blocks > VEC_MAX_BLOCKS) blocks = VEC_MAX_BLOCKS;
    const int ls = fold_log2(blocks) + FOLD_LOG_THREADS;
    const bool low = (flags & MLE_LOW) != 0;
    const uint32_t direct = blocks == 1 ? 1u : 0u;
    uint32_t* const part = direct ? out : ws;
    const dim3 grid((unsigned)blocks);
    switch (k) {
        case 1: mle_round_launch<Fr, 1>(st, low, grid, part, a, b, c, half, ls, points, direct); break;
        case 2: mle_round_launch<Fr, 2>(st, low, grid, part, a, b, c, half, ls, points, direct); break;
        case 3: mle_round_launch<Fr, 3>(st, low, grid, part, a, b, c, half, ls, points, direct); break;
        default: return fail(BLZ_ERR_INVALID_PARAM, "a round polynomial takes 1 to %d operands", MLE_MAX_OPERANDS);
    }
    if (!direct) hipLaunchKernelGGL(k_mle_round_fin<Fr>, dim3(1), dim3(VEC_THREADS), 0, st, out, (const uint32_t*)ws, (uint32_t)blocks, points, k);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

// dst: 2^m words; point: m words; ws: the handle's scratch (2^(m - 10) + 2^(m - 20) words of it, m > 10)
template <class Fr>
int ntt_vec_mle_eq_t(hipStream_t st, uint32_t* dst, const uint32_t* point, uint32_t m, uint32_t* ws) {
    // level i covers the variables [base[i], base[i] + lv[i]); level 0 is the destination's
    uint32_t base[3], lv[3];
    uint32_t* out[3];
    int levels = 0;
    uint32_t* next = ws;
    for (uint32_t b = 0; levels == 0 || b < m; ++levels) {
        base[levels] = b;
        lv[levels] = m - b < (uint32_t)MLE_EQ_LOG_TILE ? m - b : (uint32_t)MLE_EQ_LOG_TILE;
        b += lv[levels];
        out[levels] = levels == 0 ? dst : next;
        if (levels > 0) next += ((size_t)8 << (m - base[levels]));
    }
    for (int i = levels - 1; i >= 0; --i) {
        const uint32_t tiles = 1u << (m - base[i] - lv[i]);
        hipLaunchKernelGGL(k_mle_eq<Fr>, dim3(tiles < VEC_MAX_BLOCKS ? tiles : VEC_MAX_BLOCKS), dim3(VEC_THREADS), 0, st, out[i], point, base[i], lv[i],
                           i + 1 < levels ? (const uint32_t*)out[i + 1] : (const uint32_t*)nullptr, tiles);
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
