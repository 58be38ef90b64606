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
// ROUND  out[t] = sum_{p < len / 2} prod_{j < K} (lo_j + t (hi_j - lo_j)): the PRODUCT gate of ntt_sumcheck.hip.hpp without r, the
//   one kernel that takes every round polynomial; mle_pair below is the pairing both share.
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
