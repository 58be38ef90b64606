// Product and fraction trees over a multilinear table (blz_ntt_mle_tree): every layer of the binary tree under 2^m words, the
// input of a GKR grand product (PROD) or of a logUp fractional sum (FRAC), templated on the scalar field like the other ops whose
// operands, wire format and 8 x 32-bit arithmetic (field.hip.hpp, vec_canon) they share.  Layer 0 is the source, len = 2^m words
// read at p & mask; layer k, 1 <= k <= m, holds len / 2^k words:
//   PROD  L_{k+1}[p] = lo hi
//   FRAC  (P, Q)_{k+1}[p] = (P_lo Q_hi + P_hi Q_lo, Q_lo Q_hi)     - the sum of two fractions, never inverted, no case for Q = 0
// with (lo, hi) = (L_k[p], L_k[p + size / 2]), or (L_k[2p], L_k[2p + 1]) with LOW.  A layer of s words sits at word len - 2s of the
// destination (layer 1 at 0, layer 2 at len / 2, the root at len - 2): len - 1 words in all, and not a byte behind them.  Blocks
// never wait for one another - every dependency between blocks is a launch -, no atomics, no allocation, no workspace.
//
// k_tree_up   a lane owns ONE node of the layer J levels above the one it reads: it loads the 2^J leaves under it, multiplies the
//   sub-tree in registers and stores every node of the J layers, 2^J - 1 of them.  Default pairing: with T nodes in the top layer
//   the leaves are q + i T, i < 2^J, the nodes of level j are q + i T, i < 2^(J - j): every load and store instruction is
//   contiguous across lanes.  LOW: the leaves are 2^J q + i, a run of 32 x 2^J bytes per lane, the nodes of level j 2^(J - j) q + i.
//   The sub-tree is walked depth first (tree_sub): one value per level is held beside the pair in hand, not 2^J leaves.
//   J is fixed per op: 3 for PROD (8 words of leaves), 2 for FRAC (4 pairs); at most 114 VGPRs, 0 scratch, under the family's 128.  The grid-stride loop of k_vec_ew, VEC_THREADS x at most VEC_MAX_BLOCKS.  The first launch reads the
//   source through its mask, the later ones the previous top layer out of the destination.
// k_tree_top  once a layer holds at most TREE_TOP words (1024: 32 KiB of LDS per table) ONE block finishes: the layer goes to LDS
//   as it is, then level after level a lane reads the pairs of its (at most two) nodes, all lanes meet, it writes the nodes to LDS
//   and to the destination, all lanes meet again.  len <= 1024 is this kernel alone, straight from the source.
// Launches: ceil((m - 10) / J) of k_tree_up, then k_tree_top: 7 at m = 27 for PROD, 10 for FRAC.
//
// PRODUCTS  The words are plain, so mont(lo, hi) would carry 1 / R.  tree_mul(lo, hi) = mont(lo, mont(hi, R^2)): the constant goes
//   in FIRST, which leaves the node plain - the word that is stored is the word the next level multiplies - and bounds the
//   second product for ANY 256-bit lo (below).  PROD: 2 products per node.  FRAC: mont(Q_lo, R^2), mont(Q_hi, R^2), then
//   P_lo Q_hi', P_hi Q_lo', Q_lo Q_hi': 5 per node.  Traffic: the leaves once, len - 1 words out, and the top layer of every
//   launch but the last read back: (2 + 1 / (2^J - 1)) len words for PROD, 2.14 len; FRAC twice (2 + 1 / 3) len.
//
// WHY EVERY INTERMEDIATE FITS  mont(a, b) = (a b + q m) / R < a b / R + m, and a raw word is below R = 2^256.
//   hi' = mont(hi raw, R^2 < m) is below 2m; strict field (BLS12-381, 4m > R): fp_mul subtracts m once, below m.
//   mont(lo raw, hi') is below 2m R / R + m = 3m - lazy fields (BLS12-377, BN254: 4m < R): no ninth word, and fp_reduce's two
//   subtractions of m bring it below m; strict: below 2m before fp_mul's own subtraction, canonical after it.
//   FRAC's sum: each product goes below 2m (tree_csub) before fp_add, which keeps [0, 2m]; fp_reduce makes it canonical.
//   Every stored word goes through fp_reduce: canonical, whatever 256-bit words the source holds.
#pragma once
#include "ntt_mle.hip.hpp"

namespace blz {

enum { TREE_PROD = 0, TREE_FRAC = 1 };   // enum blz_tree_op
constexpr int NTT_TREE_OPS = 2;
constexpr int TREE_LOG_TOP = 10;         // k_tree_top takes a layer of at most 1024 words: 32 KiB of LDS per table
constexpr uint32_t TREE_TOP = 1u << TREE_LOG_TOP;
constexpr int tree_levels(int op) { return op == TREE_PROD ? 3 : 2; }   // J of k_tree_up

// a node: one word (PROD) or the fraction's numerator and denominator (FRAC)
template <class Fr, int OP>
struct TreeVal {
    Fp<Fr> v[OP == TREE_FRAC ? 2 : 1];
};
// the op's tables, source and destination: [0] the values / numerators, [1] the denominators (FRAC)
struct TreeSrc {
    NttVecArg t[2];
};
struct TreeDst {
    uint32_t* t[2];
};

template <class Fr, int OP>
BLZ_DEV void tree_load(TreeVal<Fr, OP>& x, const TreeSrc& s, uint64_t p) {
#pragma unroll
    for (int c = 0; c < (OP == TREE_FRAC ? 2 : 1); ++c) fp_load(x.v[c], s.t[c].p + (p & s.t[c].mask) * 8);
}
template <class Fr, int OP>
BLZ_DEV void tree_store(const TreeDst& d, uint64_t p, const TreeVal<Fr, OP>& x) {
#pragma unroll
    for (int c = 0; c < (OP == TREE_FRAC ? 2 : 1); ++c) fp_store(d.t[c] + p * 8, x.v[c]);
}
// lazy fields: [0, 3m) -> [0, 2m), what fp_add takes
template <class Fr>
BLZ_DEV void tree_csub(Fp<Fr>& x) {
    if constexpr (Fr::LAZY) fp_csub_const<Fr, Fr::MOD>(x);
}

// out = the parent of lo and hi, canonical; lo and hi any 256-bit words
template <class Fr, int OP>
BLZ_DEV void tree_node(TreeVal<Fr, OP>& out, const TreeVal<Fr, OP>& lo, const TreeVal<Fr, OP>& hi) {
    using E = Fp<Fr>;
    if constexpr (OP == TREE_PROD) {
        E hm;
        fp_to_mont(hm, hi.v[0]);
        fp_mul(out.v[0], lo.v[0], hm);
        fp_reduce(out.v[0]);
    } else {
        // an input is dropped as soon as its last product is taken: hi's denominator, lo's numerator, lo's denominator, hi's numerator
        // - and the five products stay one after the other (two interleaved hold two sets of columns: past 128 VGPRs)
        E m, x, y, q;
        fp_to_mont(m, hi.v[1]);
        __builtin_amdgcn_sched_barrier(0);
        fp_mul(x, lo.v[0], m);
        __builtin_amdgcn_sched_barrier(0);
        fp_mul(q, lo.v[1], m);
        __builtin_amdgcn_sched_barrier(0);
        fp_to_mont(m, lo.v[1]);
        __builtin_amdgcn_sched_barrier(0);
        fp_mul(y, hi.v[0], m);
        __builtin_amdgcn_sched_barrier(0);
        tree_csub(x);
        tree_csub(y);
        fp_add(x, x, y);
        fp_reduce(x);
        fp_reduce(q);
        out.v[0] = x;
        out.v[1] = q;
    }
}

// out = node I of the layer D levels above src in lane q's sub-tree, stored on the way (D == 0: leaf I, loaded).  Depth first: a
// node's two sub-trees one after the other, so at most one value per level is held beside the pair in hand, and the loads of
// the second sub-tree stand behind the stores of the first
template <class Fr, int OP, bool LOW, int D, int I>
BLZ_DEV void tree_sub(TreeVal<Fr, OP>& out, const TreeDst& dst, const TreeSrc& src, uint64_t q, uint64_t top, uint64_t cur, uint64_t len) {
    constexpr int J = tree_levels(OP);
    if constexpr (D == 0) {
        tree_load<Fr, OP>(out, src, LOW ? (q << J) + I : q + I * top);
    } else {
        TreeVal<Fr, OP> lo, hi;
        tree_sub<Fr, OP, LOW, D - 1, LOW ? 2 * I : I>(lo, dst, src, q, top, cur, len);
        tree_sub<Fr, OP, LOW, D - 1, LOW ? 2 * I + 1 : I + (1 << (J - D))>(hi, dst, src, q, top, cur, len);
        tree_node<Fr, OP>(out, lo, hi);
        tree_store<Fr, OP>(dst, len - (cur >> (D - 1)) + (LOW ? (q << (J - D)) + I : q + I * top), out);   // the layer of s = cur >> D words: at len - 2s
    }
}

// src: a layer of `cur` words, cur >= 2^J; the J layers above it go to dst, a layer of s words at word len - 2s
template <class Fr, int OP, bool LOW>
__global__ __launch_bounds__(VEC_THREADS) void k_tree_up(TreeDst dst, TreeSrc src, uint64_t cur, uint64_t len) {
    constexpr int J = tree_levels(OP);
    const uint64_t top = cur >> J;
    const uint64_t stride = (uint64_t)gridDim.x * VEC_THREADS;
#pragma unroll 1
    for (uint64_t q = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; q < top; q += stride) {
        TreeVal<Fr, OP> root;
        tree_sub<Fr, OP, LOW, J, 0>(root, dst, src, q, top, cur, len);
    }
}

// src: a layer of `cur` words, 2 <= cur <= TREE_TOP; every layer above it goes to dst.  One block
template <class Fr, int OP, bool LOW>
__global__ __launch_bounds__(VEC_THREADS) void k_tree_top(TreeDst dst, TreeSrc src, uint32_t cur, uint64_t len) {
    constexpr int C = OP == TREE_FRAC ? 2 : 1;
    constexpr int PER = TREE_TOP / 2 / VEC_THREADS;   // nodes of the largest level per lane
    using V = TreeVal<Fr, OP>;
    __shared__ __attribute__((aligned(16))) uint32_t tab[C][TREE_TOP * 8];
    const uint32_t t = threadIdx.x;
    for (uint32_t p = t; p < cur; p += VEC_THREADS) {
        V x;
        tree_load<Fr, OP>(x, src, p);
#pragma unroll
        for (int c = 0; c < C; ++c) fp_store(tab[c] + p * 8, x.v[c]);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t half = cur >> 1; half >= 1; half >>= 1) {
        V r[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t p = t + k * VEC_THREADS;
            if (p < half) {
                V lo, hi;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    fp_load(lo.v[c], tab[c] + (LOW ? 2 * p : p) * 8);
                    fp_load(hi.v[c], tab[c] + (LOW ? 2 * p + 1 : p + half) * 8);
                }
                tree_node<Fr, OP>(r[k], lo, hi);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t p = t + k * VEC_THREADS;
            if (p < half) {
#pragma unroll
                for (int c = 0; c < C; ++c) fp_store(tab[c] + p * 8, r[k].v[c]);
                tree_store<Fr, OP>(dst, len - 2 * (uint64_t)half + p, r[k]);
            }
        }
        __syncthreads();
    }
}

template <class Fr, int OP, bool LOW>
int ntt_mle_tree_launch(hipStream_t st, TreeDst dst, TreeSrc src, uint64_t len) {
    constexpr int J = tree_levels(OP);
    uint64_t cur = len;
    while (cur > TREE_TOP) {
        const uint64_t top = cur >> J, blocks = (top + VEC_THREADS - 1) / VEC_THREADS;
        hipLaunchKernelGGL((k_tree_up<Fr, OP, LOW>), dim3((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), dim3(VEC_THREADS), 0, st, dst,
                           src, cur, len);
        // the next launch reads the layer this one left on top: `top` words at word len - 2 top
        for (int c = 0; c < 2; ++c) src.t[c] = NttVecArg{dst.t[c] ? dst.t[c] + (len - 2 * top) * 8 : nullptr, top - 1};
        cur = top;
    }
    hipLaunchKernelGGL((k_tree_top<Fr, OP, LOW>), dim3(1), dim3(VEC_THREADS), 0, st, dst, src, (uint32_t)cur, len);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

// dst / dst_q: len - 1 words each (dst_q and a_q: FRAC alone); no destination word may be a word the op reads of a source
template <class Fr>
int ntt_mle_tree_t(hipStream_t st, uint32_t op, uint32_t flags, uint32_t* dst, uint32_t* dst_q, NttVecArg a, NttVecArg a_q, uint64_t len) {
    const TreeDst d{{dst, dst_q}};
    const TreeSrc s{{a, a_q}};
    const bool low = flags & MLE_LOW;
    if (op == TREE_PROD) return low ? ntt_mle_tree_launch<Fr, TREE_PROD, true>(st, d, s, len) : ntt_mle_tree_launch<Fr, TREE_PROD, false>(st, d, s, len);
    return low ? ntt_mle_tree_launch<Fr, TREE_FRAC, true>(st, d, s, len) : ntt_mle_tree_launch<Fr, TREE_FRAC, false>(st, d, s, len);
}

}  // namespace blz
