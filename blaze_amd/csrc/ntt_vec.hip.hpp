// Element-wise polynomial ops on resident buffers (blz_ntt_vec_op), templated on the scalar field like the transform's kernels.
//
// Words are plain canonical integers on the wire, as everywhere in the NTT; any 256-bit input counts as its residue.  The 8 x 32-bit
// arithmetic of field.hip.hpp is used as it stands: these kernels stream 64 - 128 bytes per element and a 9-limb conversion
// would buy nothing.
//   * product of two wire words = two Montgomery products: b' = mont(b, R^2) = b R is below 2m for ANY 256-bit b, then
//     mont(a, b') = a b is below 3m for any 256-bit a (strict field: below 2m, reduced by the product itself) - so the
//     product needs no reduction of its inputs, only fp_reduce on the way out;
//   * sums and differences take their inputs through vec_canon: one quotient estimate from the top limb, one subtraction.
//   * BLZ_VEC_INV is Montgomery's trick as a product tree: k_vec_inv_up multiplies each tile of NTT_VEC_INV_TILE elements down to
//     one total (4 elements per lane, a 256-leaf tree in LDS), k_vec_inv_mid inverts the totals (the trick once more, eight to a lane, one Fermat chain each),
//     k_vec_inv_down rebuilds the tile's tree, pushes the inverse from the root to the leaves (the inverse of a child is the
//     inverse of its parent times its sibling) and unwinds the lane's four elements.  Zeros enter the products as the
//     identity and leave as 0.  Per element: 12 / 4 products in the lanes, 2 x 255 + 510 per 1024 in the trees, under 0.06 in k_vec_inv_mid.
//     The products run on the raw words: mont(x, y) = x y / R is associative, R (Montgomery one) is its identity, and the
//     stray powers of R come off in k_vec_inv_mid (two products by the integer 1 per tile).
// dst may alias any operand: every lane reads the elements it owns before it writes them, and owns them alone.
#pragma once
#include "ntt_engine.hpp"
#include "field.hip.hpp"

namespace blz {

constexpr int VEC_THREADS = 256;
constexpr unsigned VEC_MAX_BLOCKS = 2048;   // 256 CUs x 8 blocks: the rest of a large vector is walked by the grid-stride loop
constexpr int VEC_INV_PER_LANE = 4;
static_assert(NTT_VEC_INV_TILE == (uint64_t)VEC_THREADS * VEC_INV_PER_LANE, "tile = block x elements per lane");

// any 256-bit word -> its residue in [0, m).  q = floor(top limb / (m's top limb + 1)) never exceeds floor(x / m) and falls
// short of it by at most one (m's top limb is above 2^28 in all three fields: the estimate's error is below 2^-20), so x - q m
// is below 2m.
template <class P>
BLZ_DEV void vec_canon(Fp<P>& x) {
    constexpr int N = P::N;
    const uint32_t q = x.v[N - 1] / (P::MOD[N - 1] + 1u);
    uint32_t carry = 0, br = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t pr = (uint64_t)q * P::MOD[i] + carry;
        carry = (uint32_t)(pr >> 32);
        x.v[i] = sub_bb(x.v[i], (uint32_t)pr, br);
    }
    fp_csub_const<P, P::MOD>(x);
}

// r = a b (wire words in, residue below 3m out - canonical in the strict field): two Montgomery products
template <class P>
BLZ_DEV void vec_mul(Fp<P>& r, const Fp<P>& a, const Fp<P>& b) {
    Fp<P> bm;
    fp_to_mont(bm, b);
    fp_mul(r, a, bm);
}

// r = r / R: the product by the integer 1 strips one Montgomery factor
template <class P>
BLZ_DEV void vec_strip_mont(Fp<P>& r) {
    const Fp<P> one{{1u}};
    fp_mul(r, r, one);
}

// one 32-byte word between LDS and global memory by two lanes, 16 bytes each; every lane calls it
BLZ_DEV void vec_copy32(uint32_t* dst, const uint32_t* src) {
    if (threadIdx.x < 2) reinterpret_cast<uint4*>(dst)[threadIdx.x] = reinterpret_cast<const uint4*>(src)[threadIdx.x];
}

enum { VEC_ADD = 0, VEC_SUB = 1, VEC_MUL = 2, VEC_MULADD = 3, VEC_MULSUB = 4, VEC_INV = 5 };   // enum blz_vec_op

// the five arithmetic ops: one element per lane per step, 2 x 16 bytes per operand, a wave touches 2 KiB contiguous
template <class Fr, int OP>
__global__ __launch_bounds__(VEC_THREADS) void k_vec_ew(uint32_t* dst, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t n) {
    using E = Fp<Fr>;
    const uint64_t stride = (uint64_t)gridDim.x * VEC_THREADS;
    for (uint64_t e = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; e < n; e += stride) {
        E x, y, r;
        fp_load(x, a.p + (e & a.mask) * 8);
        fp_load(y, b.p + (e & b.mask) * 8);
        if constexpr (OP == VEC_ADD || OP == VEC_SUB) {
            vec_canon(x);
            vec_canon(y);
            if constexpr (OP == VEC_ADD) fp_add(r, x, y); else fp_sub(r, x, y);
        } else {
            vec_mul(r, x, y);
            if constexpr (OP != VEC_MUL) {
                E z;
                fp_load(z, c.p + (e & c.mask) * 8);
                vec_canon(z);
                fp_reduce(r);
                if constexpr (OP == VEC_MULADD) fp_add(r, r, z); else fp_sub(r, r, z);
            }
        }
        fp_reduce(r);
        fp_store(dst + e * 8, r);
    }
}

// ---- batch inversion
BLZ_DEV uint32_t* vec_node(uint32_t* tree, uint32_t i) { return tree + (size_t)i * 8; }

// The lane's elements (tile position j * 256 + lane: a wave's loads stay contiguous), canonical, zeros (and positions past n)
// replaced by the identity; pre[j] = x[0] .. x[j] under mont; the leaves' products climb the tree in LDS (node i = node 2i x
// node 2i + 1, leaves 256 .. 511) to the tile's total in node 1.  Returns the zero mask.
template <class Fr, bool KEEP>
BLZ_DEV uint32_t vec_inv_climb(uint32_t* tree, NttVecArg a, uint64_t base, uint64_t n, Fp<Fr> (&x)[VEC_INV_PER_LANE],
                               Fp<Fr> (&pre)[VEC_INV_PER_LANE]) {
    using E = Fp<Fr>;
    const uint32_t t = threadIdx.x;
    uint32_t zero = 0;
#pragma unroll
    for (int j = 0; j < VEC_INV_PER_LANE; ++j) {
        const uint64_t e = base + (uint64_t)j * VEC_THREADS + t;
        bool z = true;
        if (e < n) {
            fp_load(x[j], a.p + (e & a.mask) * 8);
            vec_canon(x[j]);
            uint32_t o = 0;
#pragma unroll
            for (int i = 0; i < Fr::N; ++i) o |= x[j].v[i];
            z = o == 0;
        }
        if (z) {
            zero |= 1u << j;
            fp_one(x[j]);
        }
    }
    E acc = x[0];
    if constexpr (KEEP) pre[0] = acc;
#pragma unroll
    for (int j = 1; j < VEC_INV_PER_LANE; ++j) {
        fp_mul(acc, acc, x[j]);
        if constexpr (KEEP) pre[j] = acc;
    }
    fp_store(vec_node(tree, VEC_THREADS + t), acc);
    __syncthreads();
    for (uint32_t w = VEC_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) {
            E l, r;
            fp_load(l, vec_node(tree, 2 * (w + t)));
            fp_load(r, vec_node(tree, 2 * (w + t) + 1));
            fp_mul(l, l, r);
            fp_store(vec_node(tree, w + t), l);
        }
        __syncthreads();
    }
    return zero;
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_vec_inv_up(uint32_t* totals, NttVecArg a, uint64_t n) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t tree[2 * VEC_THREADS * 8];
    E x[VEC_INV_PER_LANE], pre[VEC_INV_PER_LANE];
    (void)vec_inv_climb<Fr, false>(tree, a, (uint64_t)blockIdx.x * NTT_VEC_INV_TILE, n, x, pre);
    vec_copy32(totals + (size_t)blockIdx.x * 8, vec_node(tree, 1));
}

// m - 2, the exponent of Fermat's inversion
template <class P>
struct VecExp {
    uint32_t w[P::N];
    constexpr VecExp() : w{} {
        uint32_t br = 2;
        for (int i = 0; i < P::N; ++i) {
            w[i] = P::MOD[i] - br;
            br = P::MOD[i] < br ? 1u : 0u;
        }
    }
};
// r = R^2 / x under mont (the Montgomery form of 1 / a for x = a R): x^(m - 2), square and multiply from the top bit.  Inline and
// loop-carried in registers: fp_inv (field.hip.hpp) is a call with a stack frame, and these kernels stay out of scratch.
template <class P>
BLZ_DEV void vec_inv_fermat(Fp<P>& r, const Fp<P>& x) {
    static constexpr VecExp<P> EXP{};
    fp_one(r);
    for (int i = mp_mod_bits<P>() - 1; i >= 0; --i) {
        fp_sqr(r, r);
        if ((EXP.w[i >> 5] >> (i & 31)) & 1u) fp_mul(r, r, x);
    }
}

// totals[i] = T (the raw product of a tile: R x the product of its elements / R each)  ->  1 / T.  The trick once more: a lane
// takes VEC_MID_GROUP consecutive totals, inverts their product (vec_inv_fermat gives R^2 / T; two products by the integer 1 take
// the R^2 off - then every later product of the unwinding, here and in the leaves, yields plain inverses) and unwinds it:
// (2 (G - 1) + (G - 1) + 2 + about 380) / G products per total, under 0.06 per element.
constexpr int VEC_MID_GROUP = 8;
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_vec_inv_mid(uint32_t* totals, uint64_t count) {
    using E = Fp<Fr>;
    const uint64_t first = ((uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x) * VEC_MID_GROUP;
    if (first >= count) return;
    const int cnt = count - first < (uint64_t)VEC_MID_GROUP ? (int)(count - first) : VEC_MID_GROUP;
    uint32_t* const tp = totals + first * 8;
    E pre[VEC_MID_GROUP];   // pre[k] = t[0] .. t[k]; past cnt: the last product again
    fp_load(pre[0], tp);
#pragma unroll
    for (int k = 1; k < VEC_MID_GROUP; ++k) {
        pre[k] = pre[k - 1];
        if (k < cnt) {
            E tk;
            fp_load(tk, tp + k * 8);
            fp_mul(pre[k], pre[k - 1], tk);
        }
    }
    E inv;
    vec_inv_fermat(inv, pre[VEC_MID_GROUP - 1]);
    vec_strip_mont(inv);
    vec_strip_mont(inv);
#pragma unroll
    for (int k = VEC_MID_GROUP - 1; k >= 1; --k) {
        if (k < cnt) {
            E tk, out;
            fp_load(tk, tp + k * 8);
            fp_mul(out, inv, pre[k - 1]);
            fp_mul(inv, inv, tk);
            fp_store(tp + k * 8, out);
        }
    }
    fp_store(tp, inv);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_vec_inv_down(uint32_t* dst, const uint32_t* totals, NttVecArg a, uint64_t n) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t tree[2 * VEC_THREADS * 8];
    __shared__ __attribute__((aligned(16))) uint32_t inv[2 * VEC_THREADS * 8];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * NTT_VEC_INV_TILE;
    E x[VEC_INV_PER_LANE], pre[VEC_INV_PER_LANE];
    const uint32_t zero = vec_inv_climb<Fr, true>(tree, a, base, n, x, pre);
    vec_copy32(vec_node(inv, 1), totals + (size_t)blockIdx.x * 8);
    __syncthreads();
    // root to leaves: the inverse of a node is the inverse of its parent times its sibling
    for (uint32_t w = 1; w <= VEC_THREADS / 2; w <<= 1) {
        if (t < 2 * w) {
            const uint32_t ch = 2 * w + t;
            E p, s;
            fp_load(p, vec_node(inv, ch >> 1));
            fp_load(s, vec_node(tree, ch ^ 1u));
            fp_mul(p, p, s);
            fp_store(vec_node(inv, ch), p);
        }
        __syncthreads();
    }
    E jv;
    fp_load(jv, vec_node(inv, VEC_THREADS + t));   // 1 / (x[0] .. x[3])
#pragma unroll
    for (int j = VEC_INV_PER_LANE - 1; j >= 0; --j) {
        E out;
        if (j > 0) {
            fp_mul(out, jv, pre[j - 1]);
            fp_mul(jv, jv, x[j]);   // 1 / (x[0] .. x[j - 1])
        } else {
            out = jv;
        }
        fp_reduce(out);
        if (zero & (1u << j)) fp_zero(out);
        const uint64_t e = base + (uint64_t)j * VEC_THREADS + t;
        if (e < n) fp_store(dst + e * 8, out);
    }
}

template <class Fr, int OP>
void vec_launch_ew(hipStream_t st, uint32_t* dst, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t n) {
    const uint64_t blocks = (n + VEC_THREADS - 1) / VEC_THREADS;
    hipLaunchKernelGGL((k_vec_ew<Fr, OP>), dim3((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), dim3(VEC_THREADS), 0, st,
                       dst, a, b, c, n);
}

template <class Fr>
int ntt_vec_op_t(hipStream_t st, int op, uint32_t* dst, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t n, uint32_t* totals) {
    switch (op) {
        case VEC_ADD: vec_launch_ew<Fr, VEC_ADD>(st, dst, a, b, b, n); break;
        case VEC_SUB: vec_launch_ew<Fr, VEC_SUB>(st, dst, a, b, b, n); break;
        case VEC_MUL: vec_launch_ew<Fr, VEC_MUL>(st, dst, a, b, b, n); break;
        case VEC_MULADD: vec_launch_ew<Fr, VEC_MULADD>(st, dst, a, b, c, n); break;
        case VEC_MULSUB: vec_launch_ew<Fr, VEC_MULSUB>(st, dst, a, b, c, n); break;
        case VEC_INV: {
            const uint64_t tiles = (n + NTT_VEC_INV_TILE - 1) / NTT_VEC_INV_TILE;
            hipLaunchKernelGGL(k_vec_inv_up<Fr>, dim3((unsigned)tiles), dim3(VEC_THREADS), 0, st, totals, a, n);
            hipLaunchKernelGGL(k_vec_inv_mid<Fr>, dim3((unsigned)((tiles + (uint64_t)VEC_THREADS * VEC_MID_GROUP - 1) / ((uint64_t)VEC_THREADS * VEC_MID_GROUP))), dim3(VEC_THREADS), 0, st, totals, tiles);
            hipLaunchKernelGGL(k_vec_inv_down<Fr>, dim3((unsigned)tiles), dim3(VEC_THREADS), 0, st, dst, (const uint32_t*)totals, a, n);
            break;
        }
        default: return fail(BLZ_ERR_INVALID_PARAM, "unknown element-wise op %d", op);
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
