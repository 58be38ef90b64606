// Weighted (Horner) scans along a resident buffer (blz_ntt_vec_horner): dst[p] = a[p] + z dst[p - 1], forward or - with the
// position p mapped to n - 1 - p on the wire - from the top down, inclusive or exclusive.  Reverse + exclusive is synthetic
// division by X - z.  Operands, wire format and arithmetic are those of ntt_fold.hip.hpp, and so are the house rules: blocks never
// wait for one another (every dependency between blocks is a launch), no atomics, no allocation.
//
// ONE WORD PER SEGMENT.  A segment of 2^k positions is summarised by its own inclusive value S = sum_j a[j] z^(len - 1 - j); two
// neighbours combine as L z^|R| + R, and |R| is known from the level of the tree: only the powers z^(2^i) are ever needed.
// They are kept in Montgomery form, so mont(x, z^(2^i) R) = x z^(2^i) keeps plain values plain: elements enter through vec_canon
// and leave through fp_reduce, nothing is converted and no power of 1 / R builds up (SCAN_PROD pays a product per word for that).
//
// Reduce-then-scan over tiles of NTT_FOLD_TILE = 1024 positions, lane t owning the FOUR CONSECUTIVE positions 4t .. 4t + 3:
//   k_horner_pow   one block, one lane: pw[i] = z^(2^i) R, i < logn, squared ONCE per op (a 2^27 vector is 131072 short blocks;
//                  squaring inside each would cost about as much as the block's own work).  A block copies the <= 9 it uses to LDS.
//   k_horner_up    one total per tile: the lane's Horner value (3 products by Z), then a 256-leaf LDS tree x[t] = x[t] Z^(4w) +
//                  x[t + w] (255 products per tile).
//   k_horner_down  the tile again with a carry-in: the lane's Horner value (3), the carry enters as a virtual element ahead of
//                  lane 0 (lane 0's value += Z^4 carry, 1), a Kogge-Stone scan of the lanes' values in LDS (step k: x[t] = x[t - 2^k]
//                  Z^(4 2^k) + x[t], 8 steps), then the recurrence once more from the value before the lane (4 products by Z), which
//                  yields the four outputs with no per-position power.  Every lane reads what it owns before it writes it, and
//                  owns it alone: dst may be the buffer a names, in both directions.
//   Z = z^(2^base) is the level's multiplier: the tiles' totals obey the same recurrence with Z = z^1024 (exclusive, in place,
//   WIRE = false) and theirs with Z = z^(2^20), along the scans' ladder (scan_ladder, ntt_fold.hip.hpp).
//   Totals stay in logical order; REVERSE only mirrors the wire loads and stores (contiguous still, descending).
//   A block scans only as many lanes as hold elements: ceil(log2(lanes)) Kogge-Stone steps.  The largest power any block reads
//   is therefore z^(2^(logn - 1)) - in the one block over the top level's totals.
//   Products per element: up 3/4 + 255/1024, down (3 + 8 + 4)/4 + 1/1024 (the carry's, lane 0's alone) -> 4.75, and as much
//   again per 1024 elements for the totals' level.  What the SIMDs issue is 5.125: a tree level narrower than a wave still
//   occupies one (9 wave-products per tile, not 255 / 64), and so does the carry's product.
//   Nothing is special-cased for zeros: 0^0 = 1 because position p's own term is never multiplied.
//
// WORKSPACE: the handle's `scratch`.  n <= 1024: none (one block, no carry; lane 0 squares the <= 9 powers into LDS).  Else the
//   scans' levels and, behind them, the logn powers: scan_plan and scan_ws_words (ntt_fold.hip.hpp), bounded there.
#pragma once
#include "ntt_fold.hip.hpp"

namespace blz {

enum { HORNER_EXCLUSIVE = 1, HORNER_REVERSE = 2 };   // BLZ_HORNER_*
constexpr int HORNER_LOG_TILE = 10;
static_assert(NTT_FOLD_TILE == 1ull << HORNER_LOG_TILE, "a level's multiplier is z^(tile^level)");
constexpr int HORNER_SLOTS = 1 + FOLD_LOG_THREADS;   // LDS: slot 0 = Z, slot 1 + k = Z^(4 2^k), k < 8

// pw[i] = z^(2^i) in Montgomery form, i < npow
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_horner_pow(uint32_t* pw, const uint32_t* z, int npow) {
    if (threadIdx.x == 0) fold_square_chain<Fr>(pw, z, npow);
}

// The block's powers -> LDS: slot 0 = Z = z^(2^base), slot 1 + k = Z^(4 2^k) for k < ks.  pwg: k_horner_pow's table, or nullptr
// (the single block of a short vector, base 0): lane 0 squares them from z.  Every lane calls it.
template <class Fr>
BLZ_DEV void horner_powers(uint32_t* pw, const uint32_t* z, const uint32_t* pwg, int base, int ks) {
    const uint32_t t = threadIdx.x;
    if (pwg) {
        if (t < 2u * (1 + ks)) {
            const uint32_t slot = t >> 1;
            const uint32_t* src = pwg + (size_t)(slot == 0 ? base : base + 1 + slot) * 8;
            reinterpret_cast<uint4*>(pw + slot * 8)[t & 1] = reinterpret_cast<const uint4*>(src)[t & 1];
        }
    } else if (t == 0) {
        Fp<Fr> p;
        fp_load(p, z);
        fp_to_mont(p, p);
        fp_store(pw, p);
        if (ks > 0) {
            fp_sqr(p, p);
            fp_sqr(p, p);
            fp_store(pw + 8, p);
#pragma unroll 1
            for (int k = 1; k < ks; ++k) {
                fp_sqr(p, p);
                fp_store(pw + (1 + k) * 8, p);
            }
        }
    }
    __syncthreads();
}

// the lane's four consecutive elements (WIRE: from 256-bit words, position e at word n - 1 - e when rev; else as the level
// below left them), zero past `count`
template <class Fr, bool WIRE>
BLZ_DEV void horner_load(Fp<Fr> (&x)[FOLD_PER_LANE], NttVecArg a, uint64_t first, uint64_t count, uint32_t rev) {
#pragma unroll
    for (int j = 0; j < FOLD_PER_LANE; ++j) {
        const uint64_t e = first + j;
        if (e < count) {
            const uint64_t w = WIRE && rev ? count - 1 - e : e;
            fp_load(x[j], a.p + (w & a.mask) * 8);
            if constexpr (WIRE) vec_canon(x[j]);
        } else {
            fp_zero(x[j]);
        }
    }
}

// r = r zp + v
template <class Fr>
BLZ_DEV void horner_step(Fp<Fr>& r, const Fp<Fr>& zp, const Fp<Fr>& v) {
    fp_mul(r, r, zp);
    fp_add(r, r, v);
}

// totals[tile] = sum_j a[tile's j-th position] Z^(1023 - j); count is a multiple of the tile
template <class Fr, bool WIRE>
__global__ __launch_bounds__(VEC_THREADS) void k_horner_up(uint32_t* totals, NttVecArg a, uint64_t count, uint32_t rev,
                                                            const uint32_t* pwg, int base) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    __shared__ __attribute__((aligned(16))) uint32_t pw[HORNER_SLOTS * 8];
    const uint32_t t = threadIdx.x;
    horner_powers<Fr>(pw, nullptr, pwg, base, FOLD_LOG_THREADS);
    E v[FOLD_PER_LANE];
    horner_load<Fr, WIRE>(v, a, (uint64_t)blockIdx.x * NTT_FOLD_TILE + (uint64_t)t * FOLD_PER_LANE, count, rev);
    {
        E z1;
        fp_load(z1, pw);
#pragma unroll
        for (int j = 1; j < FOLD_PER_LANE; ++j) horner_step<Fr>(v[0], z1, v[j]);
    }
    fold_block_tree<Fr>(x, v[0], [&](E& l, const E& r, int lw) {
        E zw;
        fp_load(zw, pw + (1 + lw) * 8);   // the right half spans 4 w positions
        horner_step<Fr>(l, zw, r);
    });
    vec_copy32(totals + (size_t)blockIdx.x * 8, x);
}

// dst[e] = carry[tile] Z^(e - tile's first + 1) + sum_{tile's first <= j <= e} a[j] Z^(e - j) (exclusive: the value of e - 1; the
// carry itself at the tile's first), e < count; carry == nullptr: zero (the single tile of a one-block scan).  total (nullable):
// the inclusive value of position count - 1, canonical.  WIRE && rev: position e is word count - 1 - e of a and of dst.
// dst may be a.p.
template <class Fr, bool WIRE>
__global__ __launch_bounds__(VEC_THREADS) void k_horner_down(uint32_t* dst, NttVecArg a, const uint32_t* carry, uint64_t count,
                                                              uint32_t flags, uint32_t* total, const uint32_t* z, const uint32_t* pwg,
                                                              int base) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t x[VEC_THREADS * 8];
    __shared__ __attribute__((aligned(16))) uint32_t pw[HORNER_SLOTS * 8];
    const uint32_t t = threadIdx.x;
    const uint32_t rev = flags & HORNER_REVERSE, exclusive = flags & HORNER_EXCLUSIVE;
    const uint64_t tile0 = (uint64_t)blockIdx.x * NTT_FOLD_TILE;
    const uint64_t first = tile0 + (uint64_t)t * FOLD_PER_LANE;
    // the lanes that hold elements, and the Kogge-Stone steps that reach across them (block-uniform)
    const uint32_t held = count - tile0 < NTT_FOLD_TILE ? (uint32_t)(count - tile0) : (uint32_t)NTT_FOLD_TILE;
    const uint32_t lanes = (held + FOLD_PER_LANE - 1) / FOLD_PER_LANE;
    int ks = 0;
    while ((1u << ks) < lanes) ++ks;
    horner_powers<Fr>(pw, z, pwg, base, ks);
    E v[FOLD_PER_LANE];
    horner_load<Fr, WIRE>(v, a, first, count, rev);
    E z1, s = v[0];
    fp_load(z1, pw);
#pragma unroll
    for (int j = 1; j < FOLD_PER_LANE; ++j) horner_step<Fr>(s, z1, v[j]);
    // the carry-in is a virtual element ahead of lane 0: four positions below the lane's last.  A carry means full tiles: ks = 8
    E below;
    fp_zero(below);
    if (carry && t == 0) {
        E z4, c;
        fp_load(below, carry + (size_t)blockIdx.x * 8);
        fp_load(z4, pw + 8);
        fp_mul(c, below, z4);
        fp_add(s, s, c);
    }
    // Kogge-Stone over the lanes' values: after step k, x[t] is the inclusive value at lane t's last position over the lanes
    // t - 2^(k + 1) + 1 .. t
    fp_store(x + t * 8, s);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < ks; ++k) {
        const uint32_t d = 1u << k;
        E o, zd;
        if (t >= d) fp_load(o, x + (t - d) * 8); else fp_zero(o);
        fp_load(zd, pw + (1 + k) * 8);
        __syncthreads();
        fp_mul(o, o, zd);
        fp_add(s, o, s);
        fp_store(x + t * 8, s);
        __syncthreads();
    }
    if (t > 0) fp_load(below, x + (t - 1) * 8);
    // the recurrence from the value before the lane's first element
#pragma unroll
    for (int j = 0; j < FOLD_PER_LANE; ++j) {
        const uint64_t e = first + j;
        E inc = below;
        horner_step<Fr>(inc, z1, v[j]);
        if (e < count) {
            E out = exclusive ? below : inc;
            if constexpr (WIRE) fp_reduce(out);
            fp_store(dst + (WIRE && rev ? count - 1 - e : e) * 8, out);
            if (total && e == count - 1) {
                fp_reduce(inc);
                fp_store(total, inc);
            }
        }
        below = inc;
    }
}

template <class Fr>
int ntt_vec_horner_t(hipStream_t st, uint32_t flags, uint32_t* dst, NttVecArg a, NttVecArg z, uint64_t n, uint32_t* total, uint32_t* ws) {
    const dim3 thr(VEC_THREADS);
    const ScanPlan p = scan_plan(n, ws);
    const uint32_t* const pw = p.free;   // z^(2^i), i < logn, behind the levels; none for a single tile, which squares its own
    if (pw) hipLaunchKernelGGL((k_horner_pow<Fr>), dim3(1), dim3(64), 0, st, p.free, z.p, fold_log2(n));
    // level l runs on Z = z^(2^(10 l)); above the wire: forward, exclusive, no total
    scan_ladder(
        p, dst, a, n,
        [&](auto wire, const ScanLevel& l, uint32_t* totals) {
            hipLaunchKernelGGL((k_horner_up<Fr, decltype(wire)::value>), l.grid(), thr, 0, st, totals, l.src, l.count,
                               l.level ? 0u : flags & HORNER_REVERSE, pw, l.level * HORNER_LOG_TILE);
        },
        [&](auto wire, const ScanLevel& l, const uint32_t* carry) {
            hipLaunchKernelGGL((k_horner_down<Fr, decltype(wire)::value>), l.grid(), thr, 0, st, l.dst, l.src, carry, l.count,
                               l.level ? (uint32_t)HORNER_EXCLUSIVE : flags, l.level ? nullptr : total, z.p, pw, l.level * HORNER_LOG_TILE);
        });
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
