// Poseidon kernels over one scalar field (included by poseidon_<field>.hip; the hash itself is stated in
// include/blaze_hip.h, the design in DESIGN.md section 8).
//
// ONE LANE PER STATE ELEMENT.  A hash of width t lives on t adjacent lanes of a wave (64 / t hashes per wave: 5 at t = 12,
// 7 at t = 9), each lane holding one element in the reduced radix (9 x 29 bits, Montgomery form).  A round is
//   lane e:  y = state[e] + c[round][e];  S-box y^5 (all lanes in a full round, lane 0 only in a partial one);  y -> LDS;
//            state[e] = sum_j M[e][j] y_j,  the y_j read back from LDS (a broadcast inside the hash's lanes), row e of M from the
//            matrix's LDS image
// so a lane never holds more than one element plus the operands of the dot product it is in: the kernel stays far below the
// register count that would leave a SIMD with one wave (one lane per hash needs 2 x 108 registers for the state alone).
// The row product is rr_mul2 generalised: up to SIX products a_i b_i share one Montgomery reduction (the 64-bit column
// bound (sum F_a F_b + 1) 9 + 1 <= 64 admits six normalised operands pairs), so a t = 12 row costs 12 x 81 + 2 x 81 multiply-adds
// instead of 12 x 162.  Every range is in the types, as in field_rr.hip.hpp.
#pragma once
#include "ntt_rr.hip.hpp"   // rr_canon
#include "poseidon_engine.hpp"

namespace blz {

// r = (sum_i a_i b_i) / Rrr under ONE reduction
template <class Q, int K, class A, class B, int... Is>
BLZ_DEV void rr_dot_col(uint64_t& acc, const A& a, const B& b, std::integer_sequence<int, Is...>) {
    (BLZ_RR_AB<Q::NL, K>(acc, a[Is].v, b[Is].v), ...);
}
template <class Q, int N, int Fa, int Va, int Fb, int Vb>
BLZ_DEV void rr_dot(Frr<Q, 1, 2>& r, const Frr<Q, Fa, Va> (&a)[N], const Frr<Q, Fb, Vb> (&b)[N]) {
    static_assert(rr_cols_ok<Q>(N * Fa * Fb), "column sum would overflow 64 bits: fewer products per reduction");
    static_assert(rr_vals_ok<Q>(N * Va * Vb), "sum of products would leave the lazy value range");
    rr_columns<Q>(r, [&](auto k, uint64_t& acc) { rr_dot_col<Q, decltype(k)::value>(acc, a, b, std::make_integer_sequence<int, N>{}); },
                  std::make_integer_sequence<int, 2 * Q::NL - 1>{});
}

constexpr int POS_DOT = 6;   // products per reduction (the column bound above)
constexpr int pos_reductions(int t) { return (t + POS_DOT - 1) / POS_DOT; }

template <class Q, int F, int V>
BLZ_DEV void pos_lds_load(Frr<Q, F, V>& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < Q::NL; ++i) r.v[i] = p[i];
}

// products [C0, C0 + N) of a row: M[e][C0 + i] y_(C0 + i)
template <class Q, int C0, int N, class Y>
BLZ_DEV void pos_row_part(Frr<Q, 1, 2>& r, const uint32_t* mrow, const uint32_t* ys) {
    Frr<Q, 1, 1> m[N];
    Y y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pos_lds_load(m[i], mrow + (C0 + i) * POS_SD);
        pos_lds_load(y[i], ys + (C0 + i) * POS_SD);
    }
    rr_dot<Q>(r, y, m);
}

// canonical 32-byte words -> x Rrr mod r, canonical, POS_SD dwords apart (the tables of PoseidonWidth)
template <class Q>
__global__ __launch_bounds__(64) void k_poseidon_prep(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    uint32_t w[Q::N32];
#pragma unroll
    for (int k = 0; k < Q::N32; ++k) w[k] = words[(size_t)i * Q::N32 + k];
    Frr<Q, 1, 2> x;
    rr_to_mont_from_words<Q>(x, w);
    const Frr<Q, 1, 1> c = rr_canon(x);
    uint32_t* o = out + (size_t)i * POS_SD;
#pragma unroll
    for (int k = 0; k < POS_SD; ++k) o[k] = k < Q::NL ? c.v[k] : 0u;
}

template <class Q, int T>
__global__ __launch_bounds__(64) void k_poseidon_hash(PoseidonWidth w, PoseidonJob job) {
    constexpr int HW = 64 / T;                 // hashes per wave
    constexpr int NR = pos_reductions(T);      // reductions per matrix row
    static_assert(T >= POS_T_MIN && T <= POS_T_MAX && NR <= 3, "width out of range");
    using State = Frr<Q, NR, 2 * NR>;          // a row's NR reduced parts, summed
    using Elem = Frr<Q, 1, 2 * NR + 1>;        // ... plus the round constant, carries propagated: what the S-box and the matrix read
    __shared__ __attribute__((aligned(16))) uint32_t s_m[T * T * POS_SD];
    __shared__ __attribute__((aligned(16))) uint32_t s_y[HW * T * POS_SD];
    const uint32_t lane = threadIdx.x;
    const uint32_t hsh = lane / T, e = lane - hsh * T;
    const bool active = hsh < (uint32_t)HW;    // (64 - HW T lanes of a wave have no hash)
    const uint32_t hs = active ? hsh : 0u;
    const uint64_t j = (uint64_t)blockIdx.x * HW + hsh;
    const bool live = active && j < job.n;

    for (uint32_t i = lane; i < (uint32_t)(T * T * POS_SD / 4); i += 64u)
        reinterpret_cast<uint4*>(s_m)[i] = reinterpret_cast<const uint4*>(w.mds)[i];

    Frr<Q, 1, 2> x0;
    if (e == 0u || !live) {
        Frr<Q, 1, 1> tag;
        rr_load(tag, w.tag);
        x0 = rr_as<1, 2>(tag);
    } else {
        const uint4* p = reinterpret_cast<const uint4*>(job.in + (j * (uint64_t)(T - 1) + (e - 1u)) * 8u);
        const uint4 lo = p[0], hi = p[1];
        const uint32_t wd[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        rr_to_mont_from_words<Q>(x0, wd);     // any 256-bit word: taken as its residue
    }
    State x = rr_as<NR, 2 * NR>(x0);

    const int rounds = w.rf + w.rp, half = w.rf / 2;
    const uint32_t* rc = w.rc + e * POS_SD;
    const uint32_t* mrow = s_m + e * (T * POS_SD);
    const uint32_t* ys = s_y + hs * (T * POS_SD);
    uint32_t* ymine = s_y + (hs * T + e) * POS_SD;
    for (int r = 0; r < rounds; ++r, rc += T * POS_SD) {
        Frr<Q, 1, 1> c;
        rr_load(c, rc);
        Elem y = rr_norm(rr_add(x, c));
        const bool full = r < half || r >= half + w.rp;
        if (full || e == 0u) {
            Frr<Q, 1, 2> y2, y4, y5;
            rr_sqr(y2, y);
            rr_sqr(y4, y2);
            rr_mul(y5, y4, y);
            y = rr_as<1, 2 * NR + 1>(y5);
        }
        __syncthreads();   // the round before has read its y
        if (active) {
#pragma unroll
            for (int i = 0; i < Q::NL; ++i) ymine[i] = y.v[i];
        }
        __syncthreads();
        Frr<Q, 1, 2> p0;
        pos_row_part<Q, 0, (T < POS_DOT ? T : POS_DOT), Elem>(p0, mrow, ys);
        if constexpr (NR == 1) {
            x = p0;
        } else if constexpr (NR == 2) {
            Frr<Q, 1, 2> p1;
            pos_row_part<Q, POS_DOT, T - POS_DOT, Elem>(p1, mrow, ys);
            x = rr_add(p0, p1);
        } else {
            Frr<Q, 1, 2> p1, p2;
            pos_row_part<Q, POS_DOT, POS_DOT, Elem>(p1, mrow, ys);
            pos_row_part<Q, 2 * POS_DOT, T - 2 * POS_DOT, Elem>(p2, mrow, ys);
            x = rr_add(rr_add(p0, p1), p2);
        }
    }

    if (live && e == 1u) {   // digest = state[1]
        Frr<Q, 1, 1> one;
#pragma unroll
        for (int i = 0; i < Q::NL; ++i) one.v[i] = i == 0 ? 1u : 0u;
        Frr<Q, 1, 2> d;
        rr_mul(d, rr_norm(x), one);   // x Rrr / Rrr, < 2r
        uint32_t o[Q::N32];
        rr_to_words<Q>(o, rr_canon(d));
        const uint4 lo = make_uint4(o[0], o[1], o[2], o[3]), hi = make_uint4(o[4], o[5], o[6], o[7]);
        uint4* dg = reinterpret_cast<uint4*>(job.dig + j * 8u);
        dg[0] = lo;
        dg[1] = hi;
        if (job.rec) {
            // the record of parse_poseidon_hash_results: digest | 256-bit word with hash_id in bits 0-29, layer_id in bits 30-39
            const uint64_t tagw = ((job.id0 + j) & 0x3fffffffull) | ((uint64_t)(job.layer & 0x3ffu) << 30);
            uint4* rw = reinterpret_cast<uint4*>(job.rec + j * 16u);
            rw[0] = lo;
            rw[1] = hi;
            rw[2] = make_uint4((uint32_t)tagw, (uint32_t)(tagw >> 32), 0u, 0u);
            rw[3] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

template <class Q>
int poseidon_prep_t(hipStream_t st, const uint32_t* d_words, uint32_t* d_out, uint32_t n) {
    if (!n) return BLZ_OK;
    hipLaunchKernelGGL(k_poseidon_prep<Q>, dim3((n + 63u) / 64u), dim3(64), 0, st, d_words, d_out, n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

template <class Q, int T>
int poseidon_launch(hipStream_t st, const PoseidonWidth& w, const PoseidonJob& job) {
    constexpr uint64_t HW = 64 / T;
    const uint64_t blocks = (job.n + HW - 1) / HW;
    if (blocks > 0x7fffffffull) return fail(BLZ_ERR_INVALID_PARAM, "Poseidon job of %llu hashes exceeds one launch", (unsigned long long)job.n);
    hipLaunchKernelGGL((k_poseidon_hash<Q, T>), dim3((unsigned)blocks), dim3(64), 0, st, w, job);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

template <class Q>
int poseidon_hash_t(hipStream_t st, const PoseidonWidth& w, const PoseidonJob& job) {
    if (!job.n) return BLZ_OK;
    switch (w.t) {
#define BLZ_POS_CASE(T) case T: return poseidon_launch<Q, T>(st, w, job);
        BLZ_POS_CASE(2) BLZ_POS_CASE(3) BLZ_POS_CASE(4) BLZ_POS_CASE(5) BLZ_POS_CASE(6) BLZ_POS_CASE(7) BLZ_POS_CASE(8) BLZ_POS_CASE(9)
        BLZ_POS_CASE(10) BLZ_POS_CASE(11) BLZ_POS_CASE(12) BLZ_POS_CASE(13) BLZ_POS_CASE(14) BLZ_POS_CASE(15) BLZ_POS_CASE(16)
#undef BLZ_POS_CASE
    }
    return fail(BLZ_ERR_INVALID_PARAM, "no Poseidon kernel of width %d", w.t);
}

}  // namespace blz

#include "poseidon_hades.hip.hpp"   // the optimised partial rounds: k_hades_derive, k_hades_hash

namespace blz {

template <class Fr>
PoseidonFieldOps make_poseidon_ops() {
    using Q = typename Fr::RR;
    static_assert(Q::NL == 9 && Q::B == 29 && Q::N32 == 8, "the Poseidon kernels are written for 9 x 29-bit limbs");
    PoseidonFieldOps ops{};
    for (int i = 0; i < 8; ++i) ops.modulus[i] = Fr::MOD[i];
    ops.prep = &poseidon_prep_t<Q>;
    ops.hash = &poseidon_hash_t<Q>;
    ops.derive = &hades_derive_t<Fr>;
    ops.hash_plan = &hades_hash_t<Q>;
    return ops;
}

}  // namespace blz
