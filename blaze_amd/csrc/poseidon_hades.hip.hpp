// The optimised partial rounds of the Poseidon permutation (the Hades strategy's sparse matrices; include/blaze_hip.h "ROUNDS",
// DESIGN.md section 8).  Included by poseidon_impl.hip.hpp; two kernels per field:
//   k_hades_derive  one workgroup per width: inverts Mh (M without row 0 and column 0) and writes the sparse matrices, the
//                   transformed constants and the pre-sparse matrix as tables in the format of PoseidonWidth.  On the 8 x 32-bit
//                   Montgomery arithmetic of field.hip.hpp - the host side has no field arithmetic.
//   k_hades_hash    the lane layout of k_poseidon_hash (one lane per state element), the same PoseidonJob contract; its partial
//                   rounds run on those tables.
//
// THE ALGEBRA.  Round = add constants -> S-box -> state <- M state, M = [[m00, v^T], [w, Mh]], P = R_P.  For the partial rounds
// k = 1 .. P put j = P - k + 1 and carry the state as z with state = diag(1, Mh^-(j-1)) z behind round k (a diag(1, A) commutes
// with the partial S-box).  Round k becomes z <- S_k sbox0(z + c'_k) with
//     S_k = [[m00, v^T Mh^-j], [Mh^(j-1) w, I]],   c'_k = diag(1, Mh^j) c_k,
// the full round in front multiplies by diag(1, Mh^P) M, and behind round P the substitution is the identity.
//
// A PARTIAL ROUND ON THE LANES (lane e of a hash holds z_e;  U = row 0 of S_k, K = its column 0 with K_0 = m00):
//     y = z_e + c'_e                                       every lane
//     y^2, y^4                              2 SQR          lane 0's S-box; the other lanes' squares are not used
//     lane 0: s = y^4 y    lane e: p_e = U_e y  1 MUL      ONE product, the first operand chosen per lane
//     s, p_e -> LDS;  q_e = K_e s               1 MUL      lane 0: m00 s,  lane e: (Mh^(j-1) w)_e s
//     lane 0: z_0 = q_0 + sum p_e    lane e: z_e = q_e + y   additions, then one quotient digit (rr_reduce2m, 9 multiply-adds)
// Row 0's t products are spread over the hash's lanes, each under its own reduction (the lanes reduce at the same time: one QM
// for the wave where a shared reduction of six would cost ceil(t / 6)), and only 9 dwords per lane cross the lanes.
#pragma once

namespace blz {

// ---- derivation -----------------------------------------------------------------------------------------------------------
constexpr int HADES_DERIVE_THREADS = 256;   // >= (t - 1) t entries of the largest matrix product below

template <class P>
BLZ_DEV void hd_ld(Fp<P>& x, const uint32_t* s, int i) {
#pragma unroll
    for (int k = 0; k < P::N; ++k) x.v[k] = s[i * P::N + k];
}
template <class P>
BLZ_DEV void hd_st(uint32_t* s, int i, const Fp<P>& x) {
#pragma unroll
    for (int k = 0; k < P::N; ++k) s[i * P::N + k] = x.v[k];
}
// canonical word i of the block -> Montgomery form
template <class P>
BLZ_DEV void hd_word(Fp<P>& x, const uint32_t* words, size_t i) {
    fp_load(x, words + i * P::N);
    fp_to_mont(x, x);
}
// sum_l a[a0 + l as] b[b0 + l bs], l < n  (LDS images)
template <class P>
BLZ_DEV void hd_dot(Fp<P>& acc, const uint32_t* a, int a0, int as, const uint32_t* b, int b0, int bs, int n) {
    fp_zero(acc);
    for (int l = 0; l < n; ++l) {
        Fp<P> x, y, pr;
        hd_ld(x, a, a0 + l * as);
        hd_ld(y, b, b0 + l * bs);
        fp_mul(pr, x, y);
        fp_add(acc, acc, pr);
    }
}
// a^(r - 2)
template <class P>
BLZ_DEV void hd_fermat(Fp<P>& r, const Fp<P>& a) {
    uint32_t ex[P::N], br = 0;
#pragma unroll
    for (int i = 0; i < P::N; ++i) ex[i] = sub_bb(P::MOD[i], i == 0 ? 2u : 0u, br);
    fp_one(r);
#pragma unroll
    for (int i = P::N - 1; i >= 0; --i) {
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            fp_mul(r, r, r);
            if ((ex[i] >> bit) & 1u) fp_mul(r, r, a);
        }
    }
}
// an element of a table: x R32 -> canonical -> x Rrr, canonical, POS_SD dwords
template <class P>
BLZ_DEV void hd_out(uint32_t* o, const Fp<P>& x) {
    using Q = typename P::RR;
    Fp<P> c;
    fp_from_mont(c, x);
    Frr<Q, 1, 2> y;
    rr_to_mont_from_words<Q>(y, c.v);
    const Frr<Q, 1, 1> z = rr_canon(y);
#pragma unroll
    for (int k = 0; k < POS_SD; ++k) o[k] = k < Q::NL ? z.v[k] : 0u;
}

// words: the block's canonical words from its tag on (tag | t (rf + rp) constants | t t matrix entries)
template <class P>
__global__ __launch_bounds__(HADES_DERIVE_THREADS) void k_hades_derive(const uint32_t* __restrict__ words, int t, int rf, int rp,
                                                                       uint32_t* __restrict__ tables, uint32_t* __restrict__ status) {
    constexpr int TM = POS_T_MAX, NM = POS_T_MAX - 1;
    static_assert(HADES_DERIVE_THREADS >= NM * TM, "one thread per entry of diag(1, Mh^P) M");
    __shared__ uint32_t s_m[TM * TM * P::N];    // M
    __shared__ uint32_t s_a[NM * NM * P::N];    // Mh (the elimination's left half in between)
    __shared__ uint32_t s_b[NM * NM * P::N];    // Mh^-1
    __shared__ uint32_t s_pw[NM * NM * P::N];   // Mh^j
    __shared__ uint32_t s_u[NM * P::N];         // v^T Mh^-j
    __shared__ uint32_t s_w[NM * P::N];         // Mh^(j-1) w
    const int tid = threadIdx.x, n = t - 1;
    const int ri = tid / n, ci = tid - ri * n;  // this thread's entry of an n x n matrix (tid < n n)
    const bool entry = tid < n * n;
    const size_t rc0 = 1, mds0 = 1 + (size_t)t * (rf + rp);
    uint32_t* const sp = tables;
    uint32_t* const prc = sp + (size_t)2 * t * rp * POS_SD;
    uint32_t* const pre = prc + (size_t)t * rp * POS_SD;

    for (int i = tid; i < t * t; i += HADES_DERIVE_THREADS) {
        Fp<P> x;
        hd_word(x, words, mds0 + i);
        hd_st(s_m, i, x);
    }
    __syncthreads();
    Fp<P> one, zero;
    fp_one(one);
    fp_zero(zero);
    if (entry) {
        Fp<P> x;
        hd_ld(x, s_m, (ri + 1) * t + ci + 1);
        hd_st(s_a, tid, x);
        hd_st(s_b, tid, ri == ci ? one : zero);
    }
    __syncthreads();
    // Gauss-Jordan on [Mh | I]; every branch on the matrix is uniform (all threads read the same LDS words)
    for (int c = 0; c < n && rp > 0; ++c) {
        int p = -1;
        Fp<P> piv;
        for (int i = c; i < n && p < 0; ++i) {
            hd_ld(piv, s_a, i * n + c);
            if (!fp_is_zero(piv)) p = i;
        }
        if (p < 0) {   // no pivot in this column: Mh is singular, the width does not admit the plan
            if (tid == 0) *status = HADES_REFUSED;
            return;
        }
        Fp<P> inv;
        hd_fermat(inv, piv);
        __syncthreads();
        if (tid < n) {   // rows p and c change places, the new row c times 1 / pivot
            Fp<P> ac, ap, bc, bp;
            hd_ld(ac, s_a, c * n + tid); hd_ld(ap, s_a, p * n + tid);
            hd_ld(bc, s_b, c * n + tid); hd_ld(bp, s_b, p * n + tid);
            if (p != c) { hd_st(s_a, p * n + tid, ac); hd_st(s_b, p * n + tid, bc); }
            fp_mul(ap, ap, inv);
            fp_mul(bp, bp, inv);
            hd_st(s_a, c * n + tid, ap);
            hd_st(s_b, c * n + tid, bp);
        }
        __syncthreads();
        const bool elim = entry && ri != c;
        Fp<P> f, ac, bc, a, b;
        if (elim) {
            hd_ld(f, s_a, ri * n + c);
            hd_ld(ac, s_a, c * n + ci); hd_ld(bc, s_b, c * n + ci);
            hd_ld(a, s_a, tid); hd_ld(b, s_b, tid);
        }
        __syncthreads();   // column c is read before it is cleared
        if (elim) {
            Fp<P> pr;
            fp_mul(pr, f, ac); fp_sub(a, a, pr);
            fp_mul(pr, f, bc); fp_sub(b, b, pr);
            hd_st(s_a, tid, a);
            hd_st(s_b, tid, b);
        }
        __syncthreads();
    }
    // Mh again, Mh^0, v, w
    if (entry) {
        Fp<P> x;
        hd_ld(x, s_m, (ri + 1) * t + ci + 1);
        hd_st(s_a, tid, x);
        hd_st(s_pw, tid, ri == ci ? one : zero);
    }
    if (tid < n) {
        Fp<P> x;
        hd_ld(x, s_m, tid + 1);
        hd_st(s_u, tid, x);
        hd_ld(x, s_m, (tid + 1) * t);
        hd_st(s_w, tid, x);
    }
    __syncthreads();
    Fp<P> m00;
    hd_ld(m00, s_m, 0);
    for (int j = 1; j <= rp; ++j) {
        const int k = rp - j;   // partial round k (from 0)
        uint32_t* const urow = sp + (size_t)(2 * k) * t * POS_SD;
        uint32_t* const kcol = urow + (size_t)t * POS_SD;
        Fp<P> nu, nw, npw;
        if (tid < n) {
            Fp<P> wk;
            hd_ld(wk, s_w, tid);
            hd_out(kcol + (tid + 1) * POS_SD, wk);                   // (Mh^(j-1) w)_e
            hd_dot(nu, s_u, 0, 1, s_b, tid, n, n);                   // v^T Mh^-j
            hd_dot(nw, s_a, tid * n, 1, s_w, 0, 1, n);               // Mh^j w, the next step's
        }
        if (tid == n) {
            hd_out(kcol, m00);
            hd_out(urow, zero);                                      // (slot 0 of the row is not read)
        }
        if (entry) hd_dot(npw, s_pw, ri * n, 1, s_a, ci, n, n);      // Mh^j
        __syncthreads();
        if (tid < n) { hd_st(s_u, tid, nu); hd_st(s_w, tid, nw); }
        if (entry) hd_st(s_pw, tid, npw);
        __syncthreads();
        const size_t c0 = rc0 + (size_t)(rf / 2 + k) * t;            // the round's constants in the stream
        if (tid < n) {
            hd_out(urow + (tid + 1) * POS_SD, nu);
            Fp<P> acc;
            fp_zero(acc);
            for (int l = 0; l < n; ++l) {
                Fp<P> x, y, pr;
                hd_ld(x, s_pw, tid * n + l);
                hd_word(y, words, c0 + 1 + l);
                fp_mul(pr, x, y);
                fp_add(acc, acc, pr);
            }
            hd_out(prc + ((size_t)k * t + tid + 1) * POS_SD, acc);   // (Mh^j c)_e
        }
        if (tid == n) {
            Fp<P> x;
            hd_word(x, words, c0);
            hd_out(prc + (size_t)k * t * POS_SD, x);
        }
    }
    // diag(1, Mh^P) M  (M itself when there is no partial round)
    if (tid < n * t) {
        const int r1 = tid / t, col = tid - r1 * t;
        Fp<P> acc;
        hd_dot(acc, s_pw, r1 * n, 1, s_m, t + col, t, n);
        hd_out(pre + ((size_t)(r1 + 1) * t + col) * POS_SD, acc);
    } else if (tid - n * t < t) {
        Fp<P> x;
        hd_ld(x, s_m, tid - n * t);
        hd_out(pre + (size_t)(tid - n * t) * POS_SD, x);
    }
    if (tid == 0) *status = HADES_OK;
}

// ---- the hash ---------------------------------------------------------------------------------------------------------------
// products per reduction in the FULL rounds of k_hades_hash.  The partial rounds need 74 registers; the operands of a six-product
// group (108) would set the kernel's register count for the 8 of 65 rounds that are full
#ifndef BLZ_HADES_DOT
#define BLZ_HADES_DOT 3
#endif
constexpr int HADES_DOT = BLZ_HADES_DOT;
static_assert(HADES_DOT >= 1 && HADES_DOT <= POS_DOT, "products per reduction: the column bound admits six");
// slots [I, T) of a hash's LDS state summed; the limb bound F < 2^(32 - B) is kept by a carry propagation whenever the next
// addition would leave it (every bound is in the types)
template <class Q, int I, int T, int F, int V>
BLZ_DEV auto hades_sum(const Frr<Q, F, V>& acc, const uint32_t* ys) {
    if constexpr (I >= T) {
        return rr_norm(acc);
    } else {
        Frr<Q, 1, 2> p;
        pos_lds_load(p, ys + I * POS_SD);
        if constexpr (F + 1 >= (1 << (32 - Q::B))) return hades_sum<Q, I + 1, T>(rr_add(rr_norm(acc), p), ys);
        else return hades_sum<Q, I + 1, T>(rr_add(acc, p), ys);
    }
}
// a dense row in groups of HADES_DOT products per reduction, the groups' results added and brought below 2r again
template <class Q, int C0, int T, int F, int V>
BLZ_DEV auto hades_row_groups(const Frr<Q, F, V>& acc, const uint32_t* mrow, const uint32_t* ys) {
    if constexpr (C0 >= T) {
        return acc;
    } else {
        Frr<Q, 1, 2> p;
        pos_row_part<Q, C0, (T - C0 < HADES_DOT ? T - C0 : HADES_DOT), Frr<Q, 1, 2>>(p, mrow, ys);
        return hades_row_groups<Q, C0 + HADES_DOT, T>(rr_add(acc, p), mrow, ys);
    }
}
template <class Q, int T>
BLZ_DEV Frr<Q, 1, 2> hades_row(const uint32_t* mrow, const uint32_t* ys) {
    Frr<Q, 1, 2> p0;
    pos_row_part<Q, 0, (T < HADES_DOT ? T : HADES_DOT), Frr<Q, 1, 2>>(p0, mrow, ys);
    if constexpr (T <= HADES_DOT) return p0;
    else return rr_reduce2m(hades_row_groups<Q, HADES_DOT, T>(p0, mrow, ys));
}
template <class Q, int F, int V>
BLZ_DEV Frr<Q, F, V> rr_select(bool first, const Frr<Q, F, V>& a, const Frr<Q, F, V>& b) {
    Frr<Q, F, V> r;
#pragma unroll
    for (int i = 0; i < Q::NL; ++i) r.v[i] = first ? a.v[i] : b.v[i];
    return r;
}

template <class Q, int T>
__global__ __launch_bounds__(64) void k_hades_hash(PoseidonWidth w, HadesPlan pl, PoseidonJob job) {
    constexpr int HW = 64 / T;                 // hashes per wave
    static_assert(T >= POS_T_MIN && T <= POS_T_MAX, "width out of range");
    using State = Frr<Q, 1, 2>;                // every round leaves the state below 2r
    using Elem = Frr<Q, 1, 3>;                 // state + round constant, carries propagated
    constexpr int VSUM = 2 * (T - 1) > 3 ? 2 * (T - 1) : 3;   // row 0's t - 1 products, or a lane's own y
    __shared__ __attribute__((aligned(16))) uint32_t s_m[T * T * POS_SD];
    __shared__ __attribute__((aligned(16))) uint32_t s_y[HW * T * POS_SD];
    const uint32_t lane = threadIdx.x;
    const uint32_t hsh = lane / T, e = lane - hsh * T;
    const bool active = hsh < (uint32_t)HW;    // (64 - HW T lanes of a wave have no hash)
    const uint32_t hs = active ? hsh : 0u;
    const uint64_t j = (uint64_t)blockIdx.x * HW + hsh;
    const bool live = active && j < job.n;

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
    State x = x0;

    const int half = w.rf / 2;
    const uint32_t* mrow = s_m + e * (T * POS_SD);
    const uint32_t* ys = s_y + hs * (T * POS_SD);
    uint32_t* ymine = s_y + (hs * T + e) * POS_SD;
    const uint32_t eo = e * POS_SD;            // this lane's element inside a row of a table (the row's address stays uniform)
    // four phases: half - 1 full rounds with M, one with the pre-sparse matrix, the partial rounds, half full rounds with M
    for (int ph = 0; ph < 4; ++ph) {
        if (ph != 2) {
            const int r0 = ph == 0 ? 0 : ph == 1 ? half - 1 : half + w.rp;
            const int cnt = ph == 0 ? half - 1 : ph == 1 ? 1 : half;
            const uint4* msrc = reinterpret_cast<const uint4*>(ph == 1 ? pl.pre : w.mds);
            __syncthreads();   // the rounds before have read their matrix
            for (uint32_t i = lane; i < (uint32_t)(T * T * POS_SD / 4); i += 64u) reinterpret_cast<uint4*>(s_m)[i] = msrc[i];
            const uint32_t* rc = w.rc + (size_t)r0 * T * POS_SD;
            for (int r = 0; r < cnt; ++r, rc += T * POS_SD) {
                Frr<Q, 1, 1> c;
                rr_load(c, rc + eo);
                Elem y = rr_norm(rr_add(x, c));
                Frr<Q, 1, 2> y2, y4, y5;
                rr_sqr(y2, y);
                rr_sqr(y4, y2);
                rr_mul(y5, y4, y);
                __syncthreads();   // the round before has read its y
                if (active) {
#pragma unroll
                    for (int i = 0; i < Q::NL; ++i) ymine[i] = y5.v[i];
                }
                __syncthreads();
                x = hades_row<Q, T>(mrow, ys);
            }
        } else {
            const uint32_t* prc = pl.prc;
            const uint32_t* sp = pl.sp;
            for (int r = 0; r < w.rp; ++r, prc += T * POS_SD, sp += 2 * T * POS_SD) {
                Frr<Q, 1, 1> c, u, kc;
                rr_load(c, prc + eo);
                rr_load(u, sp + eo);
                rr_load(kc, sp + T * POS_SD + eo);
                const Elem y = rr_norm(rr_add(x, c));
                Frr<Q, 1, 2> y2, y4, s;
                rr_sqr(y2, y);
                rr_sqr(y4, y2);
                rr_mul(s, rr_select(e == 0u, y4, rr_as<1, 2>(u)), y);   // lane 0: y^5;  lane e: U_e y
                __syncthreads();   // the round before has read its sums
                if (active) {
#pragma unroll
                    for (int i = 0; i < Q::NL; ++i) ymine[i] = s.v[i];
                }
                __syncthreads();
                Frr<Q, 1, 2> s0, q;
                pos_lds_load(s0, ys);
                rr_mul(q, kc, s0);                                      // lane 0: m00 y^5;  lane e: K_e y^5
                Frr<Q, 1, 2> p1;
                pos_lds_load(p1, ys + (T > 1 ? 1 : 0) * POS_SD);
                const Frr<Q, 1, 2 * (T - 1)> rowsum = hades_sum<Q, 2, T>(p1, ys);
                const Frr<Q, 1, VSUM> rest = rr_select(e == 0u, rr_as<1, VSUM>(rowsum), rr_as<1, VSUM>(y));
                x = rr_reduce2m(rr_add(q, rest));
            }
        }
    }

    if (live && e == 1u) {   // digest = state[1]: the record of k_poseidon_hash
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
            const uint64_t tagw = ((job.id0 + j) & 0x3fffffffull) | ((uint64_t)(job.layer & 0x3ffu) << 30);
            uint4* rw = reinterpret_cast<uint4*>(job.rec + j * 16u);
            rw[0] = lo;
            rw[1] = hi;
            rw[2] = make_uint4((uint32_t)tagw, (uint32_t)(tagw >> 32), 0u, 0u);
            rw[3] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

template <class P>
int hades_derive_t(hipStream_t st, const uint32_t* d_block, int t, int rf, int rp, uint32_t* d_tables, uint32_t* d_status) {
    if (t < POS_T_MIN || t > POS_T_MAX) return fail(BLZ_ERR_INVALID_PARAM, "no Poseidon kernel of width %d", t);
    hipLaunchKernelGGL(k_hades_derive<P>, dim3(1), dim3(HADES_DERIVE_THREADS), 0, st, d_block, t, rf, rp, d_tables, d_status);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

template <class Q, int T>
int hades_launch(hipStream_t st, const PoseidonWidth& w, const HadesPlan& pl, const PoseidonJob& job) {
    constexpr uint64_t HW = 64 / T;
    const uint64_t blocks = (job.n + HW - 1) / HW;
    if (blocks > 0x7fffffffull) return fail(BLZ_ERR_INVALID_PARAM, "Poseidon job of %llu hashes exceeds one launch", (unsigned long long)job.n);
    hipLaunchKernelGGL((k_hades_hash<Q, T>), dim3((unsigned)blocks), dim3(64), 0, st, w, pl, job);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

template <class Q>
int hades_hash_t(hipStream_t st, const PoseidonWidth& w, const HadesPlan& pl, const PoseidonJob& job) {
    if (!job.n) return BLZ_OK;
    if (!pl.sp || !pl.prc || !pl.pre) return fail(BLZ_ERR_UNKNOWN, "the optimised rounds of width %d were not derived", w.t);
    switch (w.t) {
#define BLZ_POS_CASE(T) case T: return hades_launch<Q, T>(st, w, pl, job);
        BLZ_POS_CASE(2) BLZ_POS_CASE(3) BLZ_POS_CASE(4) BLZ_POS_CASE(5) BLZ_POS_CASE(6) BLZ_POS_CASE(7) BLZ_POS_CASE(8) BLZ_POS_CASE(9)
        BLZ_POS_CASE(10) BLZ_POS_CASE(11) BLZ_POS_CASE(12) BLZ_POS_CASE(13) BLZ_POS_CASE(14) BLZ_POS_CASE(15) BLZ_POS_CASE(16)
#undef BLZ_POS_CASE
    }
    return fail(BLZ_ERR_INVALID_PARAM, "no Poseidon kernel of width %d", w.t);
}

}  // namespace blz
