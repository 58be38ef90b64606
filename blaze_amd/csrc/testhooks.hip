// Element-wise kernels over the device field / group primitives, so tests can compare each of them
// with the CPU oracle (include/blaze_hip.h "test hooks"), and the MSM tail plan of a shape.  Not on the MSM/NTT product path.
#include "common.hpp"
#include "ec_rr.hip.hpp"
#include "ec_row.hip.hpp"
#include "ec_law.hip.hpp"
#include "poseidon_engine.hpp"
#include "poseidon_impl.hip.hpp"   // rr_dot
#include "msm_engine.hpp"
#include "../../include/blaze_hip_aux.h"

namespace blz {

template <class P>
__global__ __launch_bounds__(64) void k_test_field(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Fp<P> x, y, r;
    fp_load(x, a + (size_t)i * P::N);
    fp_load(y, b + (size_t)i * P::N);
    fp_to_mont(x, x);
    fp_to_mont(y, y);
    switch (op) {
        case 0: fp_mul(r, x, y); break;
        case 1: fp_add(r, x, y); break;
        case 2: fp_sub(r, x, y); break;
        case 3: fp_inv(r, x); break;
        case 5:  // x y + (x + y)(x - y), unreduced sums as operands
        case 6:  // x y - (x + y)(x - y)
            if constexpr (P::LAZY) {
                Fp<P> s, d;
                fp_add(s, x, y);
                fp_sub(d, x, y);
                if (op == 5) fp_mul2(r, x, y, s, d);
                else fp_mulsub2(r, x, y, s, d);
            } else {
                fp_zero(r);
            }
            break;
        case 10: case 11: case 12: case 13: case 14: case 15:
            // the reduced-radix twin (field_rr.hip.hpp): product, square, fused sum of products on lazy operands,
            // carry propagation, zero tests; operands go in through the wire-word conversion and come back
            // through the 32-bit Montgomery form, so both conversions are under test as well
            if constexpr (USE_RR<P>) {
                using Q = typename P::RR;
                fp_load(x, a + (size_t)i * P::N);
                fp_load(y, b + (size_t)i * P::N);
                Frr<Q, 1, 2> xr, yr, rr;
                rr_to_mont_from_words<Q>(xr, x.v);
                rr_to_mont_from_words<Q>(yr, y.v);
                if (op == 10) rr_mul(rr, xr, yr);
                else if (op == 11) rr_sqr(rr, xr);
                else if (op == 12) rr_mul2(rr, xr, yr, rr_norm(rr_add(xr, yr)), rr_sub<2>(xr, yr));   // x y + (x + y)(x - y)
                else if (op == 13) rr_mul(rr, rr_norm(rr_sub_twice<2>(rr_sub<2>(xr, yr), yr)), yr);  // (x - 3y) y
                else if (op == 15) {   // x - 3y + 12m brought below 2m by the quotient-digit reduction; then x (x - 3y)
                    const auto t = rr_reduce2m(rr_sub_twice<2>(rr_sub<2>(xr, yr), yr));
                    rr_mul(rr, t, xr);
                }
                else {  // 1 if x == y (exact test behind the cheap filter), else 0; Montgomery one / zero
                    const auto d = rr_sub<2>(xr, yr);
                    const bool eq = rr_maybe_equal(xr, yr) && rr_is_zero(d);
                    if (rr_is_zero(d) != eq) { rr_zero(rr); rr.v[0] = 7; }   // the filter must never hide an equality
                    else if (eq) rr_one(rr);
                    else rr_zero(rr);
                }
                rr_to_mont32_words<Q>(r.v, rr);
            } else {
                fp_zero(r);
            }
            break;
        default: fp_sqr(r, x); break;
    }
    fp_from_mont(r, r);
    fp_store(out + (size_t)i * P::N, r);
}

template <class F>
__global__ __launch_bounds__(64) void k_test_ec(int op, const uint32_t* p, const uint32_t* q, const uint8_t* inf_flags,
                                                uint32_t* out, uint8_t* out_inf, uint32_t n) {
    uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Affine<F> P, Q;
    fp_load(P.x, p + (size_t)i * 2 * F::N);
    fp_load(P.y, p + (size_t)i * 2 * F::N + F::N);
    fp_load(Q.x, q + (size_t)i * 2 * F::N);
    fp_load(Q.y, q + (size_t)i * 2 * F::N + F::N);
    fp_to_mont(P.x, P.x); fp_to_mont(P.y, P.y); fp_to_mont(Q.x, Q.x); fp_to_mont(Q.y, Q.y);
    uint8_t fl = inf_flags[i];
    XYZZ<F> acc, qq;
    if (fl & 1) pt_set_inf(acc); else pt_from_affine(acc, P);
    if (fl & 2) pt_set_inf(qq); else pt_from_affine(qq, Q);
    // de-normalise the accumulator (scale by a non-trivial z) so the projective paths are exercised
    if (!(fl & 1)) {
        Fp<F> z, z2, z3;
        z = P.x; fp_add(z, z, Q.y);
        if (fp_is_zero(z)) fp_one(z);
        fp_sqr(z2, z); fp_mul(z3, z2, z);
        fp_mul(acc.x, acc.x, z2); fp_mul(acc.y, acc.y, z3); acc.zz = z2; acc.zzz = z3;
    }
    switch (op) {
        case 0: if (!(fl & 2)) pt_madd(acc, Q); break;
        case 1: { XYZZ<F> d; pt_dbl(d, acc); acc = d; } break;
        case 2: {
            if (!(fl & 2)) {  // de-normalise q too
                Fp<F> z, z2, z3;
                z = Q.x; fp_add(z, z, P.y);
                if (fp_is_zero(z)) fp_one(z);
                fp_sqr(z2, z); fp_mul(z3, z2, z);
                fp_mul(qq.x, qq.x, z2); fp_mul(qq.y, qq.y, z3); qq.zz = z2; qq.zzz = z3;
            }
            pt_add(acc, qq);
        } break;
        case 4: case 5:   // the reduced-radix mixed add of the bucket accumulation (ec_rr.hip.hpp); 5 subtracts
            if constexpr (USE_RR<F>) {
                if (!(fl & 2)) {
                    using QQ = typename F::RR;
                    XYZZRR<QQ> a;
                    ptrr_from_xyzz32<F>(a, acc);
                    AffineRR<QQ> q;
                    rr_from_mont32_words<QQ>(q.x, Q.x.v);
                    rr_from_mont32_words<QQ>(q.y, Q.y.v);
                    ptrr_madd<QQ, 2>(a, q, op == 5);
                    // a second, cancelling pair keeps the lazy ranges honest: (acc + Q) + Q - Q
                    ptrr_madd<QQ, 2>(a, q, op == 5);
                    ptrr_madd<QQ, 2>(a, q, op != 5);
                    ptrr_to_xyzz32<F>(acc, a);
                }
            } else {
                pt_set_inf(acc);
            }
            break;
        case 8: case 9:   // the full XYZZ add / doubling on the reduced radix (first bucket-reduce level): 8 = P + Q, 9 = 2 P
            if constexpr (USE_RR<F>) {
                using QQ = typename F::RR;
                if (op == 8 && !(fl & 2)) {  // de-normalise q too
                    Fp<F> z, z2, z3;
                    z = Q.x; fp_add(z, z, P.y);
                    if (fp_is_zero(z)) fp_one(z);
                    fp_sqr(z2, z); fp_mul(z3, z2, z);
                    fp_mul(qq.x, qq.x, z2); fp_mul(qq.y, qq.y, z3); qq.zz = z2; qq.zzz = z3;
                }
                XYZZRR<QQ> a, b;
                ptrr_from_xyzz32<F>(a, acc);
                ptrr_from_xyzz32<F>(b, qq);
                if (op == 8) ptrr_add<QQ, 2>(a, b);
                else a = ptrr_dbl_val<QQ, 2>(a);
                ptrr_to_xyzz32<F>(acc, a);
            } else {
                pt_set_inf(acc);
            }
            break;
        case 6: case 7:   // both operands affine (the first addition of a run, ptrr_aadd): 6 = P + Q, 7 = Q - P
            if constexpr (USE_RR<F>) {
                using QQ = typename F::RR;
                AffineRR<QQ> p, q;
                rr_from_mont32_words<QQ>(p.x, P.x.v);
                rr_from_mont32_words<QQ>(p.y, P.y.v);
                rr_from_mont32_words<QQ>(q.x, Q.x.v);
                rr_from_mont32_words<QQ>(q.y, Q.y.v);
                XYZZRR<QQ> a;
                ptrr_set_inf(a);
                if (fl == 0) ptrr_aadd<QQ, 2>(a, p, op == 7, q, false);
                else if (fl == 1) ptrr_madd<QQ, 2>(a, q, false);
                else if (fl == 2) ptrr_madd<QQ, 2>(a, p, op == 7);
                ptrr_to_xyzz32<F>(acc, a);
            } else {
                pt_set_inf(acc);
            }
            break;
        default: if (!(fl & 2)) { fp_neg(Q.y, Q.y); pt_madd(acc, Q); } break;
    }
    Affine<F> r;
    bool fin = pt_to_affine(r, acc);
    Fp<F> x, y;
    if (fin) { fp_from_mont(x, r.x); fp_from_mont(y, r.y); } else { fp_zero(x); fp_zero(y); }
    fp_store(out + (size_t)i * 2 * F::N, x);
    fp_store(out + (size_t)i * 2 * F::N + F::N, y);
    out_inf[i] = fin ? 0 : 1;
}

struct Tmp {
    std::vector<void*> ptrs;
    ~Tmp() { for (void* p : ptrs) (void)hipFree(p); }
    int alloc(void** p, size_t n) {
        BLZ_HIP(hipMalloc(p, n ? n : 16), BLZ_ERR_UNKNOWN);
        ptrs.push_back(*p);
        return BLZ_OK;
    }
};

// ops 20..24: the row-cooperative field arithmetic of ec_row.hip.hpp (a limb per lane, 16 lanes per element, four elements per
// wave).  Operands go in through the lane form's conversions and the results come back through them, so what is compared with
// the oracle is the value.  24 is a self-check of the carry machinery on SYNTHETIC limb patterns (random Montgomery forms
// practically never hold a run of 0xfffffff limbs): limbs drawn from {0, 1, MASK, MASK - 1, 2^28, 2^28 + 3, lazy ...} by the
// input bits, weak normalisation + exact resolve against a serial carry loop; the result is 1 (agree) or 0.
template <class P>
__global__ __launch_bounds__(64) void k_test_row(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    if constexpr (USE_RR<P>) {
        using Q = typename P::RR;
        if constexpr (!RR_TIGHT<Q> && Q::B == 28) {
            __shared__ uint32_t sh[2][4][16];
            const RowCtx<Q> c = row_ctx<Q>();
            // this row's element; the zero test (23) is wave-wide - the tail's rows are replicas - so it takes one element per wave
            const uint32_t e = op == 23 ? blockIdx.x : blockIdx.x * 4u + c.row;
            const uint32_t ee = e < n ? e : n - 1;
            Fp<P> x, y;
            fp_load(x, a + (size_t)ee * P::N);
            fp_load(y, b + (size_t)ee * P::N);
            uint32_t xl = 0, yl = 0;
            if (op == 24) {
                // limb li from 3 bits of the inputs
                const uint32_t bits = (x.v[c.li % P::N] >> (3u * (c.li / P::N))) ^ (y.v[(c.li * 5u) % P::N] >> 7);
                const uint32_t pat[8] = {0u, 1u, Q::MASK, Q::MASK - 1u, 1u << 28, (1u << 28) + 3u, 15u * (1u << 28) + Q::MASK, (7u << 28) + 1u};
                xl = c.li < (uint32_t)Q::NL ? pat[bits & 7u] : 0u;
                if (c.li == (uint32_t)Q::NL - 1u) xl &= 0xffffu;   // the top limb stays small (value bound)
            } else {
                Frr<Q, 1, 2> xr, yr;
                rr_to_mont_from_words<Q>(xr, x.v);
                rr_to_mont_from_words<Q>(yr, y.v);
                if ((threadIdx.x & 15u) == 0u) {
#pragma unroll
                    for (int i = 0; i < Q::NL; ++i) { sh[0][c.row][i] = xr.v[i]; sh[1][c.row][i] = yr.v[i]; }
                    sh[0][c.row][14] = sh[0][c.row][15] = sh[1][c.row][14] = sh[1][c.row][15] = 0u;
                }
                __syncthreads();
                xl = sh[0][c.row][c.li];
                yl = sh[1][c.row][c.li];
                __syncthreads();
            }
            uint32_t r = 0;
            if (op == 20) r = row_mul<Q>(c, xl, yl);
            else if (op == 21) r = row_mul<Q>(c, row_norm<Q>(c, xl + (c.km2 - yl) + 2u * (c.km2 - yl)), yl);   // (x - 3y + 12m) y
            else if (op == 22) {   // (x - y + 32m)(x + y): the 32m constant, a lazy operand on each side (F = 5 and 2: 11 <= 18)
                r = row_mul<Q>(c, xl + (c.km5 - yl), xl + yl);
            } else if (op == 23) {   // 1 if x == y else 0 (Montgomery one / zero), through the filter and the exact test
                const uint32_t d = row_norm<Q>(c, xl + (c.km2 - yl));
                const bool z = row_is_zero<Q>(c, d);
                const bool eq = row_maybe_equal<Q>(c, d) && z;
                r = z != eq ? (c.li == 0u ? 7u : 0u) : eq ? c.one : 0u;
            } else if (op == 24) {
                r = row_resolve<Q>(c, row_norm<Q>(c, xl));
            }
            if (op != 24) r = row_resolve<Q>(c, r);
            sh[0][c.row][c.li] = r;
            sh[1][c.row][c.li] = xl;
            __syncthreads();
            if (c.li == 0u && e < n && (op != 23 || c.row == 0u)) {
                Fp<P> o;
                if (op == 24) {
                    uint64_t carry = 0;
                    bool same = true;
                    for (int i = 0; i < Q::NL; ++i) {
                        const uint64_t t = (uint64_t)sh[1][c.row][i] + carry;
                        const uint32_t want = i + 1 < Q::NL ? (uint32_t)t & Q::MASK : (uint32_t)t;
                        carry = i + 1 < Q::NL ? t >> Q::B : 0;
                        same = same && want == sh[0][c.row][i];
                    }
                    fp_zero(o);
                    o.v[0] = same ? 1u : 0u;
                    fp_store(out + (size_t)e * P::N, o);
                } else {
                    Frr<Q, 1, 2> rr;
#pragma unroll
                    for (int i = 0; i < Q::NL; ++i) rr.v[i] = sh[0][c.row][i];
                    rr_to_mont32_words<Q>(o.v, rr);
                    fp_from_mont(o, o);
                    fp_store(out + (size_t)e * P::N, o);
                }
            }
        }
    }
}

template <class P>
int test_field_t(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
    Tmp tmp;
    size_t bytes = n * P::N * 4;
    void *da, *db, *dout;
    BLZ_TRY(tmp.alloc(&da, bytes)); BLZ_TRY(tmp.alloc(&db, bytes)); BLZ_TRY(tmp.alloc(&dout, bytes));
    BLZ_HIP(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_HIP(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    if (op >= 20 && op <= 24) {
        BLZ_HIP(hipMemset(dout, 0, bytes), BLZ_ERR_UNKNOWN);   // (fields without the row arithmetic answer zero)
        hipLaunchKernelGGL(k_test_row<P>, dim3((unsigned)(op == 23 ? n : (n + 3) / 4)), dim3(64), 0, 0, op, (const uint32_t*)da, (const uint32_t*)db,
                           (uint32_t*)dout, (uint32_t)n);
    } else
        hipLaunchKernelGGL(k_test_field<P>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, (const uint32_t*)da,
                           (const uint32_t*)db, (uint32_t*)dout, (uint32_t)n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}

template <class F>
int test_ec_t(int op, const uint8_t* p, const uint8_t* q, const uint8_t* fl, uint8_t* out, uint8_t* out_inf, size_t n) {
    Tmp tmp;
    size_t bytes = n * 2 * F::N * 4;
    void *dp, *dq, *dfl, *dout, *dinf;
    BLZ_TRY(tmp.alloc(&dp, bytes)); BLZ_TRY(tmp.alloc(&dq, bytes)); BLZ_TRY(tmp.alloc(&dfl, n));
    BLZ_TRY(tmp.alloc(&dout, bytes)); BLZ_TRY(tmp.alloc(&dinf, n));
    BLZ_HIP(hipMemcpy(dp, p, bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_HIP(hipMemcpy(dq, q, bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_HIP(hipMemcpy(dfl, fl, n, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    hipLaunchKernelGGL(k_test_ec<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, (const uint32_t*)dp,
                       (const uint32_t*)dq, (const uint8_t*)dfl, (uint32_t*)dout, (uint8_t*)dinf, (uint32_t)n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    BLZ_HIP(hipMemcpy(out_inf, dinf, n, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}


// ---- Poseidon: the DEFINITION kernel (include/blaze_hip_aux.h).  One lane per state, the dense textbook rounds on the 8 x 32-bit
// Montgomery arithmetic of field.hip.hpp: it shares neither the representation nor the schedule of the product path
// (poseidon_impl.hip.hpp), and is slow on purpose.  Constants arrive as canonical words and are converted by k_test_pos_mont.
template <class P>
__global__ __launch_bounds__(64) void k_test_pos_mont(const uint32_t* words, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Fp<P> x;
    fp_load(x, words + (size_t)i * P::N);
    fp_to_mont(x, x);
    fp_store(out + (size_t)i * P::N, x);
}
// any 256-bit word -> its residue, Montgomery form
template <class P>
BLZ_DEV void pos_def_load(Fp<P>& x, const uint32_t* p) {
    fp_load(x, p);
    for (int k = 0; k < 16; ++k) fp_csub_const<P, P::MOD>(x);   // 2^256 / r < 14 for the three scalar fields
    fp_to_mont(x, x);
}
// consts: tag | t (rf + rp) round constants | t t matrix entries, Montgomery form
template <class P>
BLZ_DEV void pos_def_permute(Fp<P> (&s)[16], const uint32_t* consts, int t, int rf, int rp) {
    const uint32_t* rc = consts + P::N;
    const uint32_t* mds = rc + (size_t)t * (rf + rp) * P::N;
    for (int r = 0; r < rf + rp; ++r) {
        const bool full = r < rf / 2 || r >= rf / 2 + rp;
        for (int i = 0; i < t; ++i) {
            Fp<P> c;
            fp_load(c, rc + ((size_t)r * t + i) * P::N);
            fp_add(s[i], s[i], c);
            if (full || i == 0) {
                Fp<P> x2, x4;
                fp_mul(x2, s[i], s[i]);
                fp_mul(x4, x2, x2);
                fp_mul(s[i], x4, s[i]);
            }
        }
        Fp<P> nw[16];
        for (int i = 0; i < t; ++i) {
            Fp<P> acc;
            fp_zero(acc);
            for (int j = 0; j < t; ++j) {
                Fp<P> m, pr;
                fp_load(m, mds + ((size_t)i * t + j) * P::N);
                fp_mul(pr, m, s[j]);
                fp_add(acc, acc, pr);
            }
            nw[i] = acc;
        }
        for (int i = 0; i < t; ++i) s[i] = nw[i];
    }
}
template <class P>
__global__ __launch_bounds__(64) void k_test_pos_permute(const uint32_t* consts, int t, int rf, int rp, const uint32_t* in, uint32_t* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Fp<P> s[16];
    for (int k = 0; k < t; ++k) pos_def_load(s[k], in + (i * t + k) * P::N);
    pos_def_permute<P>(s, consts, t, rf, rp);
    for (int k = 0; k < t; ++k) {
        Fp<P> o;
        fp_from_mont(o, s[k]);
        fp_store(out + (i * t + k) * P::N, o);
    }
}
// every node of one layer re-hashed from its children and compared with its record (digest, hash_id, layer_id): res[0] += nodes
// looked at, res[1] += nodes that differ.  child: the 32-byte words of the layer's inputs, `cstride` dwords apart (8: the element
// FIFO; 16: the digests inside the records of the layer below).
template <class P>
__global__ __launch_bounds__(64) void k_test_pos_check_layer(const uint32_t* consts, int t, int rf, int rp, const uint32_t* child, uint32_t cstride,
                                                             const uint32_t* rec, uint64_t n, uint32_t layer, unsigned long long* res) {
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Fp<P> s[16];
    fp_load(s[0], consts);   // the tag
    for (int k = 1; k < t; ++k) pos_def_load(s[k], child + (i * (uint64_t)(t - 1) + (k - 1)) * cstride);
    pos_def_permute<P>(s, consts, t, rf, rp);
    Fp<P> o;
    fp_from_mont(o, s[1]);
    const uint32_t* r = rec + i * 16u;
    bool same = true;
    for (int k = 0; k < P::N; ++k) same = same && r[k] == o.v[k];
    const uint64_t tagw = (i & 0x3fffffffull) | ((uint64_t)layer << 30);
    same = same && r[8] == (uint32_t)tagw && r[9] == (uint32_t)(tagw >> 32);
    for (int k = 10; k < 16; ++k) same = same && r[k] == 0u;
    atomicAdd(&res[0], 1ull);
    if (!same) atomicAdd(&res[1], 1ull);
}

// the product path's kernel of width t on n independent inputs (device pointers): what the tree's layers run.  Blocking.
// plan_state != nullptr: through the optimised partial rounds, derived here for width t; *plan_state = HADES_REFUSED and no
// digests when the width does not admit them.
static int poseidon_hash_batch(int device_id, int field, const uint8_t* words, size_t len, int t, const void* d_in, void* d_out, uint64_t n,
                               uint32_t* plan_state = nullptr) {
    const PoseidonFieldOps* ops = poseidon_ops_for(field);
    if (!ops) return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
    if (!words || !d_in || !d_out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (t < POS_T_MIN || t > POS_T_MAX) return fail(BLZ_ERR_INVALID_PARAM, "width %d out of range", t);
    PoseidonStream ps;
    BLZ_TRY(poseidon_parse(field, 1u << t, words, len, ps));
    BLZ_TRY(use_device(device_id));
    DevBuf raw, consts, plan;
    PoseidonWidth w[POS_T_MAX + 1];
    int rc = poseidon_upload(ops, nullptr, ps, words, raw, consts, w);
    HadesPlan pl;
    if (rc == BLZ_OK && plan_state) {
        const PoseidonBlock* blk = nullptr;
        for (const auto& b : ps.blocks)
            if (b.t == t) blk = &b;
        const size_t el = hades_plan_elements(t, blk->rp);
        rc = plan.reserve(el * POS_SD * 4 + 16, true);
        uint32_t* const d_status = plan.as<uint32_t>() + el * POS_SD;
        if (rc == BLZ_OK && hipMemset(d_status, 0, 4) != hipSuccess) rc = fail(BLZ_ERR_UNKNOWN, "hipMemset failed");
        if (rc == BLZ_OK) rc = ops->derive(nullptr, raw.as<uint32_t>() + blk->tag * 8, t, blk->rf, blk->rp, plan.as<uint32_t>(), d_status);
        if (rc == BLZ_OK) rc = sync_stream_bounded(nullptr, "Poseidon round plan derivation");
        if (rc == BLZ_OK && hipMemcpy(plan_state, d_status, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BLZ_ERR_READ, "hipMemcpy failed");
        pl = hades_plan_at(plan.as<uint32_t>(), t, blk->rp);
    }
    if (rc == BLZ_OK && !(plan_state && *plan_state != HADES_OK)) {
        PoseidonJob job;
        job.in = (const uint32_t*)d_in;
        job.dig = (uint32_t*)d_out;
        job.n = n;
        rc = plan_state ? ops->hash_plan(nullptr, w[t], pl, job) : ops->hash(nullptr, w[t], job);
    }
    if (rc == BLZ_OK) rc = sync_stream_bounded(nullptr, "Poseidon hash batch");
    raw.release();
    consts.release();
    plan.release();
    return rc;
}


// the word stream's block of width t (already checked by blz_poseidon_check_words): word indices
struct PosDefBlock { int t = 0, rf = 0, rp = 0; size_t tag = 0, count = 0; };
static bool pos_def_find(const uint8_t* words, size_t len, int t, PosDefBlock& out) {
    auto small = [&](size_t i) { uint32_t v; memcpy(&v, words + 32 * i, 4); return v; };
    const size_t n = len / 32;
    const uint32_t K = small(2);
    size_t pos = 3;
    for (uint32_t k = 0; k < K && pos + 5 <= n; ++k) {
        const uint32_t bt = small(pos), rf = small(pos + 2), rp = small(pos + 3);
        const size_t count = 1 + (size_t)bt * (rf + rp) + (size_t)bt * bt;
        if ((int)bt == t) {
            out.t = t; out.rf = (int)rf; out.rp = (int)rp; out.tag = pos + 4; out.count = count;
            return true;
        }
        pos += 4 + count;
    }
    return false;
}
// the block's constants on the device, Montgomery form (tag | rc | mds)
template <class P>
int pos_def_consts(Tmp& tmp, const uint8_t* words, const PosDefBlock& b, uint32_t** d_consts) {
    void *raw, *mont;
    BLZ_TRY(tmp.alloc(&raw, b.count * 32));
    BLZ_TRY(tmp.alloc(&mont, b.count * 32));
    BLZ_HIP(hipMemcpy(raw, words + b.tag * 32, b.count * 32, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    hipLaunchKernelGGL(k_test_pos_mont<P>, dim3((unsigned)((b.count + 63) / 64)), dim3(64), 0, 0, (const uint32_t*)raw, (uint32_t*)mont, (uint32_t)b.count);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    *d_consts = (uint32_t*)mont;
    return BLZ_OK;
}
template <class P>
int test_pos_permute_t(const uint8_t* words, const PosDefBlock& b, const uint8_t* in, uint8_t* out, uint64_t n) {
    Tmp tmp;
    uint32_t* consts = nullptr;
    BLZ_TRY(pos_def_consts<P>(tmp, words, b, &consts));
    const size_t bytes = (size_t)n * b.t * 32;
    void *din, *dout;
    BLZ_TRY(tmp.alloc(&din, bytes)); BLZ_TRY(tmp.alloc(&dout, bytes));
    BLZ_HIP(hipMemcpy(din, in, bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    hipLaunchKernelGGL(k_test_pos_permute<P>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (const uint32_t*)consts, b.t, b.rf, b.rp,
                       (const uint32_t*)din, (uint32_t*)dout, n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_TRY(sync_stream_bounded(nullptr, "Poseidon definition kernel"));
    BLZ_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}
template <class P>
int test_pos_tree_check_t(const uint8_t* words, size_t len, int tree_mode, uint32_t height, const void* d_input, const void* d_records, uint64_t out[2]) {
    Tmp tmp;
    PosDefBlock b9, b12;
    if (!pos_def_find(words, len, 9, b9) || (tree_mode == BLZ_TREE_C && !pos_def_find(words, len, 12, b12))) return fail(BLZ_ERR_INVALID_PARAM, "width missing");
    uint32_t *c9 = nullptr, *c12 = nullptr;
    BLZ_TRY(pos_def_consts<P>(tmp, words, b9, &c9));
    if (tree_mode == BLZ_TREE_C) BLZ_TRY(pos_def_consts<P>(tmp, words, b12, &c12));
    void* res;
    BLZ_TRY(tmp.alloc(&res, 16));
    BLZ_HIP(hipMemset(res, 0, 16), BLZ_ERR_UNKNOWN);
    const uint32_t* rec = (const uint32_t*)d_records;
    const uint32_t* below = (const uint32_t*)d_input;   // the inputs of the layer being checked
    uint32_t bstride = 8;
    for (uint32_t l = tree_mode == BLZ_TREE_C ? 0u : 1u; l < height; ++l) {
        const uint64_t n = 1ull << (3 * (height - 1 - l));
        const bool base = l == 0;
        const PosDefBlock& b = base ? b12 : b9;
        hipLaunchKernelGGL(k_test_pos_check_layer<P>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (const uint32_t*)(base ? c12 : c9), b.t, b.rf, b.rp,
                           below, bstride, rec, n, l, (unsigned long long*)res);
        BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
        BLZ_TRY(sync_stream_bounded(nullptr, "Poseidon tree check"));   // (layer by layer: each wait stays well inside its deadline)
        below = rec;
        bstride = 16;
        rec += n * 16u;
    }
    unsigned long long r[2];
    BLZ_HIP(hipMemcpy(r, res, 16, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    out[0] = r[0];
    out[1] = r[1];
    return BLZ_OK;
}

// ---- the group laws of the MSM tail (ec_law.hip.hpp), one program per case on raw point images (include/blaze_hip_aux.h
// blz_test_law_op).  The programs reach a law through its policy interface only, so one body serves every law; the additions and
// doublings go through one out-of-line copy each (a lane law's addition is 14 field products: inlined at every step of every
// program the kernel would be a dozen times the size of the product's largest).
template <class L>
struct LaneRROf { static constexpr bool value = false; };
template <class Q, int TAG>
struct LaneRROf<LaneLawRR<Q, TAG>> {
    static constexpr bool value = true;
    using RR = Q;
    static constexpr int tag = TAG;
};
template <class Law>
__device__ __noinline__ void law_add(const Law& law, typename Law::Pt& a, const typename Law::Pt& b) { law.add(a, b); }
template <class Law>
__device__ __noinline__ void law_dbl(const Law& law, typename Law::Pt& a) { law.dbl(a); }
template <class F>
BLZ_DEV void lane_store(uint32_t* base, size_t idx, const XYZZ<F>& p) { store_xyzz(base, idx, p); }
template <class Q>
BLZ_DEV void lane_store(uint32_t* base, size_t idx, const XYZZRR<Q>& p) { ptrr_store(base, idx, p); }

enum { LAW_IDENT = 0, LAW_ADD, LAW_DBL, LAW_RUNSUM, LAW_HORNER, LAW_REUSE, LAW_TREE, LAW_PROGRAMS };
constexpr int LAW_TEST_TAG = 9;   // the lane laws' out-of-line doubling: a copy of this kernel's own (ec_law.hip.hpp TAG)

// A group of Law::LANES lanes per case (TREE: the wave), one wave per block (RowLaw::to_lane holds a block barrier).  Every lane
// of a group runs every step: a surplus group repeats case n - 1 and stores nothing.  The host has checked that the program reads
// points 0 .. k - 1 of its case only and that arg bounds every loop.
template <class Law>
__global__ __launch_bounds__(64) void k_test_law(int program, int exit, uint32_t k, uint32_t arg, const uint32_t* in, uint32_t* out, uint32_t n) {
    using Pt = typename Law::Pt;
    const uint32_t lane = threadIdx.x & 63u, sub = lane % Law::LANES;
    const bool tree = program == LAW_TREE;
    const uint32_t e = tree ? blockIdx.x : blockIdx.x * (64u / Law::LANES) + lane / Law::LANES;
    const size_t p0 = (size_t)(e < n ? e : n - 1u) * k;
    const Law law(sub);
    Pt acc, t;
    law.inf(acc);
    switch (program) {
        case LAW_IDENT:
            law.load(acc, in, p0);
            break;
        case LAW_ADD:
            law.load(acc, in, p0);
            law.load(t, in, p0 + 1);
            law_add(law, acc, t);
            break;
        case LAW_DBL:
            law.load(acc, in, p0);
            law_dbl(law, acc);
            law.settle(acc);
            break;
        case LAW_RUNSUM: {   // reduce_segment's inner loop (acc is its s)
            Pt run;
            law.inf(run);
            for (uint32_t j = 0; j < 4; ++j) {
                law.load(t, in, p0 + j);
                law_add(law, run, t);
                law_add(law, acc, run);
            }
        } break;
        case LAW_HORNER:     // horner_walk's shape
            law.load(acc, in, p0);
            for (uint32_t j = 1; j < 3; ++j) {
                for (uint32_t d = 0; d < arg; ++d) law_dbl(law, acc);
                law.settle(acc);
                law.load(t, in, p0 + j);
                law_add(law, acc, t);
            }
            break;
        case LAW_REUSE:      // a computed sum added to its own copy, then to two more points
            law.load(acc, in, p0);
            law.load(t, in, p0 + 1);
            law_add(law, acc, t);
            t = acc;
            law_add(law, acc, t);
            for (uint32_t j = 2; j < 4; ++j) {
                law.load(t, in, p0 + j);
                law_add(law, acc, t);
            }
            break;
        case LAW_TREE:       // k_combine_buckets_wave's tree: lane i holds point i, infinity from lane arg on
            if constexpr (LaneRROf<Law>::value) {
                if (lane < arg) law.load(acc, in, p0 + lane);
                for (uint32_t r = 1; r < arg; r <<= 1) ptrr_shuffle_round<typename LaneRROf<Law>::RR, LaneRROf<Law>::tag>(acc, lane, r, arg);
            }
            break;
    }
    const bool mine = e < n && (!tree || lane == 0u);
    if (exit == 0) {
        if (mine && law.owner()) law.store(out, e, acc);
    }
    if constexpr (Law::LANES > 1) {
        if (exit == 1) {
            const auto r = law.to_lane(acc);
            if (mine && sub == 0u) lane_store(out, e, r);
        }
    }
    if constexpr (Law::LANES == 64) {
        if (exit == 2 && mine) law.store_strict(out, e, acc);
    }
}

// what a law's point type declares about its memory image: include/blaze_hip_aux.h blz_test_law_layout
struct LawBound { uint32_t vx, vy, vzz, vzzz, limb_max; };
struct LawLayout {
    uint32_t B = 0, NL = 0, stride = 0, e = 0, lanes = 0, closed = 0;
    LawBound in{}, store{}, strict{}, to_lane{};
    bool tree = false;
};
template <class F, uint32_t LANES>
LawLayout layout_32() {
    LawLayout L;
    L.B = 32; L.NL = F::N; L.stride = F::N; L.e = 32 * F::N; L.lanes = LANES;
    // field.hip.hpp: the lazy fields keep values in [0, 2m], a closed range; the others in [0, m)
    L.closed = F::LAZY ? 1 : 0;
    const uint32_t v = F::LAZY ? 2 : 1;
    L.in = L.store = LawBound{v, v, v, v, 0xffffffffu};
    if (LANES > 1) L.to_lane = L.store;
    return L;
}
template <class Q, uint32_t LANES>
LawLayout layout_rr() {
    LawLayout L;
    L.B = Q::B; L.NL = Q::NL; L.stride = rr_stride<Q>(); L.e = Q::B * Q::NL; L.lanes = LANES;
    // XYZZRR<Q>: x Frr<Q, 1, VX>, y Frr<Q, 1, VY>, zz and zzz Frr<Q, 1, 2>; F = 1 is limbs < 2^B
    L.in = L.store = LawBound{(uint32_t)XYZZRR<Q>::VX, (uint32_t)XYZZRR<Q>::VY, 2, 2, Q::MASK};
    if (LANES > 1) L.to_lane = L.store;
    L.tree = LANES == 1;
    return L;
}
// RowLaw has no bound types; from the comments of ec_row.hip.hpp:
//   in      rowpt_load takes the limbs as they are.  The law reads level 0's bucket sums (XYZZRR: x < VX m, y < VY m) and its own
//           sums: "X3 ... (1, 14)" rowpt_add, "(1, 10)" rowpt_dbl; "Y3 = t - W Y + 4m stays the lazy < 6m it is"; products "< 2m with
//           WEAKLY normalised limbs (<= 2^28 ...)".  The wider of the two per coordinate.
//   store   "limbs as they are (weakly normalised)": the same bounds, a loaded point may leave as it came.
//   strict  rowpt_store_strict / rowpt_export: "exact limbs, Y below 2m by a product with R mod m: XYZZRR's bounds".
template <class Q>
LawLayout layout_row() {
    LawLayout L = layout_rr<Q, 64>();
    const uint32_t vx = XYZZRR<Q>::VX > 14 ? XYZZRR<Q>::VX : 14, vy = XYZZRR<Q>::VY > 6 ? XYZZRR<Q>::VY : 6;
    L.in = L.store = LawBound{vx, vy, 2, 2, 1u << Q::B};
    L.strict = L.to_lane = LawBound{(uint32_t)XYZZRR<Q>::VX, 2, 2, 2, Q::MASK};
    return L;
}

struct LawOp {
    int program, exit;
    uint32_t k, arg;
    const uint32_t* in;
    uint32_t* out;
    size_t n;
};
template <class Law>
int test_law_run(const LawLayout& L, const LawOp& op) {
    const bool tree = op.program == LAW_TREE;
    const size_t pd = 4 * (size_t)L.stride * 4, in_bytes = op.n * op.k * pd, out_bytes = op.n * pd;
    Tmp tmp;
    void *din, *dout;
    BLZ_TRY(tmp.alloc(&din, in_bytes)); BLZ_TRY(tmp.alloc(&dout, out_bytes));
    BLZ_HIP(hipMemcpy(din, op.in, in_bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_HIP(hipMemset(dout, 0, out_bytes), BLZ_ERR_UNKNOWN);
    const size_t per_block = tree ? 1 : 64 / Law::LANES;
    hipLaunchKernelGGL(k_test_law<Law>, dim3((unsigned)((op.n + per_block - 1) / per_block)), dim3(64), 0, 0, op.program, op.exit, op.k, op.arg,
                       (const uint32_t*)din, (uint32_t*)dout, (uint32_t)op.n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_TRY(sync_stream_bounded(nullptr, "group law test kernel"));
    BLZ_HIP(hipMemcpy(op.out, dout, out_bytes, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}
// op == nullptr: the layout only
template <class Law>
int test_law_do(const LawLayout& L, LawLayout* layout, const LawOp* op) {
    if (layout) *layout = L;
    return op ? test_law_run<Law>(L, *op) : BLZ_OK;
}
// the laws the product instantiates for a field (msm_impl.hip.hpp HAS_RR / HAS_ROW; tests/msm_tail_ref.py LAWS)
template <class F>
int test_law_field(int law, LawLayout* layout, const LawOp* op) {
    if constexpr (USE_RR<F>) {
        using Q = typename F::RR;
        if (law == 0) return test_law_do<LaneLawRR<Q, LAW_TEST_TAG>>(layout_rr<Q, 1>(), layout, op);
        if (law == 1) return test_law_do<QuadLawRR<Q>>(layout_rr<Q, 4>(), layout, op);
        if constexpr (!RR_TIGHT<Q>) {
            if (law == 2) return test_law_do<RowLaw<Q>>(layout_row<Q>(), layout, op);
        }
    } else {
        if (law == 0) return test_law_do<LaneLaw32<F, LAW_TEST_TAG>>(layout_32<F, 1>(), layout, op);
        if (law == 1) return test_law_do<QuadLaw32<F>>(layout_32<F, 4>(), layout, op);
    }
    return fail(BLZ_ERR_INVALID_PARAM, "the field has no law %d", law);
}
struct Fq_BN254_W32 : Fq_BN254 {   // BN254 on 32-bit limbs (msm_bn254w.hip): repr 1
    using RR = void;
};
static int test_law_dispatch(int curve, int repr, int law, LawLayout* layout, const LawOp* op) {
    if (repr == 0) {
        switch (curve) {
            case BLZ_BLS377: return test_law_field<Fq_BLS377>(law, layout, op);
            case BLZ_BLS381: return test_law_field<Fq_BLS381>(law, layout, op);
            case BLZ_BN254: return test_law_field<Fq_BN254>(law, layout, op);
        }
    } else if (repr == 1 && curve == BLZ_BN254) {
        return test_law_field<Fq_BN254_W32>(law, layout, op);
    }
    return fail(BLZ_ERR_INVALID_PARAM, "no group laws for curve %d with arithmetic %d", curve, repr);
}

// ---- the reduced-radix primitives one by one, operands at the top of what their types admit (include/blaze_hip_aux.h
// blz_test_rr_op).  A VARIANT is one instantiation of one primitive: its operand and result types are the whole description - the
// layout reads (F, V) off them with rr_bounds, and a variant whose types a static_assert refuses does not compile, so the lists
// below hold only what the code admits.  Images go in and out limb for limb.
enum { RR_MUL = 0, RR_SQR, RR_MUL2, RR_PAIR, RR_DOT, RR_SHOUP, RR_SHOUP_U, RR_SHOUP_QUOT, RR_NORM, RR_REDUCE2M, RR_SUB, RR_SUB_TWICE, RR_NEG,
       RR_CNEG, RR_BFLY, RR_CANON, RR_ZERO, RR_WORDS, RR_DFT8 };

// images that are no Frr: flags (dword j = flag j), N32 raw 32-bit words, normalised limbs of any integer below Rrr
struct RrFlags {};
template <class Q> struct RrWords {};
template <class Q> struct RrRaw {};
template <> struct rr_bounds<RrFlags> { static constexpr int f = 0, v = 0; };
template <class Q> struct rr_bounds<RrWords<Q>> { static constexpr int f = 0, v = 1; };
template <class Q> struct rr_bounds<RrRaw<Q>> { static constexpr int f = 1, v = 0; };

template <class... T> struct TL { static constexpr int n = sizeof...(T); };
template <class... L> struct Cat { using type = TL<>; };
template <class... A> struct Cat<TL<A...>> { using type = TL<A...>; };
template <class... A, class... B, class... R> struct Cat<TL<A...>, TL<B...>, R...> : Cat<TL<A..., B...>, R...> {};
template <class... L> using cat_t = typename Cat<L...>::type;
template <int N, class T> struct Rep { using type = cat_t<TL<T>, typename Rep<N - 1, T>::type>; };
template <class T> struct Rep<0, T> { using type = TL<>; };
template <bool C, class T> using only_if = std::conditional_t<C, TL<T>, TL<>>;   // (naming T does not instantiate it)
template <class O> struct OctTypes;
template <class... T> struct OctTypes<RROct<T...>> { using type = TL<T...>; };

template <class T>
BLZ_DEV T rr_img(const uint32_t* in, int k) {
    constexpr int NL = sizeof(T) / 4;
    T r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.v[i] = in[k * NL + i];
    return r;
}
template <class T>
BLZ_DEV void rr_put(uint32_t* out, int k, const T& a) {
    constexpr int NL = sizeof(T) / 4;
#pragma unroll
    for (int i = 0; i < NL; ++i) out[k * NL + i] = a.v[i];
}
template <int NL, int N>
BLZ_DEV void rr_put_words(uint32_t* out, int k, const uint32_t (&w)[N]) {
#pragma unroll
    for (int i = 0; i < NL; ++i) out[k * NL + i] = i < N ? w[i] : 0u;
}

// the widest bounds the static_asserts of field_rr.hip.hpp admit for a field
template <class Q>
struct RrLim {
    static constexpr int H = rr_head<Q>(), VMAX = 1 << H, FMAX = (1 << (32 - Q::B)) - 1;   // Frr's own limits
    static constexpr int fs() { int f = 1; while (rr_cols_ok<Q>(f + 1)) ++f; return f; }
    static constexpr int FS = fs();                        // the largest sum of F products a column admits
    static constexpr int F1 = FS < FMAX ? FS : FMAX;       // the largest F against a normalised operand
    static constexpr int isqrt(int x) { int r = 1; while ((r + 1) * (r + 1) <= x) ++r; return r; }
    static constexpr int FBA = isqrt(FS), FBB = FS / FBA;  // the most balanced pair
    static constexpr int VBA = 1 << (H / 2), VBB = 1 << (H - H / 2);
    static constexpr int FSQ = 2 * isqrt(FS) <= FMAX ? isqrt(FS) : FMAX / 2;
    static constexpr int FM2 = isqrt(FS - 1);              // a b + c d balanced: FM2^2 + 1 (FS - FM2^2)
    static constexpr int FM2A = FS - 1 < FMAX ? FS - 1 : FMAX;   // ... and one-sided: FM2A 1 + (FS - FM2A) 1
    static constexpr int VHA = 1 << ((H - 1) / 2), VHB = 1 << (H - 1 - (H - 1) / 2);
    static constexpr bool r2m_ok(unsigned long long v) {
        return 4ull * (v + 1) <= Q::MOD[Q::NL - 1] && (v + 1) * (Q::MOD[Q::NL - 1] + 1ull) <= (1ull << 30);
    }
    static constexpr int r2m_v() { int v = 1; while (v < VMAX && r2m_ok(v + 1)) ++v; return v; }
    static constexpr int VR2M = r2m_v();                   // the largest V rr_reduce2m's two static_asserts admit
    static constexpr int VIN1 = 1 << (32 * Q::N32 + 1 - Q::BITS);   // a wire word as the first NTT pass reads it (ntt_rr.hip.hpp)
};

template <class Q, int VAR, int Fa, int Va, int Fb, int Vb>
struct RrvMul {
    using RQ = Q;
    static constexpr int op = RR_MUL, var = VAR, param = 0;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using In = TL<A, Bt>;
    using Out = TL<Frr<Q, 1, 2>, Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        const A a = rr_img<A>(in, 0);
        const Bt b = rr_img<Bt>(in, 1);
        Frr<Q, 1, 2> r, s;
        rr_mul(r, a, b);
        rr_mul_ref(s, a, b);
        rr_put(out, 0, r);
        rr_put(out, 1, s);
    }
};
template <class Q, int VAR, int Fa, int Va>
struct RrvSqr {
    using RQ = Q;
    static constexpr int op = RR_SQR, var = VAR, param = 0;
    using A = Frr<Q, Fa, Va>;
    using In = TL<A>;
    using Out = TL<Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        Frr<Q, 1, 2> r;
        rr_sqr(r, rr_img<A>(in, 0));
        rr_put(out, 0, r);
    }
};
template <class Q, int VAR, int Fa, int Va, int Fb, int Vb, int Fc, int Vc, int Fd, int Vd>
struct RrvMul2 {
    using RQ = Q;
    static constexpr int op = RR_MUL2, var = VAR, param = 0;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using Ct = Frr<Q, Fc, Vc>;
    using Dt = Frr<Q, Fd, Vd>;
    using In = TL<A, Bt, Ct, Dt>;
    using Out = TL<Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        Frr<Q, 1, 2> r;
        rr_mul2(r, rr_img<A>(in, 0), rr_img<Bt>(in, 1), rr_img<Ct>(in, 2), rr_img<Dt>(in, 3));
        rr_put(out, 0, r);
    }
};
template <class Q, int VAR, int Fa, int Va, int Fb, int Vb, int Fc, int Vc, int Fd, int Vd>
struct RrvMulPair {
    using RQ = Q;
    static constexpr int op = RR_PAIR, var = VAR, param = 0;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using Ct = Frr<Q, Fc, Vc>;
    using Dt = Frr<Q, Fd, Vd>;
    using In = TL<A, Bt, Ct, Dt>;
    using Out = TL<Frr<Q, 1, 2>, Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        Frr<Q, 1, 2> r1, r2;
        rr_mul_pair(r1, rr_img<A>(in, 0), rr_img<Bt>(in, 1), r2, rr_img<Ct>(in, 2), rr_img<Dt>(in, 3));
        rr_put(out, 0, r1);
        rr_put(out, 1, r2);
    }
};
template <class Q, int VAR, int Fa, int Va, int Fb, int Vb>
struct RrvSqrPair {
    using RQ = Q;
    static constexpr int op = RR_PAIR, var = VAR, param = 1;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using In = TL<A, Bt>;
    using Out = TL<Frr<Q, 1, 2>, Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        Frr<Q, 1, 2> r1, r2;
        rr_sqr_pair(r1, rr_img<A>(in, 0), r2, rr_img<Bt>(in, 1));
        rr_put(out, 0, r1);
        rr_put(out, 1, r2);
    }
};
template <class Q, int VAR, int N, int Fa, int Va, int Fb, int Vb>
struct RrvDot {
    using RQ = Q;
    static constexpr int op = RR_DOT, var = VAR, param = N;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using In = cat_t<typename Rep<N, A>::type, typename Rep<N, Bt>::type>;
    using Out = TL<Frr<Q, 1, 2>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        A a[N];
        Bt b[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            a[i] = rr_img<A>(in, i);
            b[i] = rr_img<Bt>(in, N + i);
        }
        Frr<Q, 1, 2> r;
        rr_dot<Q>(r, a, b);
        rr_put(out, 0, r);
    }
};
template <class Q, int VAR, int F, int V, bool U>
struct RrvShoup {
    using RQ = Q;
    static constexpr int op = U ? RR_SHOUP_U : RR_SHOUP, var = VAR, param = 0;
    using X = Frr<Q, F, V>;
    using In = TL<X, Frr<Q, 1, 1>>;
    using Out = TL<Frr<Q, 1, 2>, Frr<Q, 1, 1>, RrRaw<Q>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        const X x = rr_img<X>(in, 0);
        RRShoup<Q> t;
        rr_shoup_quot<Q>(t, rr_img<Frr<Q, 1, 1>>(in, 1));
        Frr<Q, 1, 2> r;
        if constexpr (U) {
            RRShoupU<Q> u;
            rr_shoup_uniform<Q>(u, t);
            rr_mul_shoup(r, x, u);
            rr_put_words<Q::NL>(out, 1, u.w);
            rr_put_words<Q::NL>(out, 2, u.wq);
        } else {
            rr_mul_shoup(r, x, t);
            rr_put_words<Q::NL>(out, 1, t.w);
            rr_put_words<Q::NL>(out, 2, t.wq);
        }
        rr_put(out, 0, r);
    }
};
template <class Q, int VAR>
struct RrvShoupQuot {   // VAR 0: from the canonical w; 1: from w Rrr (rr_shoup_from_mont)
    using RQ = Q;
    static constexpr int op = RR_SHOUP_QUOT, var = VAR, param = VAR;
    using W = Frr<Q, 1, VAR == 0 ? 1 : 2>;
    using In = TL<W>;
    using Out = TL<Frr<Q, 1, 1>, RrRaw<Q>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        RRShoup<Q> t;
        if constexpr (VAR == 0) rr_shoup_quot<Q>(t, rr_img<W>(in, 0));
        else rr_shoup_from_mont<Q>(t, rr_img<W>(in, 0));
        rr_put_words<Q::NL>(out, 0, t.w);
        rr_put_words<Q::NL>(out, 1, t.wq);
    }
};
template <class Q, int VAR, int F, int V>
struct RrvNorm {
    using RQ = Q;
    static constexpr int op = RR_NORM, var = VAR, param = 0;
    using A = Frr<Q, F, V>;
    using In = TL<A>;
    using Out = TL<decltype(rr_norm(std::declval<const A&>()))>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) { rr_put(out, 0, rr_norm(rr_img<A>(in, 0))); }
};
template <class Q, int VAR, class A>
struct RrvReduce2m {
    using RQ = Q;
    static constexpr int op = RR_REDUCE2M, var = VAR, param = 0;
    using In = TL<A>;
    using Out = TL<decltype(rr_reduce2m(std::declval<const A&>()))>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) { rr_put(out, 0, rr_reduce2m(rr_img<A>(in, 0))); }
};
// a - b + 2^J m and its kin, b at Vb = 2^(J-1), a at the largest (Fa, Va) whose result type Frr still admits
template <class Q, int J, int OP>
constexpr bool rr_subj_legal() {   // does Frr admit the result's V (Va + 2^J, Va + 2^(J+1), 2^J + 1, 2^J) with Va >= 1?
    return OP == RR_SUB || OP == RR_SUB_TWICE ? RrLim<Q>::VMAX - (OP == RR_SUB_TWICE ? 2 : 1) * (1 << J) >= 1
                                              : (1 << J) + (OP == RR_NEG ? 1 : 0) <= RrLim<Q>::VMAX;
}
template <class Q, int J, int OP>
struct RrvSubJ {
    using RQ = Q;
    using L = RrLim<Q>;
    static constexpr int op = OP, var = J, param = J;
    static constexpr int GROW = OP == RR_SUB_TWICE ? 2 : 1;   // the result is Fa + 2 GROW, Va + GROW 2^J
    using A = Frr<Q, L::FMAX - 2 * GROW, L::VMAX - GROW * (1 << J)>;
    using Bt = Frr<Q, 1, 1 << (J - 1)>;
    static BLZ_DEV auto apply(const uint32_t* in) {
        if constexpr (OP == RR_SUB) return rr_sub<J>(rr_img<A>(in, 0), rr_img<Bt>(in, 1));
        else if constexpr (OP == RR_SUB_TWICE) return rr_sub_twice<J>(rr_img<A>(in, 0), rr_img<Bt>(in, 1));
        else if constexpr (OP == RR_NEG) return rr_neg<J>(rr_img<Bt>(in, 0));
        else return rr_cneg<J>(rr_img<Bt>(in, 0), in[Q::NL] != 0u);
    }
    using In = std::conditional_t<OP == RR_NEG, TL<Bt>, std::conditional_t<OP == RR_CNEG, TL<Bt, RrFlags>, TL<A, Bt>>>;
    using Out = TL<decltype(apply(nullptr))>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) { rr_put(out, 0, apply(in)); }
};
template <class Q, int OP, int... Js>
auto rr_sub_list(std::integer_sequence<int, Js...>) -> cat_t<only_if<rr_subj_legal<Q, Js + 1, OP>(), RrvSubJ<Q, Js + 1, OP>>...>;
template <class Q, int OP>
using rr_sub_list_t = decltype(rr_sub_list<Q, OP>(std::make_integer_sequence<int, Q::NKM>{}));

template <class Q, int VAR, class Tu, class Tv>
struct RrvBfly {
    using RQ = Q;
    using R = decltype(rr_bfly(std::declval<const Tu&>(), std::declval<const Tv&>()));
    static constexpr int op = RR_BFLY, var = VAR;
    static constexpr int param = rr_bounds<Tv>::f < 2 ? 0 : rr_bfly_lazy_fits<Q, rr_bounds<Tu>::f, rr_bounds<Tv>::f>() ? 2 : 1;
    using In = TL<Tu, Tv>;
    using Out = TL<decltype(R::s), decltype(R::d)>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        const auto r = rr_bfly(rr_img<Tu>(in, 0), rr_img<Tv>(in, 1));
        rr_put(out, 0, r.s);
        rr_put(out, 1, r.d);
    }
};
// the operand types of dft8_rr's twelve butterflies, from its own first stage on
template <class Q, int VIN>
struct RrDftTypes {
    using A = Frr<Q, 1, VIN>;
    using P = decltype(rr_bfly(std::declval<const A&>(), std::declval<const A&>()));
    using Ps = decltype(P::s);
    using Pd = decltype(P::d);
    using M = Frr<Q, 1, 2>;                                                                       // a twiddled value
    using Q02 = decltype(rr_bfly(std::declval<const Ps&>(), std::declval<const Ps&>()));
    using Q13 = decltype(rr_bfly(std::declval<const Pd&>(), std::declval<const M&>()));
    using Q02s = decltype(Q02::s);
    using Q02d = decltype(Q02::d);
    using Q13s = decltype(Q13::s);
    using Q13d = decltype(Q13::d);
};
template <class Q, int VAR>
struct RrvCanon {
    using RQ = Q;
    static constexpr int op = RR_CANON, var = VAR, param = 0;
    using A = Frr<Q, 1, 2>;
    using In = TL<A>;
    using Out = TL<decltype(rr_canon(std::declval<const A&>()))>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) { rr_put(out, 0, rr_canon(rr_img<A>(in, 0))); }
};
template <class Q, int VAR, int Fa, int Va, int Fb, int Vb>
struct RrvZero {
    using RQ = Q;
    static constexpr int op = RR_ZERO, var = VAR, param = 0;
    using A = Frr<Q, Fa, Va>;
    using Bt = Frr<Q, Fb, Vb>;
    using In = TL<A, Bt>;
    using Out = TL<RrFlags>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        const A a = rr_img<A>(in, 0);
        const Bt b = rr_img<Bt>(in, 1);
        const uint32_t f[4] = {rr_is_zero(a) ? 1u : 0u, rr_all_zero(a) ? 1u : 0u, rr_maybe_equal(a, b) ? 1u : 0u, rr_is_zero(b) ? 1u : 0u};
        rr_put_words<Q::NL>(out, 0, f);
    }
};
template <class Q, int VAR>
struct RrvWords {   // 0: words in; 1: words out; 2: 32-bit Montgomery words in
    using RQ = Q;
    static constexpr int op = RR_WORDS, var = VAR, param = VAR == 2 ? 3 : 0;   // (rr_from_mont32_words reads its words as < 3m)
    static constexpr int VRAW = 1 << (32 * Q::N32 - Q::BITS + 1);
    using In = std::conditional_t<VAR == 1, TL<Frr<Q, 1, 2>>, TL<RrWords<Q>>>;
    using Out = std::conditional_t<VAR == 0, TL<Frr<Q, 1, VRAW>, Frr<Q, 1, 2>>, std::conditional_t<VAR == 1, TL<RrWords<Q>, RrWords<Q>>, TL<Frr<Q, 1, 2>>>>;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        if constexpr (VAR == 1) {
            const auto a = rr_img<Frr<Q, 1, 2>>(in, 0);
            uint32_t w[Q::N32], w32[Q::N32];
            rr_to_words<Q>(w, a);
            rr_to_mont32_words<Q>(w32, a);
            rr_put_words<Q::NL>(out, 0, w);
            rr_put_words<Q::NL>(out, 1, w32);
        } else {
            uint32_t w[Q::N32];
#pragma unroll
            for (int i = 0; i < Q::N32; ++i) w[i] = in[i];
            Frr<Q, 1, 2> r;
            if constexpr (VAR == 0) {
                Frr<Q, 1, VRAW> x;
                rr_from_words<Q>(x, w);
                rr_to_mont_from_words<Q>(r, w);
                rr_put(out, 0, x);
                rr_put(out, 1, r);
            } else {
                rr_from_mont32_words<Q>(r, w);
                rr_put(out, 0, r);
            }
        }
    }
};
template <class Q, int VAR, int VIN, bool U>
struct RrvDft8 {
    using RQ = Q;
    static constexpr int op = RR_DFT8, var = VAR, param = U ? 0 : 1;
    using A = Frr<Q, 1, VIN>;
    using W = std::conditional_t<U, RRShoupU<Q>, RRShoup<Q>>;
    using O = decltype(dft8_rr<Q>(std::declval<const A (&)[8]>(), std::declval<const W&>(), std::declval<const W&>(), std::declval<const W&>()));
    using In = cat_t<typename Rep<8, A>::type, typename Rep<3, Frr<Q, 1, 1>>::type>;
    using Out = typename OctTypes<O>::type;
    static BLZ_DEV void run(const uint32_t* in, uint32_t* out) {
        A a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = rr_img<A>(in, j);
        RRShoup<Q> t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) rr_shoup_quot<Q>(t[j], rr_img<Frr<Q, 1, 1>>(in, 8 + j));
        if constexpr (U) {
            RRShoupU<Q> u[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) rr_shoup_uniform<Q>(u[j], t[j]);
            auto o = dft8_rr<Q>(a, u[0], u[1], u[2]);
            BLZ_RR_FOR8(o, { rr_put(out, K, X); })
        } else {
            auto o = dft8_rr<Q>(a, t[0], t[1], t[2]);
            BLZ_RR_FOR8(o, { rr_put(out, K, X); })
        }
    }
};

// the variants of a field.  0 ..: the widest bounds; 100 ..: bounds the product uses (ec_rr.hip.hpp's mixed addition in its tight
// and loose budgets, ec_quad.hip.hpp rrq_diff, the butterflies and reductions of dft8_rr, Poseidon's row products)
template <class Q>
struct RrList {
    using L = RrLim<Q>;
    static constexpr bool SH = Q::NL == 9, TIGHT = RR_TIGHT<Q>;   // SH: the constant-operand columns exist (Shoup products)
    static constexpr int VX = XYZZRR<Q>::VX;
    static constexpr bool DFT = SH && !std::is_same_v<Q, Fq_BN254::RR>;   // the scalar fields: BN254's base field (q = 3 mod 4) has no w8
    using D2 = RrDftTypes<Q, 2>;
    using D1 = RrDftTypes<Q, L::VIN1>;
    using Mul = TL<RrvMul<Q, 0, L::F1, L::VMAX, 1, 1>, RrvMul<Q, 1, 1, 1, L::F1, L::VMAX>, RrvMul<Q, 2, L::FBA, L::VBA, L::FBB, L::VBB>,
                   RrvMul<Q, 100, 1, VX, 1, 2>>;
    using Sqr = TL<RrvSqr<Q, 0, L::FSQ, L::VBA>, std::conditional_t<TIGHT, RrvSqr<Q, 100, 1, 6>, RrvSqr<Q, 100, 3, 10>>>;
    using Mul2 = TL<RrvMul2<Q, 0, L::FM2A, L::VMAX / 2, 1, 1, L::FS - L::FM2A, 1, 1, L::VMAX / 2>,
                    RrvMul2<Q, 1, L::FM2, L::VHA, L::FM2, L::VHB, 1, L::VHB, L::FS - L::FM2 * L::FM2, L::VHA>,
                    std::conditional_t<TIGHT, RrvMul2<Q, 100, 3, 6, 1, 6, 2, 4, 1, 2>, RrvMul2<Q, 100, 3, 10, 3, 34, 2, 8, 1, 2>>>;
    using Pair = TL<RrvMulPair<Q, 0, L::F1, L::VMAX, 1, 1, L::FBA, L::VBA, L::FBB, L::VBB>, RrvSqrPair<Q, 1, L::FSQ, L::VBA, 1, 1>,
                    RrvMulPair<Q, 100, 1, 2, 1, 2, 2, 4, 1, 2>,
                    std::conditional_t<TIGHT, RrvSqrPair<Q, 101, 1, 6, 1, 6>, RrvSqrPair<Q, 101, 3, 34, 3, 10>>>;
    template <int... Ns>
    static auto dots(std::integer_sequence<int, Ns...>) -> TL<RrvDot<Q, Ns + 1, Ns + 1, 1, L::VMAX / (Ns + 1), 1, 1>...>;
    // every N the column bound admits (6 at 9 x 29 bits, 17 at 14 x 28); 100 / 101: poseidon_impl's Elem at t > 12, poseidon_hades'
    using Dot = cat_t<decltype(dots(std::make_integer_sequence<int, L::FS>{})),
                      only_if<SH, RrvDot<Q, 100, POS_DOT, 1, 7, 1, 1>>, only_if<SH, RrvDot<Q, 101, POS_DOT, 1, 3, 1, 1>>>;
    using Shoup = std::conditional_t<SH,
        TL<RrvShoup<Q, 0, 1, L::VMAX, false>, RrvShoup<Q, 1, L::F1, L::VMAX, false>, RrvShoup<Q, 100, 3, 6, false>, RrvShoup<Q, 101, 1, L::VIN1, false>,
           RrvShoup<Q, 0, 1, L::VMAX, true>, RrvShoup<Q, 1, L::F1, L::VMAX, true>, RrvShoup<Q, 100, 3, 6, true>, RrvShoup<Q, 101, 1, L::VIN1, true>,
           RrvShoupQuot<Q, 0>, RrvShoupQuot<Q, 1>>,
        TL<>>;
    using Lin = cat_t<TL<RrvNorm<Q, 0, L::FMAX, L::VMAX>, RrvNorm<Q, 100, 2, 4>, RrvReduce2m<Q, 0, Frr<Q, L::FMAX, L::VR2M>>,
                         RrvReduce2m<Q, 100, Frr<Q, 3, 6>>>,
                      only_if<SH, RrvReduce2m<Q, 101, typename D2::Q02s>>, only_if<SH, RrvReduce2m<Q, 102, typename D1::Q02s>>,
                      rr_sub_list_t<Q, RR_SUB>, rr_sub_list_t<Q, RR_SUB_TWICE>, rr_sub_list_t<Q, RR_NEG>, rr_sub_list_t<Q, RR_CNEG>>;
    using Bfly = cat_t<TL<RrvBfly<Q, 0, typename D2::A, typename D2::A>, RrvBfly<Q, 1, typename D2::Pd, typename D2::M>,
                          RrvBfly<Q, 2, typename D2::Ps, typename D2::Ps>, RrvBfly<Q, 3, typename D2::Q02s, typename D2::Q02s>,
                          RrvBfly<Q, 4, typename D2::Q13s, typename D2::M>, RrvBfly<Q, 5, typename D2::Q02d, typename D2::M>,
                          RrvBfly<Q, 6, Frr<Q, 1, 2>, Frr<Q, 2, 4>>>,
                       only_if<SH, RrvBfly<Q, 10, typename D1::A, typename D1::A>>, only_if<SH, RrvBfly<Q, 11, typename D1::Pd, typename D1::M>>,
                       only_if<SH, RrvBfly<Q, 12, typename D1::Ps, typename D1::Ps>>, only_if<SH, RrvBfly<Q, 13, typename D1::Q02s, typename D1::Q02s>>>;
    using Rest = cat_t<TL<RrvCanon<Q, 0>, RrvZero<Q, 0, L::F1, L::VMAX, L::F1, L::VMAX>, RrvZero<Q, 100, 3, 6, 1, 2>, RrvWords<Q, 0>, RrvWords<Q, 1>,
                          RrvWords<Q, 2>>,
                       only_if<DFT, RrvDft8<Q, 0, 2, true>>, only_if<DFT, RrvDft8<Q, 1, L::VIN1, true>>, only_if<DFT, RrvDft8<Q, 2, 2, false>>>;
    using type = cat_t<Mul, Sqr, Mul2, Pair, Dot, Shoup, Lin, Bfly, Rest>;
};

struct RrOp {
    int op, var;
    const uint32_t* in;
    uint32_t* out;
    size_t n;
};
// one lane per case.  Every lane of the last wave runs (the SGPR-uniform forms read the wave's first lane): a surplus lane repeats
// case n - 1 and writes into the padding of `out`, which holds a whole number of waves.
template <class Vt>
__global__ __launch_bounds__(64) void k_test_rr(const uint32_t* in, uint32_t* out, uint32_t n) {
    constexpr uint32_t NL = Vt::RQ::NL;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const uint32_t e = i < n ? i : n - 1u;
    Vt::run(in + (size_t)e * Vt::In::n * NL, out + (size_t)i * Vt::Out::n * NL);
}
template <class Vt>
int rr_run(const RrOp& o) {
    constexpr size_t NL = Vt::RQ::NL;
    const size_t waves = (o.n + 63) / 64, in_bytes = o.n * Vt::In::n * NL * 4, out_bytes = o.n * Vt::Out::n * NL * 4;
    Tmp tmp;
    void *din, *dout;
    BLZ_TRY(tmp.alloc(&din, in_bytes));
    BLZ_TRY(tmp.alloc(&dout, waves * 64 * Vt::Out::n * NL * 4));
    BLZ_HIP(hipMemcpy(din, o.in, in_bytes, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_HIP(hipMemset(dout, 0, waves * 64 * Vt::Out::n * NL * 4), BLZ_ERR_UNKNOWN);
    hipLaunchKernelGGL(k_test_rr<Vt>, dim3((unsigned)waves), dim3(64), 0, 0, (const uint32_t*)din, (uint32_t*)dout, (uint32_t)o.n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_TRY(sync_stream_bounded(nullptr, "reduced-radix primitive test kernel"));
    BLZ_HIP(hipMemcpy(o.out, dout, out_bytes, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}
template <class... T>
void rr_emit_bounds(std::vector<uint32_t>& w, TL<T...>) {
    ((w.push_back((uint32_t)rr_bounds<T>::f), w.push_back((uint32_t)rr_bounds<T>::v)), ...);
}
template <class Vt>
void rr_emit(std::vector<uint32_t>& w) {
    const uint32_t head[5] = {(uint32_t)Vt::op, (uint32_t)Vt::var, (uint32_t)Vt::In::n, (uint32_t)Vt::Out::n, (uint32_t)Vt::param};
    w.insert(w.end(), head, head + 5);
    rr_emit_bounds(w, typename Vt::In{});
    rr_emit_bounds(w, typename Vt::Out{});
}
// lay: the records of every variant; o: run the one variant (op, var)
template <class... Vs>
int rr_each(TL<Vs...>, std::vector<uint32_t>* lay, const RrOp* o) {
    int rc = -1;
    ([&] {
        if (lay) rr_emit<Vs>(*lay);
        if (o && Vs::op == o->op && Vs::var == o->var) rc = rr_run<Vs>(*o);
    }(), ...);
    if (!o) return BLZ_OK;
    return rc == -1 ? fail(BLZ_ERR_INVALID_PARAM, "the field has no variant %d of reduced-radix op %d", o->var, o->op) : rc;
}
template <class Q>
int test_rr_field(uint32_t* layout, const RrOp* o) {
    using L = RrLim<Q>;
    std::vector<uint32_t> rec;
    BLZ_TRY(rr_each(typename RrList<Q>::type{}, layout ? &rec : nullptr, o));
    if (layout) {
        constexpr size_t R0 = 16 + Q::NL;
        if (R0 + rec.size() > BLZ_RR_LAYOUT_WORDS) return fail(BLZ_ERR_UNKNOWN, "the layout needs %zu words", R0 + rec.size());
        memset(layout, 0, BLZ_RR_LAYOUT_WORDS * sizeof(uint32_t));
        const uint32_t head[11] = {(uint32_t)Q::B, (uint32_t)Q::NL, (uint32_t)L::H, (uint32_t)Q::NKM, (uint32_t)L::FS, (uint32_t)(Q::B * Q::NL),
                                   (uint32_t)Q::N32, (uint32_t)POS_DOT, Q::T2M, (uint32_t)RrList<Q>::type::n, (uint32_t)(R0 + rec.size())};
        memcpy(layout, head, sizeof(head));
        for (int i = 0; i < Q::NL; ++i) layout[16 + i] = Q::MOD[i];
        memcpy(layout + R0, rec.data(), rec.size() * sizeof(uint32_t));
    }
    return BLZ_OK;
}
static int test_rr_dispatch(int curve, int field, uint32_t* layout, const RrOp* o) {
    if (field == 0 || field == 1) {
        switch (curve) {
            case BLZ_BLS377: return field ? test_rr_field<Fr_BLS377::RR>(layout, o) : test_rr_field<Fq_BLS377::RR>(layout, o);
            case BLZ_BLS381: return field ? test_rr_field<Fr_BLS381::RR>(layout, o) : test_rr_field<Fq_BLS381::RR>(layout, o);
            case BLZ_BN254: return field ? test_rr_field<Fr_BN254::RR>(layout, o) : test_rr_field<Fq_BN254::RR>(layout, o);
        }
    }
    return fail(BLZ_ERR_INVALID_PARAM, "no reduced-radix field %d of curve %d", field, curve);
}

}  // namespace blz

using namespace blz;

extern "C" {

int blz_test_field_op(int device_id, int curve, int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
    BLZ_TRY(use_device(device_id));
    if (n == 0) return BLZ_OK;
    if (field == 0) {
        switch (curve) {
            case BLZ_BLS377: return test_field_t<Fq_BLS377>(op, a, b, out, n);
            case BLZ_BLS381: return test_field_t<Fq_BLS381>(op, a, b, out, n);
            case BLZ_BN254: return test_field_t<Fq_BN254>(op, a, b, out, n);
        }
    } else {
        switch (curve) {
            case BLZ_BLS377: return test_field_t<Fr_BLS377>(op, a, b, out, n);
            case BLZ_BLS381: return test_field_t<Fr_BLS381>(op, a, b, out, n);
            case BLZ_BN254: return test_field_t<Fr_BN254>(op, a, b, out, n);
        }
    }
    return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d", curve);
}

int blz_test_ec_op(int device_id, int curve, int op, const uint8_t* p, const uint8_t* q, const uint8_t* inf_flags,
                   uint8_t* out, uint8_t* out_inf, size_t n) {
    BLZ_TRY(use_device(device_id));
    if (n == 0) return BLZ_OK;
    switch (curve) {
        case BLZ_BLS377: return test_ec_t<Fq_BLS377>(op, p, q, inf_flags, out, out_inf, n);
        case BLZ_BLS381: return test_ec_t<Fq_BLS381>(op, p, q, inf_flags, out, out_inf, n);
        case BLZ_BN254: return test_ec_t<Fq_BN254>(op, p, q, inf_flags, out, out_inf, n);
    }
    return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d", curve);
}

int blz_test_poseidon_permute(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* states_in, uint8_t* states_out, size_t n) {
    if (!words || !states_in || !states_out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (t < 2 || t > 16) return fail(BLZ_ERR_INVALID_PARAM, "width %d out of range", t);
    PoseidonStream checked;   // (the load-time checks; the block itself is looked up by this file's own reader)
    BLZ_TRY(poseidon_parse(field, 1u << t, words, len, checked));
    PosDefBlock b;
    if (!pos_def_find(words, len, t, b)) return fail(BLZ_ERR_INVALID_PARAM, "the stream has no block of width %d", t);
    BLZ_TRY(use_device(device_id));
    if (n == 0) return BLZ_OK;
    switch (field) {
        case BLZ_BLS377: return test_pos_permute_t<Fr_BLS377>(words, b, states_in, states_out, n);
        case BLZ_BLS381: return test_pos_permute_t<Fr_BLS381>(words, b, states_in, states_out, n);
        case BLZ_BN254: return test_pos_permute_t<Fr_BN254>(words, b, states_in, states_out, n);
    }
    return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
}

int blz_test_poseidon_hash(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* inputs, uint8_t* digests, size_t n) {
    if (!words || !inputs || !digests) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (t < 2 || t > 16) return fail(BLZ_ERR_INVALID_PARAM, "width %d out of range", t);
    BLZ_TRY(use_device(device_id));
    if (n == 0) return BLZ_OK;
    Tmp tmp;
    void *din, *dout;
    BLZ_TRY(tmp.alloc(&din, n * (size_t)(t - 1) * 32)); BLZ_TRY(tmp.alloc(&dout, n * 32));
    BLZ_HIP(hipMemcpy(din, inputs, n * (size_t)(t - 1) * 32, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_TRY(poseidon_hash_batch(device_id, field, words, len, t, din, dout, n));
    BLZ_HIP(hipMemcpy(digests, dout, n * 32, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}

int blz_test_poseidon_hash_plan(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* inputs, uint8_t* digests, size_t n,
                                uint32_t* state) {
    if (!words || !inputs || !digests || !state) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (t < 2 || t > 16) return fail(BLZ_ERR_INVALID_PARAM, "width %d out of range", t);
    BLZ_TRY(use_device(device_id));
    *state = 0;
    Tmp tmp;
    void *din, *dout;
    BLZ_TRY(tmp.alloc(&din, (n ? n : 1) * (size_t)(t - 1) * 32)); BLZ_TRY(tmp.alloc(&dout, (n ? n : 1) * 32));
    BLZ_HIP(hipMemcpy(din, inputs, n * (size_t)(t - 1) * 32, hipMemcpyHostToDevice), BLZ_ERR_WRITE);
    BLZ_TRY(poseidon_hash_batch(device_id, field, words, len, t, din, dout, n, state));
    if (*state == HADES_OK) BLZ_HIP(hipMemcpy(digests, dout, n * 32, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    return BLZ_OK;
}

int blz_test_poseidon_tree_check(int device_id, int field, const uint8_t* words, size_t len, int tree_mode, uint32_t tree_height, const void* d_input,
                                 const void* d_records, uint64_t out[2]) {
    if (!words || !d_input || !d_records || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (tree_height < 1 || tree_height > 11) return fail(BLZ_ERR_INVALID_PARAM, "tree height out of range");
    BLZ_TRY(blz_poseidon_check_words(field, tree_mode, words, len, nullptr));
    BLZ_TRY(use_device(device_id));
    switch (field) {
        case BLZ_BLS377: return test_pos_tree_check_t<Fr_BLS377>(words, len, tree_mode, tree_height, d_input, d_records, out);
        case BLZ_BLS381: return test_pos_tree_check_t<Fr_BLS381>(words, len, tree_mode, tree_height, d_input, d_records, out);
        case BLZ_BN254: return test_pos_tree_check_t<Fr_BN254>(words, len, tree_mode, tree_height, d_input, d_records, out);
    }
    return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
}

int blz_test_msm_tail_plan(int curve, int repr, uint32_t npts, int sbits, int pieces, int table_c, int bit_lo, int bit_hi, uint32_t plan_out[8],
                           uint8_t* widths, char* text, size_t cap) {
    if (!plan_out || !text || cap == 0) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    const MsmCurveOps* ops = msm_ops_for(curve, repr);
    if (!ops || npts == 0) return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d or empty task", curve);
    // the steps of MsmEngine::begin()
    MsmPlan P;
    BLZ_TRY(msm_task_plan(curve, npts, sbits, table_c, bit_lo, bit_hi, P, nullptr));
    uint32_t per = 0;
    pieces = msm_task_pieces(P, pieces, false, &per);
    TailPlan T;
    BLZ_TRY(plan_tail(P, ops->tail, pieces > 1, T));
    const uint32_t out[8] = {(uint32_t)P.c, (uint32_t)P.W, (uint32_t)P.G, P.L, P.Bw, (uint32_t)P.Wv, (uint32_t)P.ebits, P.table ? 1u : 0u};
    memcpy(plan_out, out, sizeof(out));
    if (widths) memcpy(widths, P.width, (size_t)P.W);
    const std::string line = describe(T);
    if (line.size() >= cap) return fail(BLZ_ERR_INVALID_PARAM, "text buffer of %zu bytes for a line of %zu", cap, line.size());
    memcpy(text, line.c_str(), line.size() + 1);
    return BLZ_OK;
}

int blz_test_msm_sort_plan(int curve, int repr, uint32_t npts, int sbits, int pieces, int table_c, int bit_lo, int bit_hi, int hide_env, int other_busy,
                           int recent_hot, int fits, char* text, size_t cap) {
    if (!text || cap == 0) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (!msm_ops_for(curve, repr) || npts == 0) return fail(BLZ_ERR_INVALID_PARAM, "unknown curve %d or empty task", curve);
    // the steps of MsmEngine::begin()
    MsmPlan P;
    BLZ_TRY(msm_task_plan(curve, npts, sbits, table_c, bit_lo, bit_hi, P, nullptr));
    uint32_t per = 0;
    pieces = msm_task_pieces(P, pieces, false, &per);
    const std::string line = describe(plan_sort(P, npts, sbits, pieces, SortInputs{hide_env, other_busy != 0, recent_hot != 0, fits != 0}));
    if (line.size() >= cap) return fail(BLZ_ERR_INVALID_PARAM, "text buffer of %zu bytes for a line of %zu", cap, line.size());
    memcpy(text, line.c_str(), line.size() + 1);
    return BLZ_OK;
}

int blz_test_law_layout(int curve, int repr, int law, uint32_t out[32]) {
    if (!out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    LawLayout L;
    BLZ_TRY(test_law_dispatch(curve, repr, law, &L, nullptr));
    memset(out, 0, 32 * sizeof(uint32_t));
    const uint32_t head[6] = {L.B, L.NL, L.stride, L.e, L.lanes, L.closed};
    memcpy(out, head, sizeof(head));
    const LawBound* b[4] = {&L.in, &L.store, &L.strict, &L.to_lane};
    for (int i = 0; i < 4; ++i) memcpy(out + 6 + 5 * i, b[i], sizeof(LawBound));
    out[26] = L.tree ? 1u : 0u;
    return BLZ_OK;
}

int blz_test_law_op(int device_id, int curve, int repr, int law, int program, int exit, uint32_t k, uint32_t arg, const uint32_t* in, uint32_t* out,
                    size_t n) {
    if (!in || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    LawLayout L;
    BLZ_TRY(test_law_dispatch(curve, repr, law, &L, nullptr));
    // every index and loop bound of the kernel is decided here
    if (program < 0 || program >= LAW_PROGRAMS) return fail(BLZ_ERR_INVALID_PARAM, "unknown program %d", program);
    if (program == LAW_TREE) {
        if (!L.tree) return fail(BLZ_ERR_INVALID_PARAM, "the shuffle tree runs on the reduced-radix lane law only");
        if (k < 1 || k > 64 || arg < 1 || arg > k) return fail(BLZ_ERR_INVALID_PARAM, "tree of %u lanes over %u points", arg, k);
    } else {
        if (k != 4) return fail(BLZ_ERR_INVALID_PARAM, "program %d takes 4 points per case, not %u", program, k);
        if (arg > 64) return fail(BLZ_ERR_INVALID_PARAM, "%u doublings per step (at most 64)", arg);
    }
    const LawBound& ex = exit == 0 ? L.store : exit == 1 ? L.to_lane : L.strict;
    if (exit < 0 || exit > 2 || ex.limb_max == 0) return fail(BLZ_ERR_INVALID_PARAM, "law %d has no exit %d", law, exit);
    if (n == 0) return BLZ_OK;
    if (n > (1u << 20)) return fail(BLZ_ERR_INVALID_PARAM, "%zu cases (at most 2^20)", n);
    BLZ_TRY(use_device(device_id));
    const LawOp op = {program, exit, k, arg, in, out, n};
    return test_law_dispatch(curve, repr, law, nullptr, &op);
}

int blz_test_rr_layout(int curve, int field, uint32_t* out) {
    if (!out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    return test_rr_dispatch(curve, field, out, nullptr);
}

int blz_test_rr_op(int device_id, int curve, int field, int op, int variant, const uint32_t* in, uint32_t* out, size_t n) {
    if (!in || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (n == 0 || n > (1u << 20)) return fail(BLZ_ERR_INVALID_PARAM, "%zu cases (1 .. 2^20)", n);
    BLZ_TRY(use_device(device_id));
    const RrOp o = {op, variant, in, out, n};
    return test_rr_dispatch(curve, field, nullptr, &o);
}

int blz_test_sort_fits_beside(int acc_vgprs, int sort_vgprs, int acc_lds, int sort_lds) {
    return msm_sort_fits_beside(acc_vgprs, sort_vgprs, acc_lds, sort_lds) ? 1 : 0;
}

}  // extern "C"
