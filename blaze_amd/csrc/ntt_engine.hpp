// Host-side interface of the NTT device passes (per-field translation units: ntt_<field>.hip).
#pragma once
#include "common.hpp"

namespace blz {

struct NttTables {  // all Montgomery form, device memory
    uint32_t* wpass[3];  // wpass[p][j] = root_p^j, j < radix_p       (root_p = primitive radix_p-th root)
    uint32_t* t0;        // w^j            j < 512
    uint32_t* t1;        // w^(512 j)      j < 512
    uint32_t* t2;        // w^(2^18 j)     j < 512
    uint32_t* ninv;      // n^-1 (Montgomery) for the inverse transform, else nullptr
    uint32_t* wbase;     // w (Montgomery): the transform's primitive 2^logn-th root - the field generator's (ROOT^(2^(s - logn)))
                         // or the caller's (blz_ntt_new_ex3), inverted for the inverse transform; every table is powers of it
};

// reduced-radix twiddle tables of the 512-point kernel (ntt_rr.hip.hpp): entries of 10 dwords (27-bit limbs), Montgomery
// R_rr, < 2m
struct NttTablesRR {
    // wpass and tA hold SHOUP entries (canonical twiddle | floor(twiddle R_rr / m): 2 x 10 dwords, field_rr.hip.hpp
    // rr_mul_shoup), ts2 too (the step of pass 2's boundary twiddle: a constant); t0 / t1 / t2 / fin stay Montgomery (R_rr)
    uint32_t* wpass[3];
    uint32_t* t0;
    uint32_t* t1;
    uint32_t* t2;
    uint32_t* fin;   // closing factor of the last pass: n^-1 R_rr (inverse) or nullptr (forward: no product)
    uint32_t* tA;    // w^(A e), e < 2^18 (n / 512 entries, 10 MiB), or nullptr: the boundary factor after pass 1 that
                     // does not depend on the column, read instead of stepped (2^27 transforms only; ntt_rr.hip.hpp)
    uint32_t* ts2;   // w^(64 C i0), i0 < 512: the step of pass 2's boundary factor along a lane's rows (one per column); times
                     // s^(64 C) on an inverse coset handle whose pass 2 carries a part of the shift (NttCoset below)
    uint32_t* tB;    // pass 2's boundary factor of EVERY element, w^((C k1 + k2) i0) R_rr mod m (times the part of a coset handle's shift
                     // that pass 2 carries) as 8 words, in the order pass 2 consumes them
                     // (n x 32 bytes: 4 GiB at 2^27), or nullptr: stepped along the lane's rows (ntt_rr.hip.hpp)
    uint32_t swz;    // 0: plain tile order; 1 + s: pass 1 walks its tiles in the channel-spreading order with 2^s adjacent column
                     // groups back to back (2^27 transforms; ntt_rr.hip.hpp)
};
constexpr size_t NTT_RR_BOUNDARY_ENTRIES = (size_t)1 << 18;
constexpr size_t NTT_RR_ENTRY_DWORDS = 10;
constexpr size_t NTT_RR_TABLE_BYTES = (4 * 512 * 2 + 3 * 512 + 1) * NTT_RR_ENTRY_DWORDS * 4;   // 4 Shoup tables (wpass x 3, ts2: 2 entries' worth each), 3 Montgomery, fin
constexpr size_t NTT_RR_BOUNDARY_BYTES = NTT_RR_BOUNDARY_ENTRIES * 2 * NTT_RR_ENTRY_DWORDS * 4;   // tA, Shoup entries

// Tables of a coset handle (blz_ntt_set_coset): powers of s = g (forward) or g^-1 (inverse).  With i = i0 + A i1 + AB i2 and
// k = k2 + C k1 + CB k0 (ntt.hip):
//   forward  X[k] = sum_i x[i] g^i w^(i k): the wire pass multiplies the element as loaded.  Where that pass is the radix-2-in-LDS
//            kernel it takes the whole g^i (d0 d1 d2); where it is the 512-point kernel it takes ONE Shoup entry, tG: g^(i0 + A i1)
//            at 2^18 (pass 2: the whole factor) and g^(A (i1 + B i2)) at 2^27 (pass 1), where the rest, g^i0 - constant along the
//            indices passes 1 and 2 transform over - joins pass 2's boundary factor (its start value, or the table tB);
//   inverse  x[k] = g^-k n^-1 sum_i X[i] w^(-i k): the last pass closes with a product anyway.  The radix-2-in-LDS kernel takes
//            n^-1 s^k there (d0 carries n^-1); the 512-point kernel takes n^-1 s^(CB k0) by output row (finr), and s^(k2 + C k1) -
//            constant along the index pass 3 transforms over - joins pass 2's boundary factor (start value and step ts2, or tB).
struct NttCoset {
    uint32_t *d0, *d1, *d2;   // 32-bit Montgomery: s^e = d0[e & 511] d1[(e >> 9) & 511] d2[e >> 18]  (inverse: d0 carries n^-1)
    uint32_t *u0, *u1, *u2;   // the same three powers (no n^-1) in the reduced radix, Montgomery R_rr
    uint32_t* tG;             // Shoup entries, 2^18: s^(e << gshift), e = (logical index) >> gshift; or nullptr
    uint32_t* finr;           // n^-1 s^(CB k0), k0 < 512, Montgomery R_rr (inverse)
    int gshift;               // 0 at 2^18, logA at 2^27
    int inverse;
    int mode[3];              // per pass: 0 the plain kernel, 1 product on the element as loaded, 2 pass 2 with the folded boundary
                              // factor, 3 the closing product of an inverse transform
};
constexpr size_t NTT_CS_SMALL_BYTES = (size_t)(4 * 512 * 8 + 4 * 512 * NTT_RR_ENTRY_DWORDS + 4 * 8) * 4;   // d0 (x 2: with / without n^-1), d1, d2; u0..u2, finr; the set-up's words (s, the caller's shift, the check's flag)
constexpr size_t NTT_CS_WIRE_BYTES = NTT_RR_BOUNDARY_BYTES;   // tG

struct NttGeom {
    int logA, logB, logC, logn;
    int wire_pass;   // the pass that reads the caller's words (1, 2 or 3): the first one that runs
    int brin, brout; // blz_ntt_new_ex3: the caller's input / output buffers are in bit-reversed order (position p holds the element of
                     // index bitrev(p)): folded into the wire pass's loads / the last pass's stores
};

constexpr int NTT_MAX_LOG = 27;   // the largest log_size a handle accepts (blz_ntt_new*)

// Element-wise ops on resident buffers (blz_ntt_vec_op; kernels: ntt_vec.hip.hpp).  An operand is `mask + 1` (a power of two)
// 32-byte words at p; position e of the op reads word e & mask.
struct NttVecArg {
    const uint32_t* p;
    uint64_t mask;
};
// A caller-defined gate (blz_sum_gate, checked and packed by ntt.hip; kernels: ntt_gate.hip.hpp), by value in the kernel arguments.
// term[m] = nfactors | negate << 3 | deficit << 4 | factor j << (8 + 4 j): deficit = F - nfactors, F the longest term's nfactors;
// close_k = F + (common >= 0), the operands of the longest product: what the finish strips
constexpr int NTT_GATE_MAX_TABLES = 12, NTT_GATE_MAX_TERMS = 8, NTT_GATE_MAX_FACTORS = 4, NTT_GATE_MAX_POINTS = 6;   // BLZ_GATE_MAX_*
struct NttGate {
    uint32_t ntables, nterms;
    int32_t common;   // < 0: none
    uint32_t close_k;
    uint32_t term[NTT_GATE_MAX_TERMS];
    NttVecArg t[NTT_GATE_MAX_TABLES];
};
// The same with linear-form factors (blz_lin_gate, checked and packed by ntt.hip; kernel: ntt_lineval.hip.hpp).  A factor byte
// below NTT_LIN_FORM is a table index, NTT_LIN_FORM | k is form k; common likewise, < 0: none.
//   term_hdr[m] = nfactors | negate << 3, term_fac[m] = factor j << 8 j
//   form_n[k] = nsummands, form[k][s] = table | coef << 8 | negate << 16 (coef NTT_LIN_NO_COEF: 1)
//   coef_tables: bit i is set where table i is the coefficient of a summand of a form that a term or common names
constexpr int NTT_LIN_MAX_TABLES = 16, NTT_LIN_MAX_FORMS = 8, NTT_LIN_MAX_SUMMANDS = 4;   // BLZ_LIN_MAX_*
constexpr uint32_t NTT_LIN_FORM = 0x80, NTT_LIN_NO_COEF = 0xFF;
struct NttLinGate {
    uint32_t ntables, nterms;
    int32_t common;
    uint32_t coef_tables;
    uint32_t term_hdr[NTT_GATE_MAX_TERMS], term_fac[NTT_GATE_MAX_TERMS];
    uint32_t form_n[NTT_LIN_MAX_FORMS];
    uint32_t form[NTT_LIN_MAX_FORMS][NTT_LIN_MAX_SUMMANDS];
    NttVecArg t[NTT_LIN_MAX_TABLES];
};
// One launch of the GKR grand product's own kernels (blz_ntt_gkr_prove; kernels and the layout: ntt_gkr.hip.hpp), by value in the
// kernel arguments.  tree, a: the product tree over 2^m leaves and the leaves; weight: the layer's summed weight (read by a tail
// alone); state, rounds, points, claims: the op's four outputs.  The layers [first, last) are run by ONE block:
//   tail != 0    last == first + 1 and 2^first > 512: the chain of step launches has brought layer `first` down to the live
//                length 512 and left its current row in `rounds`; the block finishes the layer;
//   tail == 0    whole layers, 2^(last - 1) <= 512: nothing of them has run yet;
//   claims_only  no sumcheck: word 0 of the two tables of layer `first` goes to its row of the claims (the chain's own step).
// keep_bits: the challenge keeps bits [0, keep_bits) of a digest
constexpr int GKR_TAIL_LOG = 9;
constexpr uint32_t GKR_TAIL_LEN = 1u << GKR_TAIL_LOG;   // the largest live length the block takes: 2 x 512 + 256 words are 40 KiB of LDS
struct NttGkrTail {
    const uint32_t* tree;
    const uint32_t* a;
    const uint32_t* weight;
    uint32_t *state, *rounds, *points, *claims;
    uint32_t m, first, last, tail, claims_only, keep_bits;
};
// One launch of the fraction GKR's own kernels (blz_ntt_gkr_prove_frac; kernels and the layout: ntt_fgkr.hip.hpp), by value in the
// kernel arguments: NttGkrTail over the numerator and denominator trees and leaves, with the layer challenges beside the four
// outputs.  The layers [first, last) are run by ONE block:
//   tail != 0    last == first + 1 and 2^first > 256: the chain of step launches has written lambda and T = P_hi + lambda Q_hi
//                (over P_hi), brought the layer down to the live length 256 and left its current row in `rounds`;
//   tail == 0    whole layers, 2^(last - 1) <= 256: nothing of them has run yet;
//   claims_only  no sumcheck: word 0 of the four tables of layer `first` (P_hi's from T and lambda) goes to its row of the claims.
constexpr int FGKR_TAIL_LOG = 8;
constexpr uint32_t FGKR_TAIL_LEN = 1u << FGKR_TAIL_LOG;   // the largest live length the block takes: 4 x 256 + 128 words are 36 KiB of LDS
struct NttFgkrTail {
    const uint32_t *tree_p, *tree_q, *a_p, *a_q;
    const uint32_t* weight;
    uint32_t *state, *rounds, *points, *claims, *lambdas;
    uint32_t m, first, last, tail, claims_only, keep_bits;
};
constexpr int NTT_VEC_OPS = 6;              // enum blz_vec_op: ADD SUB MUL MULADD MULSUB INV
constexpr uint64_t NTT_VEC_INV_TILE = 1024;  // batch inversion: elements per block (256 lanes x 4); one 32-byte total per tile
constexpr int NTT_FOLD_OPS = 3;              // enum blz_fold_op: SUM DOT EVAL
constexpr int NTT_SCAN_OPS = 2;              // enum blz_scan_op: SUM PROD
constexpr uint64_t NTT_FOLD_TILE = 1024;     // prefix scans: elements per block (256 lanes x 4 consecutive); one 32-byte total per tile

// per-field entry points.  Field ids follow enum blz_curve: the scalar field Fr of that curve.
struct NttFieldOps {
    int two_adicity;
    // fill the twiddle tables (device memory already carved into T) for a 2^logn transform
    // user_root: device pointer to the caller's root (8 canonical words) or nullptr; *flag (device u32): 1 the root is not a
    // canonical field element, 2 it is not a primitive 2^logn-th root of unity
    int (*setup)(hipStream_t st, NttTables& T, NttTablesRR& TR, const NttGeom& g, int inverse, const uint32_t* user_root, uint32_t* flag);
    // one of the three passes; cols_log is the tile width of the radix-2-in-LDS kernel
    // cs: the coset tables of a handle with a shift in force (its mode[] selects the kernels), or nullptr: the plain transform
    int (*pass)(int pass, hipStream_t st, const void* in, void* out, const NttGeom& g, const NttTables& T, const NttTablesRR& TR,
                int cols_log, bool force_generic, const NttCoset* cs);
    // which pass carries which part of the shift (cs.mode, cs.gshift, cs.inverse); true when the 512-point kernel's wire pass
    // needs tG
    bool (*coset_plan)(const NttGeom& g, int inverse, bool force_generic, NttCoset& cs);
    // the shift (8 words at d_shift) checked (*flag: 1 = not in (0, r)) and turned into s at d_s; nothing else is written
    int (*coset_check)(hipStream_t st, const uint32_t* d_shift, uint32_t* d_s, uint32_t* flag, int inverse);
    // every table of cs from s, and pass 2's folded factors (ts2, tB) where cs.mode says so
    int (*coset_tables)(hipStream_t st, const NttTables& T, const NttTablesRR& TR, const NttGeom& g, const NttCoset& cs, const uint32_t* d_s);
    // ts2 and tB of the plain transform again
    int (*coset_unfold)(hipStream_t st, const NttTables& T, const NttTablesRR& TR, const NttGeom& g);
    // dst[e] = op(a, b, c)[e], e < n (enum blz_vec_op; b / c ignored by the ops that do not take them).  dst may be an operand.
    // totals: ceil(n / NTT_VEC_INV_TILE) x 32 bytes of device memory for the batch inversion's tile totals
    int (*vec_op)(hipStream_t st, int op, uint32_t* dst, NttVecArg a, NttVecArg b, NttVecArg c, uint64_t n, uint32_t* totals);
    // Folds along the buffer (blz_ntt_vec_reduce / blz_ntt_vec_scan; kernels and the workspace's layout: ntt_fold.hip.hpp).
    // ws: n x 32 bytes of device memory nothing else uses while the op runs
    // out (32 bytes) = the fold of a (and b) over e < n (enum blz_fold_op; EVAL: b is the one-word point)
    int (*vec_reduce)(hipStream_t st, int op, uint32_t* out, NttVecArg a, NttVecArg b, uint64_t n, uint32_t* ws);
    // dst[e] = the running fold of a (enum blz_scan_op, flags: BLZ_SCAN_EXCLUSIVE); total (32 bytes, nullable) = the fold of all n.
    // dst may be a.p
    int (*vec_scan)(hipStream_t st, int op, uint32_t flags, uint32_t* dst, NttVecArg a, uint64_t n, uint32_t* total, uint32_t* ws);
    // Weighted scan (blz_ntt_vec_horner; kernels and the workspace's layout: ntt_horner.hip.hpp): dst[p] = a[p] + z dst[p - 1],
    // flags: BLZ_HORNER_EXCLUSIVE | BLZ_HORNER_REVERSE; z: one device word; total (32 bytes, nullable) = the last inclusive value.
    // dst may be a.p
    int (*vec_horner)(hipStream_t st, uint32_t flags, uint32_t* dst, NttVecArg a, NttVecArg z, uint64_t n, uint32_t* total, uint32_t* ws);
    // Gather (blz_ntt_vec_gather; kernels: ntt_gather.hip.hpp): dst[p] = a[(offset + stride p) & a.mask] for p < len, 0 for
    // len <= p < n; a may hold more than n words.  offset <= a.mask, stride reduced modulo a.mask + 1, len <= n.  dst must NOT
    // overlap a's words
    int (*vec_gather)(hipStream_t st, uint32_t* dst, NttVecArg a, uint64_t offset, uint64_t stride, uint64_t len, uint64_t n);
    // Sparse matrix times vector (blz_ntt_vec_spmv; kernels and the workspace's layout: ntt_spmv.hip.hpp): dst[p] = sum over
    // row_ptr[p] <= k < row_ptr[p + 1] of val[k] x[col[k] & x.mask] for p < rows.  row_ptr == nullptr: row p is nonzero p
    // (rows == nnz <= n) and every position of dst is written; else dst holds zeros already, rows >= 1 and nnz >= 1.
    // val == nullptr: coefficients 1.  dst must NOT overlap x's words
    int (*vec_spmv)(hipStream_t st, uint32_t* dst, NttVecArg x, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* val,
                    uint64_t rows, uint64_t nnz, uint64_t n, uint32_t* ws);
    // Scatter-add (blz_ntt_vec_scatter; kernels, the accumulators' layout and the workspace: ntt_scatter.hip.hpp): dst[t] = sum
    // over k < nnz with (idx[k] & (n - 1)) == t of val[k] x[(src ? src[k] : k) & x.mask], 0 where no nonzero points; every
    // position of dst is written.  x.p == nullptr: every x word is 1 (and src is nullptr); val == nullptr: coefficients 1;
    // both: the histogram of idx.  1 <= nnz <= 2^31.  dst must NOT overlap x's words
    int (*vec_scatter)(hipStream_t st, uint32_t* dst, NttVecArg x, const uint32_t* idx, const uint32_t* src, const uint32_t* val,
                       uint64_t nnz, uint64_t n, uint32_t* ws);
    // Multilinear tables (blz_ntt_vec_mle_fold / _eq; kernels and the workspace's layout: ntt_mle.hip.hpp).  len = 2^m, 2 <= len,
    // is the live length; flags: BLZ_MLE_LOW.  None of them writes past the words named here.  blz_ntt_vec_mle_round has no entry
    // of its own: it is sumcheck_step below with BLZ_GATE_PRODUCT, no r and its flags.
    // dst[p] = lo + r (hi - lo), p < len / 2; r: one device word.  dst may be a.p without BLZ_MLE_LOW, and must not overlap a's
    // words otherwise
    int (*vec_mle_fold)(hipStream_t st, uint32_t flags, uint32_t* dst, NttVecArg a, const uint32_t* r, uint64_t len);
    // dst[p] = eq(point, p), p < 2^m; point: m device words (not read when m == 0)
    int (*vec_mle_eq)(hipStream_t st, uint32_t* dst, const uint32_t* point, uint32_t m, uint32_t* ws);
    // A sumcheck step (blz_ntt_sumcheck_step; kernels and the workspace's layout: ntt_sumcheck.hip.hpp) over the gate's k tables
    // t[0 .. k) (BLZ_GATE_PRODUCT: 1 .. 3, BLZ_GATE_R1CS: 4), top-variable pairing.  r (one device word) != nullptr: every table
    // is folded in place - it holds at least len words, no two overlap, len / 2 words of each are written - and out[t], t < points,
    // is the round polynomial of the folded tables (len >= 4); points == 0: the folds alone (len >= 2), out is not looked at.
    // r == nullptr: the round polynomial of the tables as they are (periodic ones allowed), nothing else is written; flags:
    // BLZ_MLE_LOW pairs (2p, 2p + 1), for BLZ_GATE_PRODUCT without r alone
    int (*sumcheck_step)(hipStream_t st, uint32_t gate, uint32_t flags, int k, const NttVecArg* t, const uint32_t* r, uint32_t points,
                         uint64_t len, uint32_t* out, uint32_t* ws);
    // The same step for a caller-defined gate (blz_ntt_sumcheck_gate; kernels: ntt_gate.hip.hpp): g's tables take the place of
    // t[0 .. k) under the same rules, EVERY table of g is folded with r, points <= NTT_GATE_MAX_POINTS
    int (*sumcheck_gate)(hipStream_t st, const NttGate& g, const uint32_t* r, uint32_t points, uint64_t len, uint32_t* out, uint32_t* ws);
    // The same description evaluated position by position (blz_ntt_gate_eval; kernel: ntt_geval.hip.hpp): dst[p] = G over table i
    // read at (p + rot[i]) & g.t[i].mask, p < len; rot: g.ntables values; exactly len words are written.  A table may be dst
    // itself where it starts at dst, holds at least len words and has rot 0; no other table word may lie in dst's len words
    int (*gate_eval)(hipStream_t st, uint32_t* dst, const NttGate& g, const uint64_t* rot, uint64_t len);
    // A gate with linear-form factors evaluated position by position (blz_ntt_gate_eval_lin; kernel: ntt_lineval.hip.hpp):
    // gate_eval's rules over NttLinGate; a table may be dst itself under the same rule whatever names it
    int (*gate_eval_lin)(hipStream_t st, uint32_t* dst, const NttLinGate& g, const uint64_t* rot, uint64_t len);
    // sumcheck_gate's step with a summed weight table beside the gate (blz_ntt_zerocheck_gate; kernel: ntt_zerocheck.hip.hpp):
    // 1 <= points; w: device words.  With r it holds at least len / 2 words clear of every table's first len, and its first
    // len / 4 are written, W[q] += W[q + len / 4]; without r it is read at p & w.mask
    int (*zerocheck_gate)(hipStream_t st, const NttGate& g, NttVecArg w, const uint32_t* r, uint32_t points, uint64_t len, uint32_t* out,
                          uint32_t* ws);
    // Product and fraction trees (blz_ntt_mle_tree; kernels and the layout: ntt_tree.hip.hpp): every layer of the binary tree
    // under the len = 2^m >= 2 words of a (read at p & mask), a layer of s words at word len - 2s of dst, len - 1 words in all.
    // op: enum blz_tree_op; BLZ_TREE_FRAC carries (a, a_q) to (dst, dst_q), BLZ_TREE_PROD ignores both _q; flags: BLZ_MLE_LOW.
    // No destination word may be a word the op reads of a source, nor one of the other destination's
    int (*mle_tree)(hipStream_t st, uint32_t op, uint32_t flags, uint32_t* dst, uint32_t* dst_q, NttVecArg a, NttVecArg a_q, uint64_t len);
    // The small rounds of a GKR grand product in one block (blz_ntt_gkr_prove; kernels: ntt_gkr.hip.hpp): the layers g names, or
    // the claims of one layer.  Nothing of the tree, the leaves or the weight is written
    int (*gkr_tail)(hipStream_t st, const NttGkrTail& g);
    // The same for a fraction tree (blz_ntt_gkr_prove_frac; kernels: ntt_fgkr.hip.hpp): the layers g names over four tables, or the
    // claims of one layer.  Nothing of the trees, the leaves or the weight is written
    int (*fgkr_tail)(hipStream_t st, const NttFgkrTail& g);
};
const NttFieldOps& ntt_ops_bls377();
const NttFieldOps& ntt_ops_bls381();
const NttFieldOps& ntt_ops_bn254();

}  // namespace blz
