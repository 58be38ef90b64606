/* libblaze_hip_aux - test, bench and calibration scaffolding around libblaze_hip (include/blaze_hip.h).
 *
 * NOT part of the product library: synthetic input generators, the multiply-add calibration kernel of bench.py, element-wise
 * test hooks for the device field / group arithmetic, and stall kernels for the bounded-wait tests.  Built as
 * blaze_amd/lib/libblaze_hip_aux.so (links against libblaze_hip.so); loaded by tests/, bench.py and tools/ only.
 * Same conventions as blaze_hip.h (return codes, blz_last_error_message).
 */
#ifndef BLAZE_HIP_AUX_H
#define BLAZE_HIP_AUX_H

#include "blaze_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ synthetic inputs (bench/tests) */

/* scalars: n x 32 B, uniform-ish in [0, r) from a counter-based generator */
int blz_synth_scalars(int device_id, int curve, void* d_out, uint64_t n, uint64_t seed);
/* same stream of values, elements [start, start+n): a shard of a larger synthetic set */
int blz_synth_scalars_at(int device_id, int curve, void* d_out, uint64_t n, uint64_t seed, uint64_t start);
/* points: element i gets pf bases B_{i,j} = 2^(32 j) * (start+i+1) * G, wire format x||y canonical */
int blz_synth_points(int device_id, int curve, void* d_out, uint64_t n, int pf, uint64_t start);
/* NTT input: n x 32 B uniform-ish in [0, r) of BLS12-381 Fr */
int blz_synth_field_elements(int device_id, void* d_out, uint64_t n, uint64_t seed);

/* The issue rate of v_mad_u64_u32 - the instruction the MSM / NTT kernels are bound by - measured on this device at
 * its clocks of this moment: a ~target_ms kernel of independent multiply-add chains on every SIMD.  out[0] lane-ops
 * per second, [1] kernel ms, [2] the device's nominal clock in MHz (hipDeviceAttributeClockRate), [3] ops executed.
 * Measurement aid of bench.py (roofline.integer_issue.peak); no reference counterpart. */
int blz_calib_mad_rate(int device_id, uint32_t target_ms, double out[4]);

/* Test hooks for the bounded waits: enqueue, on the handle's main stream, a one-lane kernel that spins until
 * blz_test_stall_release(token) or until max_ms (1..30000) have passed on the device clock, whichever comes first. */
int blz_test_msm_stall(blz_msm* h, uint32_t max_ms, void** token);
int blz_test_ntt_stall(blz_ntt* h, uint32_t max_ms, void** token);
int blz_test_stall_release(void* token);

/* ------------------------------------------------------------------ test hooks (element-wise kernels)
 * Run the device field / group primitives on arrays so tests can compare them one by one with the
 * CPU oracle.  Host pointers; canonical little-endian encodings.
 *   fq ops (field = 0: Fq, 1: Fr): 0 mul, 1 add, 2 sub, 3 inverse(a), 4 sqr(a), 5/6 a b +- (a + b)(a - b);
 *     reduced-radix twin (every base field and every scalar field has one):
 *     10 mul, 11 sqr, 12 a b + (a + b)(a - b), 13 (a - 3b) b, 14 [a == b], 15 a (a - 3b) through the
 *     product-free reduction of a lazy value
 *   ec ops: 0 P+Q (mixed, P as accumulator), 1 2P, 2 P+Q (full XYZZ add), 3 P-Q (mixed, negated),
 *     4 / 5 P+Q / P-Q through the reduced-radix mixed add; 6 / 7 P+Q / Q-P with both operands affine (the first
 *     addition of a bucket run); 8 P+Q through the reduced-radix full add, 9 2P through its doubling (bucket reduce)
 *     points x||y; inf_flags[i] bit0: P is infinity, bit1: Q is infinity; out_inf[i]=1 if result inf */
int blz_test_field_op(int device_id, int curve, int field, int op, const uint8_t* a, const uint8_t* b,
                      uint8_t* out, size_t n);
int blz_test_ec_op(int device_id, int curve, int op, const uint8_t* p, const uint8_t* q,
                   const uint8_t* inf_flags, uint8_t* out, uint8_t* out_inf, size_t n);

/* The window plan and the tail schedule MsmEngine::begin() gives a task of npts points of sbits-bit scalars (256 / 32 / 64) on `curve`
 * with arithmetic `repr` (0, or 1 = BN254 on 32-bit limbs), asked for in `pieces` pieces, with a window table of width table_c (0: none)
 * and the scalar range [bit_lo, bit_hi) (0, 0: all).  Host only, no device (like blz_msm_plan); BLAZE_MSM_PLAN applies.
 * plan_out = {c, W, G, L, Bw, Wv, ebits, table}; widths (nullable, 96 bytes): the window widths; text: the kernels behind the
 * accumulation as one line, "units<k_combine_units passes> [hot|hot_row] fold_<none|lane|wave|row_strict|row_weak> |
 * L0<w32|rr|quad|row> L<..> ... finish[_row]".  A plan the kernels cannot serve is an error, as it is for the task. */
int blz_test_msm_tail_plan(int curve, int repr, uint32_t npts, int sbits, int pieces, int table_c, int bit_lo, int bit_hi, uint32_t plan_out[8],
                           uint8_t* widths, char* text, size_t cap);
/* The sort stage the same task gets in front of its accumulation (plan_sort()), from what begin() reads besides the plan: hide_env
 * (BLAZE_SORT_HIDE, passed in - the environment is not read), other_busy (the handle's other slot holds a task), recent_hot (one of
 * the last two collected tasks piled its entries into a few buckets), fits (the three-level sort's blocks fit beside the
 * accumulation's), each 0 / 1.  Host only, no device.  text: "lds open" | "tiny open" | "s3 open" | "s3 hidden" | "s3 pingpong". */
int blz_test_msm_sort_plan(int curve, int repr, uint32_t npts, int sbits, int pieces, int table_c, int bit_lo, int bit_hi, int hide_env, int other_busy,
                           int recent_hot, int fits, char* text, size_t cap);

/* The group laws of the MSM tail (ec_law.hip.hpp), element by element on RAW point images: what a law loads and stores, limb for limb.
 * law: 0 lane, 1 quad (a DPP quad per point), 2 row (a wave per point); repr as above.  A (curve, repr, law) the product does not
 * instantiate is BLZ_ERR_INVALID_PARAM (the set: tests/msm_tail_ref.py LAWS).
 * blz_test_law_layout (host only): what the point type and the law declare about an image -
 *   out[0] limb bits B, [1] limbs NL, [2] dwords per coordinate (an image is x | y | zz | zzz, 4 out[2] dwords), [3] the Montgomery
 *   exponent e (R = 2^e), [4] LANES, [5] 1 when the value bounds are closed (value <= V m: the 32-bit lazy range [0, 2m]), 0 when open
 *   (value < V m), then four bounds of five words each - the value factors V of x, y, zz, zzz and the largest limb admitted - at
 *   [6] what the law reads, [11] what store writes, [16] store_strict, [21] to_lane (all zero: the law has no such exit);
 *   [26] 1 when the law has the shuffle tree (program 6).  Limbs are B bits apart whatever their size: a coordinate is
 *   sum limb_i 2^(B i); infinity is zz with every limb zero.
 * blz_test_law_op: n cases of k images each (host pointers, the law's own layout), one result image per case.  Programs (k = 4
 *   except TREE): 0 IDENT P0; 1 ADD P0 + P1; 2 DBL 2 P0; 3 RUNSUM run = s = inf, for j: run += Pj, s += run (the bucket reduce's
 *   inner loop: 4 P0 + 3 P1 + 2 P2 + P3); 4 HORNER acc = P0, arg doublings, += P1, arg doublings, += P2 (arg <= 64);
 *   5 REUSE a = P0 + P1, a += copy of a, a += P2, a += P3; 6 TREE (reduced-radix lane law only, 1 <= arg <= k <= 64): lane i < arg of a
 *   wave holds Pi, the others infinity, then the pairwise shuffle rounds 1, 2, 4 .. < arg; lane 0's sum.
 *   exit: 0 the law's store; 1 to_lane, written by the owner lane in the lane law's layout (cooperative laws); 2 store_strict (row). */
int blz_test_law_layout(int curve, int repr, int law, uint32_t out[32]);
int blz_test_law_op(int device_id, int curve, int repr, int law, int program, int exit, uint32_t k, uint32_t arg, const uint32_t* in,
                    uint32_t* out, size_t n);

/* The reduced-radix primitives (field_rr.hip.hpp; rr_bfly / rr_canon / dft8_rr of ntt_rr.hip.hpp, rr_dot of poseidon_impl.hip.hpp), one
 * by one on RAW limb images with operands at the top of what their TYPES admit: Frr<Q, F, V> is "every limb < F 2^B, integer < V m".
 * field: 0 Fq, 1 Fr of `curve`; all six fields have a reduced-radix twin (BLS12-377 / 381 Fq at 14 x 28 bits, the others 9 x 29).
 * An image is NL dwords, limb i at dword i, the integer sum limb_i 2^(B i) whatever the limbs' size; no conversion on the way.
 * blz_test_rr_layout (host only): out[BLZ_RR_LAYOUT_WORDS] =
 *   [0] B, [1] NL, [2] HEAD (Rrr / 2^BITS = 2^HEAD: value factors V reach 2^HEAD), [3] NKM, [4] the largest fsum rr_cols_ok admits,
 *   [5] the Montgomery exponent B NL, [6] N32 (32-bit words of the wire form), [7] POS_DOT, [8] T2M, [9] the number of records,
 *   [10] the words used, [16 ..) the NL limbs of m, then the records, one per (op, variant) the hook instantiates:
 *     op, variant, k_in, k_out, param, then k_in + k_out pairs (F, V) read off the operand and result types with rr_bounds.
 *     F = 0 is no limb image: V = 0 a flag image (dword j = flag j), V = 1 N32 raw 32-bit words.  F = 1, V = 0: limbs < 2^B, any
 *     integer below Rrr (a Shoup quotient).
 *   Every op is instantiated at the widest bounds its own static_asserts admit for the field (variants 0 ..) and at bounds the product
 *   uses where they differ (variants 100 ..: ec_rr.hip.hpp, ntt_rr.hip.hpp, poseidon_impl / poseidon_hades).
 * blz_test_rr_op: n cases (host pointers) of k_in images each, one lane per case, k_out images per case out, limb for limb as the
 *   primitive left them.  An (op, variant) the field has no record of is BLZ_ERR_INVALID_PARAM.  Ops (in -> out; param):
 *    0 MUL        a, b -> rr_mul, rr_mul_ref
 *    1 SQR        a -> rr_sqr
 *    2 MUL2       a, b, c, d -> rr_mul2 (a b + c d)
 *    3 PAIR       variant 0 / 100: a1, b1, a2, b2 -> rr_mul_pair; variant 1 / 101: a1, a2 -> rr_sqr_pair (param 1)
 *    4 DOT        a_0 .. a_N-1, b_0 .. b_N-1 -> rr_dot; param N
 *    5 SHOUP      x, w (canonical, plain) -> rr_mul_shoup(x, entry), entry.w, entry.wq; the entry made by rr_shoup_quot.  9 limbs only
 *    6 SHOUP_U    the same through the SGPR-uniform entry: every lane of a wave (64 consecutive cases) multiplies by the w of the
 *                 wave's FIRST case, and returns that entry
 *    7 SHOUP_QUOT variant 0: w -> rr_shoup_quot's w, wq; variant 1 (param 1): w Rrr (< 2m) -> rr_shoup_from_mont's w, wq
 *    8 NORM       a -> rr_norm
 *    9 REDUCE2M   a -> rr_reduce2m
 *   10 SUB        a, b -> rr_sub<J>;   11 SUB_TWICE a, b -> rr_sub_twice<J>;   12 NEG b -> rr_neg<J>;
 *   13 CNEG       b, flag image (dword 0: sign) -> rr_cneg<J> (a literal zero stays zero).  variant = param = J, 1 .. NKM where the
 *                 result type exists (rr_neg's is Frr<Q, 2, 2^J + 1>: 2^J m - 0 is 2^J m)
 *   14 BFLY       u, v -> rr_bfly's sum, difference; param 0 normalised v, 1 lazy v carry-propagated first, 2 lazy v against (Fv + 1)
 *                 times the borrow form.  The difference is u - v + (V_d - V_u) m.
 *   15 CANON      a -> rr_canon
 *   16 ZERO       a, b -> flag image: rr_is_zero(a), rr_all_zero(a), rr_maybe_equal(a, b), rr_is_zero(b)
 *   17 WORDS      variant 0: words -> rr_from_words, rr_to_mont_from_words; 1: a -> rr_to_words, rr_to_mont32_words;
 *                 2: words (an integer < param m) -> rr_from_mont32_words
 *   18 DFT8       a_0 .. a_7 (x0, x4, x2, x6, x1, x5, x3, x7), w8, w8^2, w8^3 (canonical, plain) -> dft8_rr's eight outputs; param
 *                 0: RRShoupU entries (the first case's of the wave), 1: RRShoup.  The three scalar fields only */
#define BLZ_RR_LAYOUT_WORDS 8192
int blz_test_rr_layout(int curve, int field, uint32_t* out);
int blz_test_rr_op(int device_id, int curve, int field, int op, int variant, const uint32_t* in, uint32_t* out, size_t n);

/* MsmEngine::begin()'s test for hiding a task's digit sort under another task's accumulation: 1 when a block of the sort (sort_vgprs
 * registers per lane, sort_lds bytes of LDS) fits on a CU beside the accumulation's blocks of 128 lanes (acc_vgprs, acc_lds), else 0.
 * Host only.  A count <= 0 is "not known" and is taken to fit. */
int blz_test_sort_fits_beside(int acc_vgprs, int sort_vgprs, int acc_lds, int sort_lds);

/* ------------------------------------------------------------------ Poseidon (blaze_hip.h "Poseidon")
 * words / len: an instruction word stream as blz_poseidon_initialize_words takes it.
 * blz_test_poseidon_permute: the DEFINITION kernel - one lane per state, the dense textbook rounds on the 8 x 32-bit Montgomery
 *   arithmetic (fp_mul, fp_add), sharing neither representation nor schedule with the product path; slow on purpose.  n states of
 *   t words each (host pointers; any 256-bit words, taken as residues), permuted, canonical.
 * blz_test_poseidon_hash: the PRODUCT path's kernel of width t on n independent inputs of t - 1 words (host pointers): n digests.
 * blz_test_poseidon_hash_plan: the same through the OPTIMISED PARTIAL ROUNDS (k_hades_hash), derived here for width t whatever the
 *   tree modes use: *state = 1 and n digests, or *state = 2 and no digests when the matrix without row 0 and column 0 is singular.
 * blz_test_poseidon_tree_check: every node of a finished tree re-hashed from its children by the definition kernel and compared
 *   on the device: d_input the tree's elements, d_records its records as blz_poseidon_tree_device returns them;
 *   out = {nodes checked, nodes whose record differs}. */
int blz_test_poseidon_permute(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* states_in,
                              uint8_t* states_out, size_t n);
int blz_test_poseidon_hash(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* inputs, uint8_t* digests,
                           size_t n);
int blz_test_poseidon_hash_plan(int device_id, int field, const uint8_t* words, size_t len, int t, const uint8_t* inputs, uint8_t* digests,
                                size_t n, uint32_t* state);
int blz_test_poseidon_tree_check(int device_id, int field, const uint8_t* words, size_t len, int tree_mode, uint32_t tree_height,
                                 const void* d_input, const void* d_records, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* BLAZE_HIP_AUX_H */
