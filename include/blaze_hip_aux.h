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
