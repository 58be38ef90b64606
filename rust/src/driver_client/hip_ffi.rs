//! `extern "C"` view of `include/blaze_hip.h` (libblaze_hip.so): what replaces the three XDMA file handles of the
//! reference's `DriverClient` (`/root/reference/src/driver_client/dclient.rs:50-59`).  One function per
//! `DriverPrimitive` method per primitive; plain pointers and sizes; return value 0 = Ok, else the ordinal of a
//! `DriverClientError` variant.  tests/test_rust_ffi.py compares every declaration below with the header.
#![allow(dead_code)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct BlzMsm {
    _private: [u8; 0],
}
#[repr(C)]
pub struct BlzNtt {
    _private: [u8; 0],
}
#[repr(C)]
pub struct BlzPoseidon {
    _private: [u8; 0],
}
/// `struct blz_vec_arg`: one operand of `blz_ntt_vec_op` - transform buffer `buf` of the handle (`d_ptr` null) or `count`
/// 32-byte device words at `d_ptr`, read periodically along the buffer position.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzVecArg {
    pub d_ptr: *const c_void,
    pub buf: u32,
    pub reserved: u32,
    pub count: u64,
}
/// `struct blz_vec_view`: the source positions `blz_ntt_vec_gather` reads - destination position p < `len` takes source element
/// (`offset` + `stride` p) mod count, positions from `len` up become 0.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzVecView {
    pub offset: u64,
    pub stride: u64,
    pub len: u64,
}
/// `struct blz_vec_scatter`: the nonzeros `blz_ntt_vec_scatter` adds up, index arrays in device memory.  `d_src` null: nonzero k
/// reads x\[k mod count\]; `d_val` null: every coefficient is 1; `reserved` must be 0.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzVecScatter {
    pub d_idx: *const u32,
    pub d_src: *const u32,
    pub d_val: *const c_void,
    pub nnz: u64,
    pub reserved: u64,
}
/// `struct blz_vec_csr`: the sparse matrix `blz_ntt_vec_spmv` multiplies by, CSR arrays in device memory.  `d_row_ptr` null: row p
/// holds nonzero p alone (`rows` == `nnz`); `d_val` null: every coefficient is 1.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzVecCsr {
    pub d_row_ptr: *const u32,
    pub d_col: *const u32,
    pub d_val: *const c_void,
    pub rows: u64,
    pub nnz: u64,
}
/// `BLZ_MLE_LOW`: `blz_ntt_vec_mle_fold` / `_round` pair (a\[2p\], a\[2p + 1\]) - variable 0 - instead of (a\[p\], a\[p + len / 2\]).
pub const BLZ_MLE_LOW: u32 = 1;
/// `BLZ_GKR_UNFUSED`: `blz_ntt_gkr_prove` takes the chain of single launches only, not its one-block kernel.
pub const BLZ_GKR_UNFUSED: u32 = 1;
/// `BLZ_GATE_PRODUCT`: the gate of `blz_ntt_sumcheck_step` is the product of its 1 to 3 tables.
pub const BLZ_GATE_PRODUCT: u32 = 0;
/// `BLZ_GATE_R1CS`: the gate is a (b c - d) over its four tables.
pub const BLZ_GATE_R1CS: u32 = 1;
/// The limits of a caller-defined gate (`blz_ntt_sumcheck_gate`): tables, terms, factors per term (the common factor not counted), points.
pub const BLZ_GATE_MAX_TABLES: usize = 12;
pub const BLZ_GATE_MAX_TERMS: usize = 8;
pub const BLZ_GATE_MAX_FACTORS: usize = 4;
pub const BLZ_GATE_MAX_POINTS: u32 = 6;
/// `struct blz_gate_term` (8 bytes): one signed product of `nfactors` tables, named by their index in the call's `tables`.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct BlzGateTerm {
    pub nfactors: u8,
    pub negate: u8,
    pub factor: [u8; BLZ_GATE_MAX_FACTORS],
    pub reserved: [u8; 2],
}
/// `struct blz_sum_gate` (80 bytes): G = T\[common\] x the signed sum of the first `nterms` terms; `common` = -1: no common factor.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzSumGate {
    pub ntables: u32,
    pub nterms: u32,
    pub common: i32,
    pub reserved: u32,
    pub term: [BlzGateTerm; BLZ_GATE_MAX_TERMS],
}
/// The limits and marks of a gate with linear-form factors (`blz_ntt_gate_eval_lin`): tables, forms, summands per form; a factor
/// byte (or `common`) `BLZ_LIN_FORM | k` names form k; a summand's `coef` `BLZ_LIN_NO_COEF` is the coefficient 1.
pub const BLZ_LIN_MAX_TABLES: usize = 16;
pub const BLZ_LIN_MAX_FORMS: usize = 8;
pub const BLZ_LIN_MAX_SUMMANDS: usize = 4;
pub const BLZ_LIN_FORM: u8 = 0x80;
pub const BLZ_LIN_NO_COEF: u8 = 0xFF;
/// `struct blz_lin_summand` (4 bytes): (+/-) \[T\[coef\] x\] T\[table\].
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct BlzLinSummand {
    pub coef: u8,
    pub table: u8,
    pub negate: u8,
    pub reserved: u8,
}
/// `struct blz_lin_form` (20 bytes): the signed sum of the first `nsummands` summands.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct BlzLinForm {
    pub nsummands: u8,
    pub reserved: [u8; 3],
    pub summand: [BlzLinSummand; BLZ_LIN_MAX_SUMMANDS],
}
/// `struct blz_lin_gate` (240 bytes): `blz_sum_gate` whose factors and `common` may name one of the first `nforms` forms.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct BlzLinGate {
    pub ntables: u32,
    pub nterms: u32,
    pub common: i32,
    pub nforms: u32,
    pub term: [BlzGateTerm; BLZ_GATE_MAX_TERMS],
    pub form: [BlzLinForm; BLZ_LIN_MAX_FORMS],
}

pub const BLZ_COMM_ID_BYTES: usize = 128;

extern "C" {
    pub fn blz_last_error_message() -> *const c_char;
    pub fn blz_device_count() -> c_int;
    pub fn blz_point_size(curve: c_int) -> usize;
    pub fn blz_result_size(curve: c_int) -> usize;

    // ---- MSM: MSMClient (msm_api.rs:42-331)
    pub fn blz_msm_new(device_id: c_int, mem_type: c_int, is_precompute: c_int, curve: c_int, out: *mut *mut BlzMsm) -> c_int;
    pub fn blz_msm_free(h: *mut BlzMsm);
    pub fn blz_msm_loaded_binary_parameters(h: *mut BlzMsm, out: *mut u32) -> c_int;
    pub fn blz_msm_initialize(h: *mut BlzMsm, nof_elements: u32, has_hbm: c_int, hbm_addr: u64, hbm_off: u64) -> c_int;
    pub fn blz_msm_start_process(h: *mut BlzMsm) -> c_int;
    pub fn blz_msm_set_data(
        h: *mut BlzMsm,
        points: *const u8,
        points_len: usize,
        scalars: *const u8,
        scalars_len: usize,
        nof_elements: u32,
        has_hbm: c_int,
        hbm_addr: u64,
        hbm_off: u64,
    ) -> c_int;
    pub fn blz_msm_wait_result(h: *mut BlzMsm) -> c_int;
    pub fn blz_msm_result(h: *mut BlzMsm, out: *mut u8, out_cap: usize, out_len: *mut usize, label: *mut u32) -> c_int;
    pub fn blz_msm_load_data_to_hbm(h: *mut BlzMsm, points: *const u8, len: usize, addr: u64, off: u64) -> c_int;
    pub fn blz_msm_get_data_from_hbm(h: *mut BlzMsm, out: *mut u8, len: usize, addr: u64, off: u64) -> c_int;
    pub fn blz_msm_task_label(h: *mut BlzMsm, out: *mut u32) -> c_int;
    pub fn blz_msm_nof_elements(h: *mut BlzMsm, out: *mut u32) -> c_int;
    pub fn blz_msm_is_engine_ready(h: *mut BlzMsm, out: *mut u32) -> c_int;
    pub fn blz_msm_stream_progress(h: *mut BlzMsm, out: *mut u32) -> c_int;
    pub fn blz_msm_reset(h: *mut BlzMsm) -> c_int;
    pub fn blz_msm_memory_info(h: *mut BlzMsm, out: *mut u64) -> c_int;
    pub fn blz_msm_set_window_table(h: *mut BlzMsm, enable: c_int) -> c_int;
    pub fn blz_msm_prepare_window_table(h: *mut BlzMsm, nof_elements: u32, hbm_addr: u64, hbm_off: u64, wait_ms: c_int, ready: *mut c_int) -> c_int;
    pub fn blz_msm_set_precompute_plan(h: *mut BlzMsm, enable: c_int) -> c_int;
    pub fn blz_msm_prepare_precompute_plan(h: *mut BlzMsm, nof_elements: u32, hbm_addr: u64, hbm_off: u64, consistent: *mut c_int) -> c_int;
    pub fn blz_msm_precompute_plan_info(h: *mut BlzMsm, out: *mut u64) -> c_int;
    pub fn blz_msm_set_scalar_range(h: *mut BlzMsm, bit_lo: u32, bit_hi: u32) -> c_int;
    pub fn blz_msm_shard_layout(curve: c_int, nof_elements: u32, nranks: c_int, rank: c_int, out: *mut u32) -> c_int;
    pub fn blz_msm_shard_layout_ex(curve: c_int, nof_elements: u32, nranks: c_int, rank: c_int, flags: u32, out: *mut u32) -> c_int;
    pub fn blz_msm_shard_layout_candidate(curve: c_int, nof_elements: u32, nranks: c_int, rank: c_int, flags: u32, r: c_int, out: *mut u32) -> c_int;
    pub fn blz_msm_window_table_info(h: *mut BlzMsm, out: *mut u64) -> c_int;
    pub fn blz_msm_last_timings(h: *mut BlzMsm, out: *mut f32) -> c_int;
    pub fn blz_msm_last_sort_hidden(h: *mut BlzMsm, out: *mut c_int) -> c_int;
    // multi-GPU exchange (no reference counterpart: README.md:20-22 leaves it to a "management layer")
    pub fn blz_msm_combine_partials(h: *mut BlzMsm, partials: *const u8, count: usize, out: *mut u8, out_cap: usize) -> c_int;
    pub fn blz_comm_unique_id(out: *mut u8) -> c_int;
    pub fn blz_msm_comm_init(h: *mut BlzMsm, rank: c_int, nranks: c_int, id: *const u8) -> c_int;
    pub fn blz_msm_all_gather_combine(h: *mut BlzMsm, partial: *const u8, out: *mut u8, out_cap: usize) -> c_int;
    pub fn blz_msm_comm_init_all(handles: *const *mut BlzMsm, n: c_int) -> c_int;
    pub fn blz_msm_all_gather_combine_all(handles: *const *mut BlzMsm, n: c_int, partials: *const u8, out: *mut u8, out_cap: usize) -> c_int;
    pub fn blz_msm_comm_free(h: *mut BlzMsm) -> c_int;
    // device arena
    pub fn blz_arena_release(device_id: c_int) -> c_int;
    pub fn blz_arena_export(device_id: c_int, registry_path: *const c_char) -> c_int;
    pub fn blz_arena_attach(device_id: c_int, registry_path: *const c_char) -> c_int;
    pub fn blz_msm_precompute_bases_device(device_id: c_int, curve: c_int, d_points_in: *const c_void, d_bases_out: *mut c_void, n: u64) -> c_int;

    // ---- NTT: NTTClient (ntt_api.rs:25-125)
    pub fn blz_ntt_new(device_id: c_int, log_size: c_int, out: *mut *mut BlzNtt) -> c_int;
    pub fn blz_ntt_new_ex(device_id: c_int, log_size: c_int, inverse: c_int, out: *mut *mut BlzNtt) -> c_int;
    pub fn blz_ntt_new_field(device_id: c_int, field: c_int, log_size: c_int, inverse: c_int, out: *mut *mut BlzNtt) -> c_int;
    pub fn blz_arena_set_policy(device_id: c_int, policy: u32) -> c_int;
    pub fn blz_host_malloc(device_id: c_int, bytes: usize, out: *mut *mut std::os::raw::c_void) -> c_int;
    pub fn blz_host_free(p: *mut std::os::raw::c_void) -> c_int;
    pub fn blz_ntt_new_ex2(device_id: c_int, field: c_int, log_size: c_int, inverse: c_int, flags: u32, out: *mut *mut BlzNtt) -> c_int;
    pub fn blz_ntt_new_ex3(device_id: c_int, field: c_int, log_size: c_int, flags: u32, root: *const u8, out: *mut *mut BlzNtt) -> c_int;
    pub fn blz_ntt_set_coset(h: *mut BlzNtt, shift: *const u8) -> c_int;
    pub fn blz_ntt_get_coset(h: *mut BlzNtt, out: *mut u8) -> c_int;
    pub fn blz_ntt_info(h: *mut BlzNtt, out: *mut u64) -> c_int;
    pub fn blz_ntt_exchange(h: *mut BlzNtt, buf: usize, next_in: *const u8, in_len: usize, prev_out: *mut u8, out_cap: usize) -> c_int;
    pub fn blz_ntt_free(h: *mut BlzNtt);
    pub fn blz_ntt_initialize(h: *mut BlzNtt) -> c_int;
    pub fn blz_ntt_set_data(h: *mut BlzNtt, buf_host: usize, data: *const u8, len: usize) -> c_int;
    pub fn blz_ntt_start_process(h: *mut BlzNtt, buf_kernel: usize) -> c_int;
    pub fn blz_ntt_wait_result(h: *mut BlzNtt) -> c_int;
    pub fn blz_ntt_result(h: *mut BlzNtt, buf: usize, out: *mut u8, out_cap: usize) -> c_int;
    pub fn blz_ntt_reset(h: *mut BlzNtt) -> c_int;
    pub fn blz_ntt_last_kernel_ms(h: *mut BlzNtt, out: *mut f32) -> c_int;
    pub fn blz_ntt_gate_eval(h: *mut BlzNtt, gate: *const BlzSumGate, dst: *const BlzVecArg, tables: *const BlzVecArg, rot: *const u64,
                             len: u64) -> c_int;
    pub fn blz_ntt_gate_eval_lin(h: *mut BlzNtt, gate: *const BlzLinGate, dst: *const BlzVecArg, tables: *const BlzVecArg, rot: *const u64,
                                 len: u64) -> c_int;
    pub fn blz_ntt_zerocheck_gate(h: *mut BlzNtt, gate: *const BlzSumGate, tables: *const BlzVecArg, weight: *const BlzVecArg, r: *const BlzVecArg,
                                  points: u32, len: u64, d_out: *mut c_void) -> c_int;
    pub fn blz_ntt_mle_tree(h: *mut BlzNtt, op: u32, flags: u32, dst: *const BlzVecArg, dst_q: *const BlzVecArg, a: *const BlzVecArg,
                            a_q: *const BlzVecArg, len: u64) -> c_int;
    pub fn blz_ntt_fs_challenge(h: *mut BlzNtt, d_state: *mut c_void, words: *const BlzVecArg, count: u32, d_r: *mut c_void) -> c_int;
    pub fn blz_ntt_sumcheck_prove(h: *mut BlzNtt, gate: *const BlzSumGate, tables: *const BlzVecArg, weight: *const BlzVecArg, points: u32,
                                  len: u64, d_state: *mut c_void, d_rounds: *mut c_void, d_challenges: *mut c_void) -> c_int;
    pub fn blz_ntt_gkr_prove(h: *mut BlzNtt, op: u32, flags: u32, tree: *const BlzVecArg, a: *const BlzVecArg, len: u64, d_weight: *mut c_void,
                             d_state: *mut c_void, d_rounds: *mut c_void, d_points: *mut c_void, d_claims: *mut c_void) -> c_int;
    pub fn blz_ntt_gkr_prove_frac(h: *mut BlzNtt, flags: u32, tree_p: *const BlzVecArg, tree_q: *const BlzVecArg, a_p: *const BlzVecArg,
                                  a_q: *const BlzVecArg, len: u64, d_weight: *mut c_void, d_state: *mut c_void, d_rounds: *mut c_void, d_points: *mut c_void,
                                  d_claims: *mut c_void, d_lambdas: *mut c_void) -> c_int;
    pub fn blz_ntt_vec_op(h: *mut BlzNtt, op: c_int, buf_dst: usize, a: *const BlzVecArg, b: *const BlzVecArg, c: *const BlzVecArg) -> c_int;
    pub fn blz_ntt_vec_reduce(h: *mut BlzNtt, op: c_int, a: *const BlzVecArg, b: *const BlzVecArg, d_out: *mut c_void) -> c_int;
    pub fn blz_ntt_vec_scan(h: *mut BlzNtt, op: c_int, flags: u32, buf_dst: usize, a: *const BlzVecArg, d_total: *mut c_void) -> c_int;
    pub fn blz_ntt_vec_horner(h: *mut BlzNtt, flags: u32, buf_dst: usize, a: *const BlzVecArg, z: *const BlzVecArg, d_total: *mut c_void) -> c_int;
    pub fn blz_ntt_vec_gather(h: *mut BlzNtt, buf_dst: usize, a: *const BlzVecArg, v: *const BlzVecView) -> c_int;
    pub fn blz_ntt_vec_scatter(h: *mut BlzNtt, buf_dst: usize, x: *const BlzVecArg, s: *const BlzVecScatter) -> c_int;
    pub fn blz_ntt_vec_spmv(h: *mut BlzNtt, buf_dst: usize, x: *const BlzVecArg, m: *const BlzVecCsr) -> c_int;
    pub fn blz_ntt_vec_mle_fold(h: *mut BlzNtt, flags: u32, dst: *const BlzVecArg, a: *const BlzVecArg, r: *const BlzVecArg, len: u64) -> c_int;
    pub fn blz_ntt_vec_mle_round(h: *mut BlzNtt, flags: u32, a: *const BlzVecArg, b: *const BlzVecArg, c: *const BlzVecArg, points: u32,
                                 len: u64, d_out: *mut c_void) -> c_int;
    pub fn blz_ntt_vec_mle_eq(h: *mut BlzNtt, dst: *const BlzVecArg, d_point: *const c_void, m: u32) -> c_int;
    pub fn blz_ntt_sumcheck_step(h: *mut BlzNtt, gate: u32, a: *const BlzVecArg, b: *const BlzVecArg, c: *const BlzVecArg, d: *const BlzVecArg,
                                 r: *const BlzVecArg, points: u32, len: u64, d_out: *mut c_void) -> c_int;
    pub fn blz_ntt_sumcheck_gate(h: *mut BlzNtt, gate: *const BlzSumGate, tables: *const BlzVecArg, r: *const BlzVecArg, points: u32, len: u64,
                                 d_out: *mut c_void) -> c_int;

    // ---- Poseidon tree: PoseidonClient (ingo_hash::poseidon_api)
    pub fn blz_poseidon_new(device_id: c_int, field: c_int, out: *mut *mut BlzPoseidon) -> c_int;
    pub fn blz_poseidon_free(h: *mut BlzPoseidon);
    pub fn blz_poseidon_loaded_binary_parameters(h: *mut BlzPoseidon, out: *mut u32) -> c_int;
    pub fn blz_poseidon_initialize(h: *mut BlzPoseidon, tree_height: u32, tree_mode: c_int, instruction_path: *const c_char) -> c_int;
    pub fn blz_poseidon_check_words(field: c_int, tree_mode: c_int, words: *const u8, len: usize, out: *mut u32) -> c_int;
    pub fn blz_poseidon_initialize_words(h: *mut BlzPoseidon, tree_height: u32, tree_mode: c_int, words: *const u8, len: usize) -> c_int;
    pub fn blz_poseidon_set_data(h: *mut BlzPoseidon, data: *const u8, len: usize) -> c_int;
    pub fn blz_poseidon_set_data_device(h: *mut BlzPoseidon, d_data: *const c_void, len: usize) -> c_int;
    pub fn blz_poseidon_wait_result(h: *mut BlzPoseidon) -> c_int;
    pub fn blz_poseidon_num_pending_results(h: *mut BlzPoseidon, out: *mut u32) -> c_int;
    pub fn blz_poseidon_raw_results(h: *mut BlzPoseidon, n: u32, out: *mut u8, cap: usize) -> c_int;
    pub fn blz_poseidon_result(h: *mut BlzPoseidon, expected: u32, out: *mut u8, cap: usize, n: *mut u32) -> c_int;
    pub fn blz_poseidon_tree_device(h: *mut BlzPoseidon, d_out: *mut c_void, cap: usize) -> c_int;
    pub fn blz_poseidon_counters(h: *mut BlzPoseidon, out: *mut u32) -> c_int;
    pub fn blz_poseidon_info(h: *mut BlzPoseidon, out: *mut u64) -> c_int;
    pub fn blz_poseidon_set_round_plan(h: *mut BlzPoseidon, enable: c_int) -> c_int;
    pub fn blz_poseidon_prepare_round_plan(h: *mut BlzPoseidon, out: *mut u32) -> c_int;
    pub fn blz_poseidon_last_kernel_ms(h: *mut BlzPoseidon, out: *mut f32) -> c_int;
    pub fn blz_poseidon_stream(h: *mut BlzPoseidon, hip_stream: *mut *mut c_void, device_id: *mut c_int) -> c_int;
    pub fn blz_poseidon_reset(h: *mut BlzPoseidon) -> c_int;
}
