//! `NTTClient` of `/root/reference/src/ingo_ntt/ntt_api.rs:8-125` over libblaze_hip.  The transform: size 2^27 over
//! the BLS12-381 scalar field, forward, natural order in and out, omega = 7^((r-1)/2^27) (the reference states none
//! of these).
use crate::{
    driver_client::{hip_ffi::*, *},
    error::*,
};

pub const NTT_LOG_SIZE: i32 = 27; // ntt_data.rs:65: NTT_SIZE = 2^27
pub const NTT_WORD_SIZE: usize = 32; // ntt_data.rs:66

pub enum NTT {
    Ntt,
}

pub struct NTTClient {
    nbytes: usize,
    pub driver_client: DriverClient,
    h: *mut BlzNtt,
}
unsafe impl Send for NTTClient {}

pub struct NttInit {}

#[derive(Debug, Clone)]
pub struct NTTInput {
    pub buf_host: usize,
    pub data: Vec<u8>,
}

impl DriverPrimitive<NTT, NttInit, NTTInput, Vec<u8>> for NTTClient {
    /// ntt_api.rs:26-31
    fn new(_ptype: NTT, dclient: DriverClient) -> Self {
        NTTClient::with_log_size(dclient, NTT_LOG_SIZE)
    }

    /// `todo!()` in the reference too (ntt_api.rs:33-35)
    fn loaded_binary_parameters(&self) -> Vec<u32> {
        todo!()
    }

    /// ntt_api.rs:37-56 writes the debug program; nothing to program here
    fn initialize(&self, _: NttInit) -> Result<()> {
        check(unsafe { blz_ntt_initialize(self.h) })
    }

    /// ntt_api.rs:58-70: select the buffer and AP_START
    fn start_process(&self, buf_kernel: Option<usize>) -> Result<()> {
        check(unsafe { blz_ntt_start_process(self.h, buf_kernel.unwrap()) })
    }

    /// ntt_api.rs:72-87: `NTTBanks::preprocess` and the 16 bank writes become one flat copy
    fn set_data(&self, input: NTTInput) -> Result<()> {
        check(unsafe { blz_ntt_set_data(self.h, input.buf_host, input.data.as_ptr(), input.data.len()) })
    }

    /// ntt_api.rs:89-108: the spin on AP_DONE
    fn wait_result(&self) -> Result<()> {
        check(unsafe { blz_ntt_wait_result(self.h) })
    }

    /// ntt_api.rs:110-124: 16 bank reads + `postprocess` become one flat copy
    fn result(&self, buf_num: Option<usize>) -> Result<Option<Vec<u8>>> {
        let mut res = vec![0u8; self.nbytes];
        check(unsafe { blz_ntt_result(self.h, buf_num.unwrap(), res.as_mut_ptr(), res.len()) })?;
        Ok(Some(res))
    }
}

impl Drop for NTTClient {
    fn drop(&mut self) {
        unsafe { blz_ntt_free(self.h) }
    }
}

impl NTTClient {
    /// Smaller transforms exist for tests (the reference has no such knob).
    pub fn with_log_size(dclient: DriverClient, log_size: i32) -> Self {
        let mut h: *mut BlzNtt = std::ptr::null_mut();
        check(unsafe { blz_ntt_new(dclient.id, log_size, &mut h) }).expect("blz_ntt_new failed");
        NTTClient { nbytes: NTT_WORD_SIZE << log_size, driver_client: dclient, h }
    }

    /// The transform's convention, which the reference leaves unstated (`NttInit {}` is empty, ntt_api.rs:8-23; its golden
    /// files are external, tests/integration_ntt.rs:15-18): `field` = a `Curve` as i32 (its scalar field), `flags` =
    /// BLZ_NTT_INVERSE (2) | BLZ_NTT_BITREV_INPUT (4) | BLZ_NTT_BITREV_OUTPUT (8) | BLZ_NTT_NO_FACTOR_TABLE (1), `root` = any
    /// primitive 2^log_size-th root of unity as 32 canonical little-endian bytes (checked on the device) or `None` for
    /// g^((r - 1) / 2^log_size).  A host that holds vectors made for the card says here what they assume.
    pub fn with_convention(dclient: DriverClient, field: i32, log_size: i32, flags: u32, root: Option<&[u8; 32]>) -> Result<Self> {
        let mut h: *mut BlzNtt = std::ptr::null_mut();
        let rp = root.map_or(std::ptr::null(), |r| r.as_ptr());
        check(unsafe { blz_ntt_new_ex3(dclient.id, field, log_size, flags, rp, &mut h) })?;
        Ok(NTTClient { nbytes: NTT_WORD_SIZE << log_size, driver_client: dclient, h })
    }

    /// Device time of the last transform in ms (HIP events around its three passes).
    pub fn last_kernel_ms(&self) -> Result<f32> {
        let mut v = 0f32;
        check(unsafe { blz_ntt_last_kernel_ms(self.h, &mut v) })?;
        Ok(v)
    }

    /// `result(Some(buf))` and `set_data(NTTInput { buf_host: buf, data })` of the double-buffered loop
    /// (tests/integration_ntt.rs:102-136) as one full-duplex call: the previous result leaves `buf` piece by piece into `out`
    /// while `data` lands in the places that have left.
    pub fn exchange(&self, buf: usize, data: &[u8], out: &mut [u8]) -> Result<()> {
        check(unsafe { blz_ntt_exchange(self.h, buf, data.as_ptr(), data.len(), out.as_mut_ptr(), out.len()) })
    }

    /// `[device bytes held, pass 2 reads its factor table (1) or steps (0), pass 1 boundary table, log_size]`.
    pub fn info(&self) -> Result<[u64; 4]> {
        let mut v = [0u64; 4];
        check(unsafe { blz_ntt_info(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }

    /// Transforms started from now on run on the coset `shift * <w>`: a forward client computes X[k] = sum_i x[i] shift^i w^(i k),
    /// an inverse one its exact inverse.  `shift` = 32 canonical little-endian bytes, 0 < shift < r (checked on the device);
    /// `None` (or 1) = the plain transform again.  Fused into the transform's passes (blaze_hip.h blz_ntt_set_coset).
    pub fn set_coset(&self, shift: Option<&[u8; 32]>) -> Result<()> {
        let sp = shift.map_or(std::ptr::null(), |s| s.as_ptr());
        check(unsafe { blz_ntt_set_coset(self.h, sp) })
    }

    /// The shift in force; the element 1 when the client runs the plain transform.
    pub fn coset(&self) -> Result<[u8; 32]> {
        let mut v = [0u8; 32];
        check(unsafe { blz_ntt_get_coset(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }

    /// Element-wise op over the client's n positions (blaze_hip.h blz_ntt_vec_op): transform buffer `dst` = a + b, a - b, a * b,
    /// a * b + c, a * b - c or 1 / a (0 -> 0), by `op` (`VecOp`).  Enqueued like a transform: `wait_result` finishes it.
    ///
    /// # Safety
    /// The library checks that a `VecOperand::Words` pointer is device memory of the client's device holding `count` words, and
    /// does not copy it: the kernels read it until `wait_result` (or `reset_engine`) returns.  The caller keeps that memory
    /// allocated and unwritten until then; nothing in the types enforces it.
    pub unsafe fn vec_op(&self, op: VecOp, dst: usize, a: VecOperand, b: Option<VecOperand>, c: Option<VecOperand>) -> Result<()> {
        let (ra, rb, rc) = (a.raw(), b.map(|v| v.raw()), c.map(|v| v.raw()));
        let p = |v: &Option<BlzVecArg>| v.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg);
        check(blz_ntt_vec_op(self.h, op as std::os::raw::c_int, dst, &ra, p(&rb), p(&rc)))
    }

    /// One value out of a vector (blaze_hip.h blz_ntt_vec_reduce): `d_out` (32 bytes of device memory) = sum a, sum a * b, or
    /// sum a\[p\] z^p with z the one-word operand `b`, by `op` (`FoldOp`).  Enqueued like a transform: `wait_result` finishes it.
    ///
    /// # Safety
    /// As for `vec_op`; `d_out` too stays allocated until `wait_result` (or `reset_engine`) returns.
    pub unsafe fn vec_reduce(&self, op: FoldOp, a: VecOperand, b: Option<VecOperand>, d_out: *mut std::os::raw::c_void) -> Result<()> {
        let (ra, rb) = (a.raw(), b.map(|v| v.raw()));
        let pb = rb.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg);
        check(blz_ntt_vec_reduce(self.h, op as std::os::raw::c_int, &ra, pb, d_out))
    }

    /// Prefix scan along the buffer (blz_ntt_vec_scan): transform buffer `dst`\[p\] = a\[0\] o .. o a\[p\], or with `exclusive`
    /// the identity at p = 0 and a\[0\] o .. o a\[p - 1\] after it; `d_total` (null, or 32 bytes of device memory) = the fold of
    /// all n elements.  `a` may name `dst`.
    ///
    /// # Safety
    /// As for `vec_reduce`.
    pub unsafe fn vec_scan(&self, op: ScanOp, exclusive: bool, dst: usize, a: VecOperand, d_total: *mut std::os::raw::c_void) -> Result<()> {
        let ra = a.raw();
        check(blz_ntt_vec_scan(self.h, op as std::os::raw::c_int, if exclusive { 1 } else { 0 }, dst, &ra, d_total))
    }

    /// Weighted (Horner) scan along the buffer (blz_ntt_vec_horner): transform buffer `dst`\[p\] = a\[p\] + z dst\[p - 1\], with
    /// `reverse` a\[p\] + z dst\[p + 1\]; `exclusive` shifts the result by one position and puts 0 at the open end.  `z` is one
    /// device word (`VecOperand::Words { count: 1, .. }`); `d_total` (null, or 32 bytes of device memory) = the last inclusive
    /// value, with `reverse` a(z).  `a` may name `dst`.
    ///
    /// # Safety
    /// As for `vec_reduce`.
    pub unsafe fn vec_horner(&self, exclusive: bool, reverse: bool, dst: usize, a: VecOperand, z: VecOperand,
                             d_total: *mut std::os::raw::c_void) -> Result<()> {
        let (ra, rz) = (a.raw(), z.raw());
        let flags = (if exclusive { 1 } else { 0 }) | (if reverse { 2 } else { 0 });
        check(blz_ntt_vec_horner(self.h, flags, dst, &ra, &rz, d_total))
    }

    /// Division by X - z: transform buffer `dst` = the n coefficients of the quotient of a(X) = sum a\[p\] X^p by X - z (the top
    /// one is 0), `d_rem` (null, or 32 bytes of device memory) = the remainder a(z).  A reverse, exclusive `vec_horner`.
    ///
    /// # Safety
    /// As for `vec_reduce`.
    pub unsafe fn vec_divide(&self, dst: usize, a: VecOperand, z: VecOperand, d_rem: *mut std::os::raw::c_void) -> Result<()> {
        self.vec_horner(true, true, dst, a, z, d_rem)
    }

    /// Gather along the buffer (blz_ntt_vec_gather): transform buffer `dst`\[p\] = a\[(offset + stride p) mod count\] for
    /// p < `len` and 0 for `len` <= p < n.  `a` is a transform buffer (count = n; `dst` itself: in place, through the client's
    /// scratch at twice the traffic) or `count` device words, a power of two that may exceed n (up to 2^27).  `stride` is taken
    /// modulo count: count - 1 walks backwards, 0 broadcasts one word.  Every output word is canonical.
    ///
    /// # Safety
    /// As for `vec_op`.
    pub unsafe fn vec_gather(&self, dst: usize, a: VecOperand, offset: u64, stride: u64, len: u64) -> Result<()> {
        let (ra, view) = (a.raw(), BlzVecView { offset, stride, len });
        check(blz_ntt_vec_gather(self.h, dst, &ra, &view))
    }

    /// Rotation: transform buffer `dst`\[p\] = a\[(p + k) mod n\], k of either sign; `a` holds n words.  On the domain,
    /// rotating the values of Z(X) by 1 gives those of Z(wX); on a 4n coset, by 4.  A `vec_gather` with stride 1.
    ///
    /// # Safety
    /// As for `vec_op`.
    pub unsafe fn vec_rotate(&self, dst: usize, a: VecOperand, k: i64) -> Result<()> {
        let n = (self.nbytes / NTT_WORD_SIZE) as u64;
        self.vec_gather(dst, a, k.rem_euclid(n as i64) as u64, 1, n)
    }

    /// Low-degree extension: transform buffer `dst` = the `count` <= n device words at `d_ptr` with zeros above them (n
    /// coefficients into a 4n client).  A `vec_gather` with len = count.
    ///
    /// # Safety
    /// As for `vec_op`.
    pub unsafe fn vec_extend(&self, dst: usize, d_ptr: *const std::os::raw::c_void, count: u64) -> Result<()> {
        self.vec_gather(dst, VecOperand::Words { d_ptr, count }, 0, 1, count)
    }

    /// Scatter-add (blz_ntt_vec_scatter): transform buffer `dst`\[t\] = the sum over k < `nnz` with `d_idx`\[k\] mod n == t of
    /// val\[k\] x\[src(k) mod count\], src(k) = `d_src`\[k\] or, with a null `d_src`, k; a position no nonzero names becomes 0.
    /// `x` None: every x word is 1 (and `d_src` must be null); a null `d_val`: every coefficient is 1; both: the histogram of
    /// `d_idx` (`vec_count`).  With `d_idx` the columns, `d_src` the row of each nonzero and `x` = y it is the transposed
    /// sparse product.  `x` may not name `dst`.  Exact in the field: two runs give the same bytes.
    ///
    /// # Safety
    /// As for `vec_op`; the three arrays are device memory of the client's device that stays valid and unwritten until
    /// `wait_result` returns.
    pub unsafe fn vec_scatter(&self, dst: usize, x: Option<VecOperand>, d_idx: *const u32, d_src: *const u32,
                              d_val: *const std::os::raw::c_void, nnz: u64) -> Result<()> {
        let (rx, s) = (x.map(|v| v.raw()), BlzVecScatter { d_idx, d_src, d_val, nnz, reserved: 0 });
        check(blz_ntt_vec_scatter(self.h, dst, rx.as_ref().map_or(std::ptr::null(), |r| r as *const BlzVecArg), &s))
    }

    /// Multiplicities: transform buffer `dst`\[t\] = the number of entries k < `nnz` of `d_idx` with `d_idx`\[k\] mod n == t, as a
    /// field element.  A `vec_scatter` without x and coefficients.
    ///
    /// # Safety
    /// As for `vec_scatter`.
    pub unsafe fn vec_count(&self, dst: usize, d_idx: *const u32, nnz: u64) -> Result<()> {
        self.vec_scatter(dst, None, d_idx, std::ptr::null(), std::ptr::null(), nnz)
    }

    /// Sparse matrix times vector (blz_ntt_vec_spmv): transform buffer `dst`\[p\] = the sum over the nonzeros k of row p
    /// (`d_row_ptr`\[p\] <= k < `d_row_ptr`\[p + 1\]) of val\[k\] x\[col\[k\] mod count\] for p < `rows`, 0 for an empty row and
    /// for `rows` <= p < n.  `x` is the other transform buffer or `count` device words (a power of two up to 2^27); it may not
    /// name `dst`.  A null `d_row_ptr` is index mode (`rows` == `nnz`, row p is nonzero p), a null `d_val` means coefficients 1.
    /// Every output word is canonical.
    ///
    /// # Safety
    /// As for `vec_op`; the three arrays are device memory of the client's device that stays valid and unwritten until
    /// `wait_result` returns.
    pub unsafe fn vec_spmv(&self, dst: usize, x: VecOperand, d_row_ptr: *const u32, d_col: *const u32,
                           d_val: *const std::os::raw::c_void, rows: u64, nnz: u64) -> Result<()> {
        let (rx, m) = (x.raw(), BlzVecCsr { d_row_ptr, d_col, d_val, rows, nnz });
        check(blz_ntt_vec_spmv(self.h, dst, &rx, &m))
    }

    /// Data-dependent gather: transform buffer `dst`\[p\] = x\[col\[p\] mod count\] (times val\[p\] unless `d_val` is null) for
    /// p < `count` entries of `d_col`, 0 above: a PLONK wire column, a looked-up column, a permutation held as an index table.
    /// A `vec_spmv` without row pointers.
    ///
    /// # Safety
    /// As for `vec_spmv`.
    pub unsafe fn vec_index(&self, dst: usize, x: VecOperand, d_col: *const u32, count: u64, d_val: *const std::os::raw::c_void) -> Result<()> {
        self.vec_spmv(dst, x, std::ptr::null(), d_col, d_val, count, count)
    }

    /// Bind one variable of a multilinear table (blz_ntt_vec_mle_fold): dst\[p\] = lo + r (hi - lo) for p < `len` / 2, with
    /// (lo, hi) = (a\[p\], a\[p + len / 2\]) - the top variable - or, with `low`, (a\[2p\], a\[2p + 1\]) - variable 0.  `dst` is a
    /// transform buffer or device words (count a power of two, len / 2 <= count <= n) and may be `a` itself; exactly len / 2
    /// words are written and every other byte of the destination keeps its value.  `r` is one device word
    /// (`VecOperand::Words { count: 1, .. }`) the host never reads.
    ///
    /// # Safety
    /// As for `vec_op`; device words named by `dst` are WRITTEN until `wait_result` returns.
    pub unsafe fn vec_mle_fold(&self, dst: VecOperand, a: VecOperand, r: VecOperand, len: u64, low: bool) -> Result<()> {
        let (rd, ra, rr) = (dst.raw(), a.raw(), r.raw());
        check(blz_ntt_vec_mle_fold(self.h, if low { BLZ_MLE_LOW } else { 0 }, &rd, &ra, &rr, len))
    }

    /// One round polynomial of a sumcheck (blz_ntt_vec_mle_round): `d_out`\[t\] = the sum over p < `len` / 2 of the product over
    /// the k tables given (a, then b, then c) of lo + t (hi - lo), for t = 0 .. `points` - 1 (1 ..= 4; k + 1 values determine the
    /// polynomial), pairing as in `vec_mle_fold`.  `d_out` is `points` x 32 bytes of device memory; nothing else is written.
    ///
    /// # Safety
    /// As for `vec_reduce`.
    pub unsafe fn vec_mle_round(&self, a: VecOperand, b: Option<VecOperand>, c: Option<VecOperand>, points: u32, len: u64, low: bool,
                                d_out: *mut std::os::raw::c_void) -> Result<()> {
        let (ra, rb, rc) = (a.raw(), b.map(|v| v.raw()), c.map(|v| v.raw()));
        let p = |v: &Option<BlzVecArg>| v.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg);
        check(blz_ntt_vec_mle_round(self.h, if low { BLZ_MLE_LOW } else { 0 }, &ra, p(&rb), p(&rc), points, len, d_out))
    }

    /// The equality table (blz_ntt_vec_mle_eq): dst\[p\] = prod over i < `m` of (x_i tau_i + (1 - x_i)(1 - tau_i)) for p < 2^m,
    /// x_i bit i of p, tau_i word i of `d_point` (m x 32 bytes of device memory the host never reads; null with m = 0, which
    /// writes the single word 1).  `dst` as for `vec_mle_fold`; exactly 2^m words are written.
    ///
    /// # Safety
    /// As for `vec_mle_fold`; `d_point` stays valid and unwritten until `wait_result` returns.
    pub unsafe fn vec_mle_eq(&self, dst: VecOperand, d_point: *const std::os::raw::c_void, m: u32) -> Result<()> {
        let rd = dst.raw();
        check(blz_ntt_vec_mle_eq(self.h, &rd, d_point, m))
    }

    /// One step of a sumcheck in one pass (blz_ntt_sumcheck_step).  `tables` are the gate's operands a, b, c, d in order, the ones
    /// not taken `None`: `BLZ_GATE_PRODUCT` takes 1 to 3 (G = a, a b, a b c), `BLZ_GATE_R1CS` (`r1cs`) four (G = a (b c - d)).  With `r` (one device word the host never reads)
    /// every table is folded IN PLACE - T\[p\] = T\[p\] + r (T\[p + len / 2\] - T\[p\]) for p < `len` / 2, exactly len / 2 words
    /// of each - and `d_out`\[t\], t < `points` (1 ..= 4), is the round polynomial of the folded tables: what `vec_mle_round` at
    /// len / 2 would write.  Without `r` it is the round polynomial of the tables as they are and nothing else is written.
    /// `points` = 0 with a null `d_out` (and `r`) binds only.  Both transform buffers may be tables; with `r` both are then
    /// written.
    ///
    /// # Safety
    /// As for `vec_mle_fold`: with `r`, device words named by `tables` are WRITTEN until `wait_result` returns; `d_out` as for
    /// `vec_reduce`.
    pub unsafe fn sumcheck_step(&self, r1cs: bool, tables: [Option<VecOperand>; 4], r: Option<VecOperand>, points: u32, len: u64,
                                d_out: *mut std::os::raw::c_void) -> Result<()> {
        let raw = tables.map(|v| v.map(|x| x.raw()));
        let rr = r.map(|v| v.raw());
        let p = |v: &Option<BlzVecArg>| v.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg);
        check(blz_ntt_sumcheck_step(self.h, if r1cs { BLZ_GATE_R1CS } else { BLZ_GATE_PRODUCT }, p(&raw[0]), p(&raw[1]), p(&raw[2]), p(&raw[3]),
                                    p(&rr), points, len, d_out))
    }

    /// The same step for a caller-defined gate (blz_ntt_sumcheck_gate): G = T\[common\] x the signed sum of `terms`, each
    /// `(negate, table indices)` a product of 1 ..= 4 of the `tables` (at most 12; an index may repeat; `common` may also be a
    /// factor).  With `r` EVERY table is folded in place, named by a term or not; `points` is 1 ..= 6, or 0 with a null `d_out`
    /// (and `r`) to bind only.  Without `r` the round alone, periodic tables allowed.
    ///
    /// # Safety
    /// As for `sumcheck_step`.
    pub unsafe fn sumcheck_gate(&self, tables: &[VecOperand], terms: &[(bool, &[u8])], common: Option<u8>, r: Option<VecOperand>, points: u32,
                                len: u64, d_out: *mut std::os::raw::c_void) -> Result<()> {
        let gate = Self::sum_gate(tables.len(), terms, common);
        let raw: Vec<BlzVecArg> = tables.iter().map(|x| x.raw()).collect();
        let rr = r.map(|v| v.raw());
        check(blz_ntt_sumcheck_gate(self.h, &gate, if raw.is_empty() { std::ptr::null() } else { raw.as_ptr() },
                                    rr.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg), points, len, d_out))
    }

    /// The gate step of a zerocheck (blz_ntt_zerocheck_gate): `sumcheck_gate` with eq out of the gate and the summed `weight`
    /// table - device words, for round 0 `vec_mle_eq` over m - 1 variables - in its place.  Without `r`: `d_out`\[t\] =
    /// sum_p W\[p\] G(pair p at t).  With `r` every table is folded in place, W\[q\] += W\[q + len / 4\] for q < len / 4 (no
    /// product), and `d_out` is the weighted round of the folded tables: u_i of s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X), one point
    /// fewer than with eq as `common`.  `points` is 1 ..= 6; the bind alone stays `sumcheck_gate`'s.
    ///
    /// # Safety
    /// As for `sumcheck_step`; with `r` the first len / 4 words of `weight` are written.
    pub unsafe fn zerocheck_gate(&self, tables: &[VecOperand], terms: &[(bool, &[u8])], weight: VecOperand, common: Option<u8>, r: Option<VecOperand>,
                                 points: u32, len: u64, d_out: *mut std::os::raw::c_void) -> Result<()> {
        let gate = Self::sum_gate(tables.len(), terms, common);
        let raw: Vec<BlzVecArg> = tables.iter().map(|x| x.raw()).collect();
        let (rw, rr) = (weight.raw(), r.map(|v| v.raw()));
        check(blz_ntt_zerocheck_gate(self.h, &gate, if raw.is_empty() { std::ptr::null() } else { raw.as_ptr() }, &rw,
                                     rr.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg), points, len, d_out))
    }

    /// The `blz_sum_gate` of `ntables` tables, `terms` and `common`, for `sumcheck_gate` and `gate_eval` alike
    fn sum_gate(ntables: usize, terms: &[(bool, &[u8])], common: Option<u8>) -> BlzSumGate {
        let mut gate = BlzSumGate { ntables: ntables as u32, nterms: terms.len() as u32, common: common.map_or(-1, |c| c as i32), reserved: 0,
                                    term: [BlzGateTerm::default(); BLZ_GATE_MAX_TERMS] };
        for (slot, (negate, factors)) in gate.term.iter_mut().zip(terms.iter()) {
            // a count the library refuses stays refusable: it is passed on, the indices that fit are copied
            slot.nfactors = factors.len().min(255) as u8;
            slot.negate = *negate as u8;
            for (f, t) in slot.factor.iter_mut().zip(factors.iter()) {
                *f = *t;
            }
        }
        gate
    }

    /// The same description evaluated position by position (blz_ntt_gate_eval): `dst`\[p\] = T\[common\]\[p_c\] x the signed sum
    /// of `terms` for p < `len` (1 ..= n, any value), table i read at p_i = (p + `rot`\[i\]) mod its count.  `tables` and `terms`
    /// as for `sumcheck_gate`; a table is a transform buffer or a power of two of device words up to n, read periodically (one
    /// word: a scalar).  `rot` holds one rotation per table (`None`: all zero; any u64, `u64::MAX` reads the previous row).
    /// `dst` as for `vec_mle_fold`; exactly `len` words are written.  `dst` may be one of the tables if that table starts where
    /// `dst` starts, holds `len` words and is not rotated: dst <- dst + alpha a b is one op.
    ///
    /// # Safety
    /// As for `vec_mle_fold`: device words named by `dst` are WRITTEN, those named by `tables` read, until `wait_result` returns.
    pub unsafe fn gate_eval(&self, dst: VecOperand, tables: &[VecOperand], terms: &[(bool, &[u8])], common: Option<u8>, rot: Option<&[u64]>,
                            len: u64) -> Result<()> {
        if let Some(k) = rot {
            if k.len() != tables.len() {
                return Err(DriverClientError::InvalidPrimitiveParam);
            }
        }
        let gate = Self::sum_gate(tables.len(), terms, common);
        let raw: Vec<BlzVecArg> = tables.iter().map(|x| x.raw()).collect();
        let rd = dst.raw();
        check(blz_ntt_gate_eval(self.h, &gate, &rd, if raw.is_empty() { std::ptr::null() } else { raw.as_ptr() },
                                rot.map_or(std::ptr::null(), |k| k.as_ptr()), len))
    }

    /// `gate_eval` with linear-form factors (blz_ntt_gate_eval_lin) - products of sums.  A factor byte of `terms`, and `common`,
    /// is a table index or `BLZ_LIN_FORM | k`, the value of `forms`\[k\]; a form is 1 to 4 summands `(negate, coef, table)`:
    /// (+/-) \[T\[coef\] x\] T\[table\], `coef` `None` for 1.  At most 16 tables, 8 forms, 8 terms; `rot` holds one rotation per
    /// table index, whatever names the index.  A one-word coefficient costs one product per position, a longer one two.
    /// `dst`, `len` and in place as for `gate_eval`.
    ///
    /// # Safety
    /// As for `gate_eval`.
    pub unsafe fn gate_eval_lin(&self, dst: VecOperand, tables: &[VecOperand], forms: &[&[(bool, Option<u8>, u8)]], terms: &[(bool, &[u8])],
                                common: Option<u8>, rot: Option<&[u64]>, len: u64) -> Result<()> {
        if rot.map_or(false, |k| k.len() != tables.len()) || forms.len() > BLZ_LIN_MAX_FORMS || terms.len() > BLZ_GATE_MAX_TERMS {
            return Err(DriverClientError::InvalidPrimitiveParam);
        }
        let sum = Self::sum_gate(tables.len(), terms, common);
        let mut gate = BlzLinGate { ntables: sum.ntables, nterms: sum.nterms, common: sum.common, nforms: forms.len() as u32, term: sum.term,
                                    form: [BlzLinForm::default(); BLZ_LIN_MAX_FORMS] };
        for (slot, form) in gate.form.iter_mut().zip(forms.iter()) {
            // a count the library refuses stays refusable: it is passed on, the summands that fit are copied
            slot.nsummands = form.len().min(255) as u8;
            for (x, (negate, coef, table)) in slot.summand.iter_mut().zip(form.iter()) {
                *x = BlzLinSummand { coef: coef.unwrap_or(BLZ_LIN_NO_COEF), table: *table, negate: *negate as u8, reserved: 0 };
            }
        }
        let raw: Vec<BlzVecArg> = tables.iter().map(|x| x.raw()).collect();
        let rd = dst.raw();
        check(blz_ntt_gate_eval_lin(self.h, &gate, &rd, if raw.is_empty() { std::ptr::null() } else { raw.as_ptr() },
                                    rot.map_or(std::ptr::null(), |k| k.as_ptr()), len))
    }

    /// Every layer of the product or fraction tree under the `len` = 2^m words of `a` (blz_ntt_mle_tree).  Layer k holds
    /// len / 2^k words at word `tree_layer(len, k).0` of `dst`; len - 1 words are written.  Pairs are (L\[p\], L\[p + size / 2\]),
    /// or (L\[2p\], L\[2p + 1\]) with `low`.  `TreeOp::Prod`: L'\[p\] = lo hi.  `TreeOp::Frac`: `frac` = `Some((dst_q, a_q))`,
    /// (P, Q)' = (P_lo Q_hi + P_hi Q_lo, Q_lo Q_hi), never inverted.  A destination meets no source and not the other one.
    ///
    /// # Safety
    /// As for `vec_mle_fold`: device words named by `dst` and `dst_q` are WRITTEN, those named by the sources read, until
    /// `wait_result` returns.
    pub unsafe fn mle_tree(&self, op: TreeOp, dst: VecOperand, a: VecOperand, frac: Option<(VecOperand, VecOperand)>, len: u64, low: bool) -> Result<()> {
        let (rd, ra) = (dst.raw(), a.raw());
        let rq = frac.map(|(d, s)| (d.raw(), s.raw()));
        check(blz_ntt_mle_tree(self.h, op as u32, low as u32, &rd, rq.as_ref().map_or(std::ptr::null(), |x| &x.0 as *const BlzVecArg), &ra,
                               rq.as_ref().map_or(std::ptr::null(), |x| &x.1 as *const BlzVecArg), len))
    }

    /// (word offset, words) of layer `k` (1 ..= m) in a destination of `mle_tree` over `len` = 2^m words
    pub fn tree_layer(len: u64, k: u32) -> (u64, u64) {
        (len - (len >> (k - 1)), len >> k)
    }

    /// One step of the on-device Fiat-Shamir transcript (blz_ntt_fs_challenge): digest = SHA3-256(state || the first `count`
    /// words of `words`, as stored); the digest is the new state at `d_state` and, with every bit from bitlen(modulus) - 1
    /// upward cleared (252 bits kept on BLS12-377, 254 on BLS12-381, 253 on BN254), the challenge at `d_r`.  `count` <= 32;
    /// `words` may be `None` when it is 0; a null `d_r` absorbs only.
    ///
    /// # Safety
    /// `d_state` and `d_r` (if not null) are one 16-byte aligned device word each, WRITTEN, off each other and off the words
    /// read; all stay valid until `wait_result` returns.
    pub unsafe fn fs_challenge(&self, d_state: *mut std::os::raw::c_void, words: Option<VecOperand>, count: u32,
                               d_r: *mut std::os::raw::c_void) -> Result<()> {
        let rw = words.map(|v| v.raw());
        check(blz_ntt_fs_challenge(self.h, d_state, rw.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg), count, d_r))
    }

    /// A whole sumcheck in one call (blz_ntt_sumcheck_prove): the round alone, then per variable the transcript step over the
    /// round just written and the step with that challenge, then the bind alone - no host wait in between.  `weight` `None`
    /// proves the sum of the gate with `sumcheck_gate`'s steps, `Some` the weighted sum with `zerocheck_gate`'s (len / 2 device
    /// words).  m = log2 `len`; `d_rounds` receives m x `points` words, `d_challenges` m words, `d_state` is the transcript.
    ///
    /// # Safety
    /// As for `sumcheck_gate` with `r`: every table is folded in place, the weight summed in place; the three outputs are
    /// device words off every table, the weight and each other, valid until `wait_result` returns.
    pub unsafe fn sumcheck_prove(&self, tables: &[VecOperand], terms: &[(bool, &[u8])], weight: Option<VecOperand>, common: Option<u8>, points: u32,
                                 len: u64, d_state: *mut std::os::raw::c_void, d_rounds: *mut std::os::raw::c_void,
                                 d_challenges: *mut std::os::raw::c_void) -> Result<()> {
        let gate = Self::sum_gate(tables.len(), terms, common);
        let raw: Vec<BlzVecArg> = tables.iter().map(|x| x.raw()).collect();
        let rw = weight.map(|v| v.raw());
        check(blz_ntt_sumcheck_prove(self.h, &gate, if raw.is_empty() { std::ptr::null() } else { raw.as_ptr() },
                                     rw.as_ref().map_or(std::ptr::null(), |x| x as *const BlzVecArg), points, len, d_state, d_rounds, d_challenges))
    }

    /// The GKR grand product over a product tree in one call (blz_ntt_gkr_prove).  `tree` is what `mle_tree(TreeOp::Prod, tree,
    /// a, None, len, false)` left over the `len` = 2^m leaves `a`.  From the root down, layer j's sumcheck runs under the weight
    /// eq(row j - 1 of the points) with every challenge made on the device - written backwards into row j, which is thereby the
    /// next layer's point -, then the two final words go to the claims and through one more transcript step.  `d_rounds`
    /// receives 3 m (m - 1) / 2 words, `d_points` m (m + 1) / 2, `d_claims` 2 m (`gkr_layout`); `d_weight` is max(len / 4, 1)
    /// words of scratch; `d_state` is the transcript.  `fused` false passes BLZ_GKR_UNFUSED: the chain of single launches.
    ///
    /// # Safety
    /// `tree` and `a` are consumed (the first half of each half-layer is WRITTEN); the five pointers are 16-byte aligned device
    /// words, WRITTEN, off the tree, the leaves and each other; all stay valid until `wait_result` returns.
    pub unsafe fn gkr_prove(&self, tree: VecOperand, a: VecOperand, len: u64, d_weight: *mut std::os::raw::c_void, d_state: *mut std::os::raw::c_void,
                            d_rounds: *mut std::os::raw::c_void, d_points: *mut std::os::raw::c_void, d_claims: *mut std::os::raw::c_void,
                            fused: bool) -> Result<()> {
        let (rt, ra) = (tree.raw(), a.raw());
        check(blz_ntt_gkr_prove(self.h, TreeOp::Prod as u32, if fused { 0 } else { BLZ_GKR_UNFUSED }, &rt, &ra, len, d_weight, d_state, d_rounds, d_points,
                                d_claims))
    }

    /// (words of rounds, words of points, words of claims) that `gkr_prove` writes for a tree over 2^m leaves; layer j's round i
    /// is at word 3 (j (j - 1) / 2 + i) of the rounds, its point row at word j (j + 1) / 2, its claims at word 2 j
    pub fn gkr_layout(m: u64) -> (u64, u64, u64) {
        (3 * m * m.saturating_sub(1) / 2, m * (m + 1) / 2, 2 * m)
    }

    /// The GKR argument over a fraction tree (logUp-GKR) in one call (blz_ntt_gkr_prove_frac).  `tree_p`, `tree_q` are what
    /// `mle_tree(TreeOp::Frac, ..)` left over the `len` = 2^m numerators `a_p` and denominators `a_q`; none of the four is
    /// periodic.  From the root down, layer j >= 1 draws the batching challenge lambda_j from the transcript, writes
    /// T = P_hi + lambda_j Q_hi over P_hi and proves sum eq (P_lo Q_hi + Q_lo T) under the weight eq(row j - 1 of the points);
    /// the four final words (P_lo, P_hi, Q_lo, Q_hi at the challenges) go to the claims and through one transcript step.
    /// `d_rounds` and `d_points` as for `gkr_prove`, `d_claims` 4 m words, `d_lambdas` m words of which word 0 is never written
    /// (`gkr_layout_frac`).  `fused` false passes BLZ_GKR_UNFUSED: the chain of single launches.
    ///
    /// # Safety
    /// The four operands are consumed (of the numerators the whole hi half and the first half of the lo half of each layer is
    /// WRITTEN, of the denominators the first half of each half); the six pointers are 16-byte aligned device words, WRITTEN,
    /// off the operands and each other; all stay valid until `wait_result` returns.
    pub unsafe fn gkr_prove_frac(&self, tree_p: VecOperand, tree_q: VecOperand, a_p: VecOperand, a_q: VecOperand, len: u64,
                                 d_weight: *mut std::os::raw::c_void, d_state: *mut std::os::raw::c_void, d_rounds: *mut std::os::raw::c_void,
                                 d_points: *mut std::os::raw::c_void, d_claims: *mut std::os::raw::c_void, d_lambdas: *mut std::os::raw::c_void,
                                 fused: bool) -> Result<()> {
        let (tp, tq, ap, aq) = (tree_p.raw(), tree_q.raw(), a_p.raw(), a_q.raw());
        check(blz_ntt_gkr_prove_frac(self.h, if fused { 0 } else { BLZ_GKR_UNFUSED }, &tp, &tq, &ap, &aq, len, d_weight, d_state, d_rounds, d_points,
                                     d_claims, d_lambdas))
    }

    /// (words of rounds, of points, of claims, of lambdas) that `gkr_prove_frac` writes for trees over 2^m leaves; rounds and
    /// points are laid out as `gkr_layout` says, layer j's four claims are at word 4 j, lambda_j at word j
    pub fn gkr_layout_frac(m: u64) -> (u64, u64, u64, u64) {
        (3 * m * m.saturating_sub(1) / 2, m * (m + 1) / 2, 4 * m, m)
    }

    pub fn reset_engine(&self) -> Result<()> {
        check(unsafe { blz_ntt_reset(self.h) })
    }
}

/// `enum blz_tree_op`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(u32)]
pub enum TreeOp {
    Prod = 0,
    Frac = 1,
}

/// `enum blz_vec_op`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum VecOp {
    Add = 0,
    Sub = 1,
    Mul = 2,
    MulAdd = 3,
    MulSub = 4,
    Inv = 5,
}

/// `enum blz_fold_op`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum FoldOp {
    Sum = 0,
    Dot = 1,
    Eval = 2,
}

/// `enum blz_scan_op`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum ScanOp {
    Sum = 0,
    Prod = 1,
}

/// An operand of `NTTClient::vec_op`: a transform buffer of the client (0 | 1), or `count` 32-byte device words (a power of two
/// up to n; 1 = a scalar) read periodically along the buffer position.
#[derive(Clone, Copy)]
pub enum VecOperand {
    Buffer(u32),
    Words { d_ptr: *const std::os::raw::c_void, count: u64 },
}

impl VecOperand {
    fn raw(&self) -> BlzVecArg {
        match *self {
            VecOperand::Buffer(buf) => BlzVecArg { d_ptr: std::ptr::null(), buf, reserved: 0, count: 0 },
            VecOperand::Words { d_ptr, count } => BlzVecArg { d_ptr, buf: 0, reserved: 0, count },
        }
    }
}
