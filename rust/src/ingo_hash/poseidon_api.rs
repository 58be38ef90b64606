//! `PoseidonClient` of the reference's `ingo_hash::poseidon_api` over libblaze_hip: the same call sequence, element
//! FIFO, tree shape and 64-byte result record.  The hash itself is the caller's: the instruction CSV carries the
//! Poseidon instance (include/blaze_hip.h "THE INSTRUCTION STREAM"; tools/poseidon_params.py writes one).
use std::ffi::CString;

use super::TreeMode;
use crate::{
    driver_client::{hip_ffi::*, *},
    error::*,
};

pub enum Hash {
    Poseidon,
}

pub struct PoseidonClient {
    pub dclient: DriverClient,
    h: *mut BlzPoseidon,
}
unsafe impl Send for PoseidonClient {}

#[derive(Clone)]
pub struct PoseidonInitializeParameters {
    pub tree_height: u32,
    pub tree_mode: TreeMode,
    pub instruction_path: String,
}

pub struct PoseidonResult {
    pub hash_byte: [u8; 32],
    pub hash_id: u32,
    pub layer_id: u32,
}

impl PoseidonResult {
    /// 64 bytes per result: the digest, then a 256-bit little-endian word with `hash_id` in bits 0-29 and `layer_id`
    /// in bits 30-39 (the reference reads the latter through an overlapping two-byte window: bytes 3..5, `>> 6`).
    pub fn parse_poseidon_hash_results(data: Vec<u8>) -> Vec<PoseidonResult> {
        let mut results: Vec<PoseidonResult> = Vec::new();
        for element in data.chunks(64) {
            assert_eq!(element.len(), 64);
            let hash: [u8; 32] = element[0..32].try_into().unwrap();
            let hash_data: [u8; 32] = element[32..].try_into().unwrap();
            let hash_first_4_bytes: [u8; 4] = hash_data[..4].try_into().unwrap();
            let mut hash_last_2_bytes: [u8; 4] = [0; 4];
            hash_last_2_bytes[..2].copy_from_slice(&hash_data[3..5]);
            results.push(PoseidonResult {
                hash_byte: hash,
                hash_id: u32::from_le_bytes(hash_first_4_bytes) & 0x3fffffff,
                layer_id: u32::from_le_bytes(hash_last_2_bytes) >> 6,
            });
        }
        results
    }
}

impl DriverPrimitive<Hash, PoseidonInitializeParameters, &[u8], Vec<PoseidonResult>> for PoseidonClient {
    /// BLS12-381 Fr, the field of the reference's TEST_SCALAR; `with_field` for the others.
    fn new(_ptype: Hash, dclient: DriverClient) -> Self {
        PoseidonClient::with_field(dclient, 1)
    }

    fn loaded_binary_parameters(&self) -> Vec<u32> {
        let mut v = [0u32; 2];
        check(unsafe { blz_poseidon_loaded_binary_parameters(self.h, v.as_mut_ptr()) }).unwrap();
        v.to_vec()
    }

    /// reset, load the instruction set, height, start layer
    fn initialize(&self, param: PoseidonInitializeParameters) -> Result<()> {
        let path = CString::new(param.instruction_path.clone()).map_err(|_| DriverClientError::LoadFailed { path: param.instruction_path.clone() })?;
        check(unsafe { blz_poseidon_initialize(self.h, param.tree_height, TreeMode::value(param.tree_mode) as i32, path.as_ptr()) })
    }

    /// `todo!()` in the reference too
    fn start_process(&self, _param: Option<usize>) -> Result<()> {
        todo!()
    }

    /// elements into the FIFO: 32 bytes each, or ONE element of fewer than 32 bytes (zero-extended)
    fn set_data(&self, input: &[u8]) -> Result<()> {
        check(unsafe { blz_poseidon_set_data(self.h, input.as_ptr(), input.len()) })
    }

    /// `todo!()` in the reference; here: every node whose inputs have arrived is hashed when it returns (bounded)
    fn wait_result(&self) -> Result<()> {
        check(unsafe { blz_poseidon_wait_result(self.h) })
    }

    /// Up to `expected_result` records; bounded where the reference polls for ever.
    fn result(&self, expected_result: Option<usize>) -> Result<Option<Vec<PoseidonResult>>> {
        let expected = expected_result.unwrap();
        let mut res = vec![0u8; 64 * expected];
        let mut n = 0u32;
        check(unsafe { blz_poseidon_result(self.h, expected as u32, res.as_mut_ptr(), res.len(), &mut n) })?;
        res.truncate(64 * n as usize);
        Ok(Some(PoseidonResult::parse_poseidon_hash_results(res)))
    }
}

impl Drop for PoseidonClient {
    fn drop(&mut self) {
        unsafe { blz_poseidon_free(self.h) }
    }
}

impl PoseidonClient {
    /// `field` = a `Curve` as i32: the hash runs over that curve's scalar field.
    pub fn with_field(dclient: DriverClient, field: i32) -> Self {
        let mut h: *mut BlzPoseidon = std::ptr::null_mut();
        check(unsafe { blz_poseidon_new(dclient.id, field, &mut h) }).expect("blz_poseidon_new failed");
        PoseidonClient { dclient, h }
    }

    fn counters(&self) -> Result<[u32; 4]> {
        let mut v = [0u32; 4];
        check(unsafe { blz_poseidon_counters(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }

    pub fn get_last_element_sent_to_ring(&self) -> Result<u32> {
        Ok(self.counters()?[0])
    }

    pub fn get_num_of_pending_results(&self) -> Result<u32> {
        let mut v = 0u32;
        check(unsafe { blz_poseidon_num_pending_results(self.h, &mut v) })?;
        Ok(v)
    }

    pub fn get_raw_results(&self, num_of_results: u32) -> Result<Vec<u8>> {
        let mut res = vec![0u8; 64 * num_of_results as usize];
        check(unsafe { blz_poseidon_raw_results(self.h, num_of_results, res.as_mut_ptr(), res.len()) })?;
        Ok(res)
    }

    pub fn get_last_hash_sent_to_host(&self) -> Result<u32> {
        Ok(self.counters()?[1])
    }

    pub fn log_api_values(&self) {
        log::debug!("=== api values ===");
        log::debug!("{:?} pending {:?}", self.counters().unwrap(), self.get_num_of_pending_results().unwrap());
        log::debug!("=== api values ===");
    }

    /// initialize with the instruction word stream from memory (32-byte little-endian words)
    pub fn initialize_words(&self, tree_height: u32, tree_mode: TreeMode, words: &[u8]) -> Result<()> {
        check(unsafe { blz_poseidon_initialize_words(self.h, tree_height, TreeMode::value(tree_mode) as i32, words.as_ptr(), words.len()) })
    }

    /// The load-time checks alone (host side): `[blocks, width mask, 0 (reserved: see prepare_round_plan), words consumed]`.
    pub fn check_words(field: i32, tree_mode: TreeMode, words: &[u8]) -> Result<[u32; 4]> {
        let mut v = [0u32; 4];
        check(unsafe { blz_poseidon_check_words(field, TreeMode::value(tree_mode) as i32, words.as_ptr(), words.len(), v.as_mut_ptr()) })?;
        Ok(v)
    }

    /// `[device bytes held, optimised partial rounds in force, state of their self-check, width mask]`
    pub fn info(&self) -> Result<[u64; 4]> {
        let mut v = [0u64; 4];
        check(unsafe { blz_poseidon_info(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }

    pub fn set_round_plan(&self, enable: bool) -> Result<()> {
        check(unsafe { blz_poseidon_set_round_plan(self.h, enable as i32) })
    }

    /// Derive and self-check the optimised partial rounds now instead of under the first tree:
    /// `[in force, self-check state (0 not run, 1 equal, 2 refused: dense rounds)]`.
    pub fn prepare_round_plan(&self) -> Result<[u32; 2]> {
        let mut v = [0u32; 2];
        check(unsafe { blz_poseidon_prepare_round_plan(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }

    pub fn last_kernel_ms(&self) -> Result<f32> {
        let mut v = 0f32;
        check(unsafe { blz_poseidon_last_kernel_ms(self.h, &mut v) })?;
        Ok(v)
    }

    pub fn reset_engine(&self) -> Result<()> {
        check(unsafe { blz_poseidon_reset(self.h) })
    }
}

pub struct PoseidonImageParametrs {
    pub hif2_cpu_c_is_stub: u8,
    pub hif2_cpu_c_number_of_cores: u8,
    pub hif2_cpu_c_place_holder: u32,
}

impl ParametersAPI for PoseidonImageParametrs {
    /// The reference unpacks `params.to_be_bytes()` with msb0 bit ranges 28..=31, 20..=27, 0..=19.
    fn parse_image_params(params: u32) -> PoseidonImageParametrs {
        PoseidonImageParametrs {
            hif2_cpu_c_is_stub: (params & 0xf) as u8,
            hif2_cpu_c_number_of_cores: ((params >> 4) & 0xff) as u8,
            hif2_cpu_c_place_holder: params >> 12,
        }
    }

    fn debug_information(&self) {
        log::debug!("Is Stub: {:?}", self.hif2_cpu_c_is_stub);
        log::debug!("Number of Cores: {:?}", self.hif2_cpu_c_number_of_cores);
        log::debug!("Place Holder: {:?}", self.hif2_cpu_c_place_holder);
    }
}
