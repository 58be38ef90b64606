//! The reference's `tests/integration_poseidon.rs`, call for call.  INSTRUCTION_PATH names a CSV written by
//! tools/poseidon_params.py (`--field BLS381 --block 9,8,57 --block 12,8,57`).
use ingo_blaze::{
    driver_client::*,
    ingo_hash::{num_of_elements_in_base_layer, Hash, PoseidonClient, PoseidonInitializeParameters, PoseidonResult, TreeMode},
};
use std::env;

fn get_instruction_path() -> String {
    env::var("INSTRUCTION_PATH").expect("INSTRUCTION_PATH must be set.")
}

const TREE_HEIGHT_4_NUM_OF_NODES: usize = 585;
/// TEST_SCALAR of the reference, 15338226384362629345253584946022322145063321004547266825580649561525819500264, little-endian
const TEST_SCALAR_LE: [u8; 32] = [
    0xe8, 0x66, 0x6b, 0xd8, 0x25, 0x22, 0x7b, 0x74, 0x34, 0x08, 0xaa, 0x30, 0x2a, 0x41, 0xe5, 0x5b,
    0x49, 0x8a, 0x32, 0x65, 0xe7, 0x44, 0xaf, 0x14, 0x47, 0x06, 0x84, 0x74, 0xe4, 0x20, 0xe9, 0x21,
];
const ZERO: u32 = 0;
const ONE: u32 = 1;

#[test]
fn test_sanity_check() {
    let id = env::var("ID").unwrap_or_else(|_| 0.to_string());
    let poseidon = PoseidonClient::new(Hash::Poseidon, DriverClient::new(&id, DriverConfig::driver_client_cfg(CardType::C1100)));
    let params = poseidon.loaded_binary_parameters();
    assert_eq!(params.len(), 2);
    poseidon
        .initialize(PoseidonInitializeParameters { tree_height: 8, tree_mode: TreeMode::TreeC, instruction_path: get_instruction_path() })
        .unwrap();
    poseidon.set_data(&ZERO.to_le_bytes()).unwrap();
    let f = poseidon.get_last_element_sent_to_ring().unwrap();
    poseidon.set_data(&ONE.to_le_bytes()).unwrap();
    let n = poseidon.get_last_element_sent_to_ring().unwrap();
    assert_ne!(f, n);
    assert_eq!(n, f + 1);
}

#[test]
fn test_build_small_tree() {
    let id = env::var("ID").unwrap_or_else(|_| 0.to_string());
    let poseidon = PoseidonClient::new(Hash::Poseidon, DriverClient::new(&id, DriverConfig::driver_client_cfg(CardType::C1100)));
    let params = PoseidonInitializeParameters { tree_height: 4, tree_mode: TreeMode::TreeC, instruction_path: get_instruction_path() };
    let nof_elements = num_of_elements_in_base_layer(params.tree_height);
    poseidon.log_api_values();
    poseidon.initialize(params).unwrap();
    poseidon.log_api_values();
    poseidon.loaded_binary_parameters();
    for _ in 0..nof_elements {
        for _ in 0..11 {
            poseidon.set_data(&TEST_SCALAR_LE).unwrap();
        }
    }
    let result: Vec<PoseidonResult> = poseidon.result(Some(TREE_HEIGHT_4_NUM_OF_NODES)).unwrap().unwrap();
    poseidon.log_api_values();
    assert_eq!(result.len(), TREE_HEIGHT_4_NUM_OF_NODES);
    // every node exactly once, the root last of its layer's own
    let mut seen = std::collections::HashSet::new();
    for r in result.iter() {
        assert!(seen.insert((r.layer_id, r.hash_id)));
    }
    assert!(seen.contains(&(3, 0)));
}

#[test]
fn test_build_small_tree_polling() {
    let id = env::var("ID").unwrap_or_else(|_| 0.to_string());
    let poseidon = PoseidonClient::new(Hash::Poseidon, DriverClient::new(&id, DriverConfig::driver_client_cfg(CardType::C1100)));
    let params = PoseidonInitializeParameters { tree_height: 4, tree_mode: TreeMode::TreeC, instruction_path: get_instruction_path() };
    let nof_elements = num_of_elements_in_base_layer(params.tree_height);
    poseidon.initialize(params).unwrap();
    let mut results: Vec<PoseidonResult> = vec![];
    for _ in 0..nof_elements * 11 {
        poseidon.set_data(&TEST_SCALAR_LE).unwrap();
        let pending = poseidon.get_num_of_pending_results().unwrap();
        let res = poseidon.get_raw_results(pending).unwrap();
        results.append(&mut PoseidonResult::parse_poseidon_hash_results(res));
    }
    assert_eq!(results.len(), TREE_HEIGHT_4_NUM_OF_NODES);
}
