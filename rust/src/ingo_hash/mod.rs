//! Poseidon primitive: `PoseidonClient`, its parameter and result types (`poseidon_api`) and the tree helpers (`utils`).
//! The reference's module of the same name also carries the FPGA register map (`hash_hw_code`); here the transport is
//! the C ABI, so there is nothing else to export.  include/blaze_hip.h "Poseidon" states the hash, which the reference
//! leaves to an instruction CSV that does not ship.
pub use self::poseidon_api::*;
pub use self::utils::*;

mod poseidon_api;
mod utils;
