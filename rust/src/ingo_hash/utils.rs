//! Tree helpers of the reference's `ingo_hash::utils`.
pub fn num_of_elements_oct_tree(tree_height: u32) -> u32 {
    (0..tree_height).map(|i| 8u32.pow(tree_height - i - 1)).sum()
}

pub fn num_of_elements_in_base_layer(tree_height: u32) -> u32 {
    8u32.pow(tree_height - 1)
}

#[repr(u8)]
#[derive(PartialEq, Eq, Copy, Clone)]
pub enum TreeMode {
    TreeC,
    TreeD,
}

impl TreeMode {
    /// The tree's start layer (enum blz_tree_mode): TreeC 0, TreeD 1.
    pub fn value(tree_mode: TreeMode) -> u32 {
        match tree_mode {
            TreeMode::TreeC => 0,
            TreeMode::TreeD => 1,
        }
    }
}
