// Poseidon kernels over the scalar field of BLS381 (one translation unit per field).
#include "poseidon_impl.hip.hpp"

namespace blz {
const PoseidonFieldOps& poseidon_ops_bls381() {
    static const PoseidonFieldOps ops = make_poseidon_ops<Fr_BLS381>();
    return ops;
}
}  // namespace blz
