// Poseidon kernels over the scalar field of BN254 (one translation unit per field).
#include "poseidon_impl.hip.hpp"

namespace blz {
const PoseidonFieldOps& poseidon_ops_bn254() {
    static const PoseidonFieldOps ops = make_poseidon_ops<Fr_BN254>();
    return ops;
}
}  // namespace blz
