// Poseidon kernels over the scalar field of BLS377 (one translation unit per field).
#include "poseidon_impl.hip.hpp"

namespace blz {
const PoseidonFieldOps& poseidon_ops_bls377() {
    static const PoseidonFieldOps ops = make_poseidon_ops<Fr_BLS377>();
    return ops;
}
}  // namespace blz
