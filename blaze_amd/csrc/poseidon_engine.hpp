// Poseidon over a scalar field: what the host code (poseidon.hip) and the per-field kernel units (poseidon_<field>.hip,
// poseidon_impl.hip.hpp) share.  include/blaze_hip.h "Poseidon" states the hash; DESIGN.md section 8 the kernel.
#pragma once
#include "common.hpp"

namespace blz {

constexpr int POS_T_MIN = 2, POS_T_MAX = 16;   // widths a parameter stream may carry
constexpr int POS_SD = 12;                     // dwords between two elements of a constant table / of the LDS state: 9 limbs, 16-byte aligned
constexpr int POS_ROUNDS_MAX = 1024;           // R_F + R_P of one block (a bound on what load accepts, not a tuning figure)

// One width's constants on the device: reduced-radix Montgomery form (x 2^261 mod r), canonical, POS_SD dwords apart.
struct PoseidonWidth {
    int t = 0, rf = 0, rp = 0;
    const uint32_t* tag = nullptr;   // 1 element: state[0] of the fixed-arity hash
    const uint32_t* rc = nullptr;    // t (rf + rp) elements, round order
    const uint32_t* mds = nullptr;   // t t elements, row-major: copied to LDS as it stands
};

// n hashes of arity t - 1: hash j reads the 32-byte words in[(t - 1) j ...], writes its digest (32 bytes, canonical) to
// dig[8 j ...] and - rec != nullptr - its 64-byte record with hash_id = id0 + j and the layer to rec[16 j ...].
struct PoseidonJob {
    const uint32_t* in = nullptr;
    uint32_t* dig = nullptr;
    uint32_t* rec = nullptr;
    uint64_t n = 0;
    uint64_t id0 = 0;
    uint32_t layer = 0;
};

// The optimised partial rounds of one width, derived on the device from the block's words; same element
// format as PoseidonWidth.  Partial round k = 0 .. rp - 1: lane e reads sp[(2 k) t + e] (row 0 of the sparse matrix: v^T Mh^-j, slot 0
// unused) and sp[(2 k + 1) t + e] (its column 0: m00, then Mh^(j-1) w), and the constant prc[k t + e].
struct HadesPlan {
    const uint32_t* sp = nullptr;    // 2 t rp elements
    const uint32_t* prc = nullptr;   // t rp elements: diag(1, Mh^j) c_k
    const uint32_t* pre = nullptr;   // t t elements, row-major: diag(1, Mh^rp) M, the matrix of the last full round of the first half
};
inline size_t hades_plan_elements(int t, int rp) { return (size_t)3 * t * rp + (size_t)t * t; }
constexpr uint32_t HADES_OK = 1, HADES_REFUSED = 2;   // blz_poseidon_info word 2

struct PoseidonFieldOps {
    uint32_t modulus[8];   // r, 32-bit words, little-endian
    // canonical 32-byte words -> the device form above (n elements, out: n * POS_SD dwords)
    int (*prep)(hipStream_t st, const uint32_t* d_words, uint32_t* d_out, uint32_t n);
    // the product path: one launch for the whole job
    int (*hash)(hipStream_t st, const PoseidonWidth& w, const PoseidonJob& job);
    // d_block: the block's canonical words on the device, from its tag on (tag | round constants | matrix).  Fills the plan's tables
    // and *d_status = HADES_OK, or *d_status = HADES_REFUSED when the matrix without row 0 and column 0 has no inverse
    int (*derive)(hipStream_t st, const uint32_t* d_block, int t, int rf, int rp, uint32_t* d_tables, uint32_t* d_status);
    // the same job through the optimised partial rounds
    int (*hash_plan)(hipStream_t st, const PoseidonWidth& w, const HadesPlan& pl, const PoseidonJob& job);
};
// where derive() put width t's tables inside d_tables
inline HadesPlan hades_plan_at(const uint32_t* d_tables, int t, int rp) {
    HadesPlan pl;
    pl.sp = d_tables;
    pl.prc = pl.sp + (size_t)2 * t * rp * POS_SD;
    pl.pre = pl.prc + (size_t)t * rp * POS_SD;
    return pl;
}
const PoseidonFieldOps& poseidon_ops_bls377();
const PoseidonFieldOps& poseidon_ops_bls381();
const PoseidonFieldOps& poseidon_ops_bn254();
const PoseidonFieldOps* poseidon_ops_for(int field);

// The word stream of blz_poseidon_initialize (include/blaze_hip.h), parsed and checked on the host.
struct PoseidonBlock {
    int t = 0, rf = 0, rp = 0;
    size_t tag = 0, rc = 0, mds = 0;   // word indices into the stream
};
struct PoseidonStream {
    std::vector<PoseidonBlock> blocks;
    uint32_t width_mask = 0;
    size_t consumed = 0;               // words, the zero pad not counted
};
// the widths a tree mode hashes with: TreeC 12 (base nodes, 11 elements) and 9 (arity 8), TreeD 9
inline uint32_t poseidon_need_mask(int tree_mode) { return tree_mode == BLZ_TREE_C ? ((1u << 9) | (1u << 12)) : (1u << 9); }
// BLZ_OK or BLZ_ERR_LOAD_FAILED with the reason as the error message; need_mask: bit t set = a block of width t must be there
int poseidon_parse(int field, uint32_t need_mask, const uint8_t* words, size_t len, PoseidonStream& out);
// upload the stream's words (waited for), convert them on `st` into `consts`, point w[t] at each block's tables; the caller waits for `st`
int poseidon_upload(const PoseidonFieldOps* ops, hipStream_t st, const PoseidonStream& ps, const uint8_t* words, DevBuf& raw, DevBuf& consts,
                    PoseidonWidth (&w)[POS_T_MAX + 1]);

}  // namespace blz
