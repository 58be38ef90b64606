// The group laws of the MSM tail as policies: the tail's algorithms (msm_impl.hip.hpp: reduce_segment, horner_walk) are
// written once over "a law", and a kernel picks the law it runs on.  A law says who holds a point and who adds:
//   lane  one lane holds the point and runs the whole formula        (ec.hip.hpp on 32-bit limbs, ec_rr.hip.hpp on the reduced radix)
//   quad  the 4 lanes of a DPP quad hold the same point, a product each  (ec_quad.hip.hpp, both radices)
//   row   the wave holds one point, a limb per lane, a product per DPP row  (ec_row.hip.hpp)
// Every law has: Pt; LANES, the lanes that share a point; a constructor from the lane's index inside that group; inf, load,
// add, dbl, store; owner(), the lanes that store (every lane of the row law stores: its own limb).  All lanes of a group run
// every call with the same arguments.  The cooperative laws also have to_lane: the point as ONE lane holds it, for emit_result.
// settle: called behind the last of a run of doublings, before the point is used - a law may put a test off until then (the row
// law's for a point of order two, ec_row.hip.hpp rowpt_dbl); a lone dbl is followed by it too.
// TAG (lane laws): a kernel's own out-of-line copy of the doubling, so that its register budget stays its own (see the NOTE
// above k_accumulate).
#pragma once
#include "ec.hip.hpp"
#include "ec_rr.hip.hpp"
#include "ec_quad.hip.hpp"
#include "ec_row.hip.hpp"
#include <type_traits>

namespace blz {

template <class F>
BLZ_DEV void load_xyzz(XYZZ<F>& a, const uint32_t* base, size_t idx) {
    const uint32_t* q = base + idx * 4 * F::N;
    fp_load(a.x, q);
    fp_load(a.y, q + F::N);
    fp_load(a.zz, q + 2 * F::N);
    fp_load(a.zzz, q + 3 * F::N);
}
template <class F>
BLZ_DEV void store_xyzz(uint32_t* base, size_t idx, const XYZZ<F>& a) {
    uint32_t* q = base + idx * 4 * F::N;
    fp_store(q, a.x);
    fp_store(q + F::N, a.y);
    fp_store(q + 2 * F::N, a.zz);
    fp_store(q + 3 * F::N, a.zzz);
}

// what every law on XYZZ<F> / XYZZRR<Q> shares: the point in memory
template <class F>
struct PointIo32 {
    using Pt = XYZZ<F>;
    BLZ_DEV void inf(Pt& p) const { pt_set_inf(p); }
    BLZ_DEV void load(Pt& p, const uint32_t* base, size_t idx) const { load_xyzz(p, base, idx); }
    BLZ_DEV void store(uint32_t* base, size_t idx, const Pt& p) const { store_xyzz(base, idx, p); }
};
template <class Q>
struct PointIoRR {
    using Pt = XYZZRR<Q>;
    BLZ_DEV void inf(Pt& p) const { ptrr_set_inf(p); }
    BLZ_DEV void load(Pt& p, const uint32_t* base, size_t idx) const { ptrr_load(p, base, idx); }
    BLZ_DEV void store(uint32_t* base, size_t idx, const Pt& p) const { ptrr_store(base, idx, p); }
};

template <class F, int TAG>
struct LaneLaw32 : PointIo32<F> {
    using Pt = XYZZ<F>;
    static constexpr uint32_t LANES = 1;
    BLZ_DEV explicit LaneLaw32(uint32_t) {}
    BLZ_DEV void add(Pt& a, const Pt& b) const { pt_add_inl<F, TAG>(a, b); }
    BLZ_DEV void dbl(Pt& a) const { a = pt_dbl_val<F, TAG>(a); }
    BLZ_DEV void settle(Pt&) const {}
    BLZ_DEV bool owner() const { return true; }
};
template <class Q, int TAG>
struct LaneLawRR : PointIoRR<Q> {
    using Pt = XYZZRR<Q>;
    static constexpr uint32_t LANES = 1;
    BLZ_DEV explicit LaneLawRR(uint32_t) {}
    BLZ_DEV void add(Pt& a, const Pt& b) const { ptrr_add<Q, TAG>(a, b); }
    BLZ_DEV void dbl(Pt& a) const { a = ptrr_dbl_val<Q, TAG>(a); }
    BLZ_DEV void settle(Pt&) const {}
    BLZ_DEV bool owner() const { return true; }
};
// the field's lane law: the reduced radix where it has one (and the tag of the kernel's copy on either)
template <class F, int TAG32, int TAGRR>
using LaneLaw = std::conditional_t<USE_RR<F>, LaneLawRR<typename F::RR, TAGRR>, LaneLaw32<F, TAG32>>;

// (ql & 3u at the calls: quad_add / quad_dbl on 32-bit limbs are out of line, and the compiler specialises them for a lane index
// below 4 only where it sees that range at the call itself - through the member it compiled them, and k_finish, otherwise)
template <class F>
struct QuadLaw32 : PointIo32<F> {
    using Pt = XYZZ<F>;
    static constexpr uint32_t LANES = 4;
    uint32_t ql;
    BLZ_DEV explicit QuadLaw32(uint32_t lane) : ql(lane) {}
    BLZ_DEV void add(Pt& a, const Pt& b) const { quad_add(a, b, ql & 3u); }
    BLZ_DEV void dbl(Pt& a) const { quad_dbl(a, ql & 3u); }
    BLZ_DEV void settle(Pt&) const {}
    BLZ_DEV bool owner() const { return ql == 0; }
    BLZ_DEV Pt to_lane(const Pt& p) const { return p; }
};
template <class Q>
struct QuadLawRR : PointIoRR<Q> {
    using Pt = XYZZRR<Q>;
    static constexpr uint32_t LANES = 4;
    uint32_t ql;
    BLZ_DEV explicit QuadLawRR(uint32_t lane) : ql(lane) {}
    BLZ_DEV void add(Pt& a, const Pt& b) const { quadrr_add(a, b, ql & 3u); }
    BLZ_DEV void dbl(Pt& a) const { quadrr_dbl(a, ql & 3u); }
    BLZ_DEV void settle(Pt&) const {}
    BLZ_DEV bool owner() const { return ql == 0; }
    BLZ_DEV Pt to_lane(const Pt& p) const { return p; }
};
template <class F>
using QuadLaw = std::conditional_t<USE_RR<F>, QuadLawRR<typename F::RR>, QuadLaw32<F>>;

// Sums leave the row law weakly normalised (store: read back by this law only) or in the accumulator form every law reads
// (store_strict).
template <class Q>
struct RowLaw {
    using Pt = RowPt;
    static constexpr uint32_t LANES = 64;
    const RowCtx<Q> c;
    BLZ_DEV explicit RowLaw(uint32_t) : c(row_ctx<Q>()) {}   // (row_ctx reads the lane's place in its wave itself)
    BLZ_DEV void inf(Pt& p) const { rowpt_set_inf(p); }
    BLZ_DEV void load(Pt& p, const uint32_t* base, size_t idx) const { rowpt_load<Q>(c, p, base, idx); }
    BLZ_DEV void add(Pt& a, const Pt& b) const { rowpt_add<Q>(c, a, b); }
    BLZ_DEV void dbl(Pt& a) const { rowpt_dbl<Q, false>(c, a); }   // (a link of a run that settle() ends: ec_row.hip.hpp)
    BLZ_DEV void settle(Pt& a) const {
        if constexpr (RR_EVEN_ORDER<Q>) rowpt_settle<Q>(c, a);
    }
    BLZ_DEV void store(uint32_t* base, size_t idx, const Pt& p) const { rowpt_store<Q>(c, base, idx, p); }
    BLZ_DEV void store_strict(uint32_t* base, size_t idx, const Pt& p) const { rowpt_store_strict<Q>(c, base, idx, p); }
    BLZ_DEV bool owner() const { return true; }
    BLZ_DEV XYZZRR<Q> to_lane(const Pt& p) const {   // (a block-wide barrier inside: one wave per block)
        __shared__ uint32_t sh[4][16];
        XYZZRR<Q> r;
        rowpt_export<Q>(c, p, sh, r);
        return r;
    }
};

// a lane's point on 32-bit limbs
template <class F>
BLZ_DEV void to_xyzz32(XYZZ<F>& o, const XYZZ<F>& p) { o = p; }
template <class F, class Q>
BLZ_DEV void to_xyzz32(XYZZ<F>& o, const XYZZRR<Q>& p) { ptrr_to_xyzz32<F>(o, p); }

// One round of the pairwise tree over the lanes of a wave: lane i holds a point (infinity from lane cnt on), round r = 1, 2, 4 ...
// adds lane i + r's to it (operands moved between lanes with ds_bpermute: 56 dwords per round, nothing against an addition);
// after the rounds below cnt the sum is in lane 0, log2(cnt) additions' worth of time later.
template <class Q, int TAG>
BLZ_DEV void ptrr_shuffle_round(XYZZRR<Q>& acc, uint32_t lane, uint32_t r, uint32_t cnt) {
    XYZZRR<Q> o;
#pragma unroll
    for (int i = 0; i < Q::NL; ++i) {
        o.x.v[i] = __shfl_down(acc.x.v[i], r, 64);
        o.y.v[i] = __shfl_down(acc.y.v[i], r, 64);
        o.zz.v[i] = __shfl_down(acc.zz.v[i], r, 64);
        o.zzz.v[i] = __shfl_down(acc.zzz.v[i], r, 64);
    }
    if ((lane & (2u * r - 1u)) == 0 && lane + r < cnt) ptrr_add<Q, TAG>(acc, o);
}

}  // namespace blz
