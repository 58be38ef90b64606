// C++17 host-side mirror of the reference's operator surface above the C ABI (include/blaze_hip.h).
// Same names, argument meaning and call order as the Rust crate:
//   src/driver_client/dclient.rs:28-46   trait DriverPrimitive<T,P,I,O>
//   src/ingo_msm/msm_api.rs:8-331        MSMClient, MSMInit, MSMParams, MSMInput, MSMResult
//   src/ingo_ntt/ntt_api.rs:8-125        NTTClient, NTT, NttInit, NTTInput
//   src/ingo_hash/poseidon_api.rs:11-278 PoseidonClient, Hash, TreeMode, PoseidonInitializeParameters, PoseidonResult
//   src/error.rs:6-32                    DriverClientError
// Header-only; link with -lblaze_hip.  Errors are thrown as DriverClientError (the reference returns
// Result<_, DriverClientError>; its panics on bad mode combinations become InvalidPrimitiveParam).
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "blaze_hip.h"

namespace ingo_blaze {

struct DriverClientError : std::runtime_error {
    enum Kind { WriteError = 1, ReadError, HBICAPNotReady, InvalidPrimitiveParam, CsvError, LoadFailed, FileError, Unknown };
    Kind kind;
    DriverClientError(int code, const std::string& msg)
        : std::runtime_error(msg), kind(code >= 1 && code <= 8 ? static_cast<Kind>(code) : Unknown) {}
};
inline void check(int rc) {
    if (rc != BLZ_OK) throw DriverClientError(rc, blz_last_error_message());
}

enum class CardType { C1100, MI355X };  // dclient_cfg.rs:1-3 (+ this build's card)
struct DriverConfig {                   // dclient_cfg.rs:9-31: AXI base addresses have no GPU meaning
    CardType card = CardType::MI355X;
    static DriverConfig driver_client_cfg(CardType c) { return DriverConfig{c}; }
};

// dclient.rs:50-93: `id` is the slot id of /dev/xdma{id}_*; here the HIP device ordinal.
class DriverClient {
   public:
    int id;
    DriverConfig cfg;
    DriverClient(int id_, DriverConfig cfg_ = {}) : id(id_), cfg(cfg_) {
        if (id < 0 || id >= blz_device_count()) throw DriverClientError(BLZ_ERR_FILE, "no HIP device with this ordinal");
    }
    void reset() const {}  // DFX decouple toggle + sleep(100 ms) on the card (dclient.rs:88-93): nothing to do
};

// dclient.rs:28-46
template <class T, class P, class I, class O>
class DriverPrimitive {
   public:
    virtual ~DriverPrimitive() = default;
    virtual std::vector<uint32_t> loaded_binary_parameters() const = 0;
    virtual void initialize(const P& param) = 0;
    virtual void set_data(const I& input) = 0;
    virtual void start_process(std::optional<size_t> param = std::nullopt) = 0;
    virtual void wait_result() = 0;
    virtual std::optional<O> result(std::optional<size_t> param = std::nullopt) = 0;
};

// ---------------------------------------------------------------- MSM (src/ingo_msm)
enum class Curve { BLS377 = 0, BLS381 = 1, BN254 = 2 };   // msm_cfg.rs:4-8
enum class PointMemoryType { HBM = 0, DMA = 1 };          // msm_cfg.rs:11-14
constexpr uint32_t PRECOMPUTE_FACTOR_BASE = 1, PRECOMPUTE_FACTOR = 8;  // msm_api.rs:39-40

struct MSMInit { PointMemoryType mem_type; bool is_precompute; Curve curve; };                       // msm_api.rs:16-20
struct MSMParams { uint32_t nof_elements; std::optional<std::pair<uint64_t, uint64_t>> hbm_point_addr; };  // :23-26
struct MSMInput { std::optional<std::vector<uint8_t>> points; std::vector<uint8_t> scalars; MSMParams params; };  // :28-32
struct MSMResult { std::vector<uint8_t> result; uint32_t result_label; };                           // :33-37

class MSMClient : public DriverPrimitive<MSMInit, MSMParams, MSMInput, MSMResult> {
    blz_msm* h_ = nullptr;
    size_t result_size_;

   public:
    DriverClient driver_client;
    MSMClient(const MSMInit& init, DriverClient dclient) : driver_client(dclient) {  // msm_api.rs:44-55
        check(blz_msm_new(dclient.id, static_cast<int>(init.mem_type), init.is_precompute, static_cast<int>(init.curve), &h_));
        result_size_ = blz_result_size(static_cast<int>(init.curve));
    }
    ~MSMClient() override { blz_msm_free(h_); }
    MSMClient(const MSMClient&) = delete;
    MSMClient& operator=(const MSMClient&) = delete;

    std::vector<uint32_t> loaded_binary_parameters() const override {  // msm_api.rs:57-70
        uint32_t v[2];
        check(blz_msm_loaded_binary_parameters(h_, v));
        return {v[0], v[1]};
    }
    void initialize(const MSMParams& p) override {  // msm_api.rs:72-111
        auto a = p.hbm_point_addr.value_or(std::make_pair<uint64_t, uint64_t>(0, 0));
        check(blz_msm_initialize(h_, p.nof_elements, p.hbm_point_addr.has_value(), a.first, a.second));
    }
    void start_process(std::optional<size_t> = std::nullopt) override { check(blz_msm_start_process(h_)); }  // :113-120
    void set_data(const MSMInput& d) override {  // msm_api.rs:155-220
        auto a = d.params.hbm_point_addr.value_or(std::make_pair<uint64_t, uint64_t>(0, 0));
        check(blz_msm_set_data(h_, d.points ? d.points->data() : nullptr, d.points ? d.points->size() : 0, d.scalars.data(),
                               d.scalars.size(), d.params.nof_elements, d.params.hbm_point_addr.has_value(), a.first, a.second));
    }
    void wait_result() override { check(blz_msm_wait_result(h_)); }  // msm_api.rs:222-238
    std::optional<MSMResult> result(std::optional<size_t> = std::nullopt) override {  // msm_api.rs:240-274
        MSMResult r;
        r.result.resize(result_size_);
        size_t n = 0;
        check(blz_msm_result(h_, r.result.data(), r.result.size(), &n, &r.result_label));
        r.result.resize(n);
        return r;
    }
    // msm_api.rs:277-331
    uint32_t task_label() const { uint32_t v; check(blz_msm_task_label(h_, &v)); return v; }
    uint32_t nof_elements() const { uint32_t v; check(blz_msm_nof_elements(h_, &v)); return v; }
    uint32_t is_msm_engine_ready() const { uint32_t v; check(blz_msm_is_engine_ready(h_, &v)); return v; }
    // a task fed by several set_data calls (blaze_hip.h "STREAMED TASKS"): {elements received, elements of the queued task}
    std::pair<uint32_t, uint32_t> stream_progress() const { uint32_t v[2]; check(blz_msm_stream_progress(h_, v)); return {v[0], v[1]}; }
    void load_data_to_hbm(const std::vector<uint8_t>& points, uint64_t addr, uint64_t offset) {
        check(blz_msm_load_data_to_hbm(h_, points.data(), points.size(), addr, offset));
    }
    std::vector<uint8_t> get_data_from_hbm(size_t data_len, uint64_t addr, uint64_t offset) {
        std::vector<uint8_t> out(data_len);
        check(blz_msm_get_data_from_hbm(h_, out.data(), data_len, addr, offset));
        return out;
    }
    // multi-GPU (no reference counterpart: README.md:20-22 leaves it to a "management layer"): one communicator
    // rank per client; comm_unique_id() on rank 0, shipped to the others by the host
    static std::vector<uint8_t> comm_unique_id() {
        std::vector<uint8_t> id(BLZ_COMM_ID_BYTES);
        check(blz_comm_unique_id(id.data()));
        return id;
    }
    // resident-base window table (blaze_hip.h): opt-in, bases in the arena, precompute_factor 1
    void set_scalar_range(uint32_t bit_lo, uint32_t bit_hi) { check(blz_msm_set_scalar_range(h_, bit_lo, bit_hi)); }   // one shard of a job split by scalar chunk
    void set_window_table(int mode) { check(blz_msm_set_window_table(h_, mode)); }   // 0 off, 1 where it pays, 2 always
    // checked-table plan of a precompute client (blaze_hip.h blz_msm_set_precompute_plan): resident x8 tables are checked once per
    // load against precompute_base_* and, if consistent, served as 4n even bases with 64-bit chunks; identical result bytes
    void set_precompute_plan(bool enable) { check(blz_msm_set_precompute_plan(h_, enable ? 1 : 0)); }
    bool prepare_precompute_plan(uint32_t nof_elements, std::pair<uint64_t, uint64_t> hbm_addr = {0, 0}) {
        int ok = 0;
        check(blz_msm_prepare_precompute_plan(h_, nof_elements, hbm_addr.first, hbm_addr.second, &ok));
        return ok != 0;
    }
    // device bytes behind this client: {workspace, staging, arena raw, arena Montgomery copies, arena window tables, total}
    std::array<uint64_t, 6> memory_info() {
        std::array<uint64_t, 6> out{};
        check(blz_msm_memory_info(h_, out.data()));
        return out;
    }
    // {took the plan, check state (0 unchecked, 1 consistent, 2 refuted), check us, even-base copy bytes} of the last HBM task
    std::array<uint64_t, 4> precompute_plan_info() {
        std::array<uint64_t, 4> out{};
        check(blz_msm_precompute_plan_info(h_, out.data()));
        return out;
    }
    // enqueue the table's build for the bases at hbm_addr (it is paced by the tasks otherwise) and wait up to wait_ms for it
    // (0: not at all, < 0: the library's wait deadline); true: the table is in place
    bool prepare_window_table(uint32_t nof_elements, std::pair<uint64_t, uint64_t> hbm_addr = {0, 0}, int wait_ms = -1) {
        int ready = 0;
        check(blz_msm_prepare_window_table(h_, nof_elements, hbm_addr.first, hbm_addr.second, wait_ms, &ready));
        return ready != 0;
    }
    // {first element, count, bit_lo, bit_hi, ranges, compute us, link us, device MiB} of `rank`: the split priced with the flow's
    // transfers (flags: BLZ_SHARD_SCALARS_FROM_HOST | BLZ_SHARD_BASES_FROM_HOST)
    static std::array<uint32_t, 8> shard_layout_ex(int curve, uint32_t nof_elements, int nranks, int rank, uint32_t flags) {
        std::array<uint32_t, 8> out{};
        check(blz_msm_shard_layout_ex(curve, nof_elements, nranks, rank, flags, out.data()));
        return out;
    }
    void comm_init(int rank, int nranks, const std::vector<uint8_t>& id) { check(blz_msm_comm_init(h_, rank, nranks, id.data())); }
    std::vector<uint8_t> all_gather_combine(const std::vector<uint8_t>& partial) {
        std::vector<uint8_t> out(result_size_);
        check(blz_msm_all_gather_combine(h_, partial.data(), out.data(), out.size()));
        return out;
    }
    // one thread driving one client per device: the group forms (the per-rank calls above are blocking rendezvous)
    static void comm_init_all(const std::vector<MSMClient*>& clients) {
        std::vector<blz_msm*> hs;
        for (MSMClient* c : clients) hs.push_back(c->h_);
        check(blz_msm_comm_init_all(hs.data(), (int)hs.size()));
    }
    static std::vector<std::vector<uint8_t>> all_gather_combine_all(const std::vector<MSMClient*>& clients,
                                                                    const std::vector<std::vector<uint8_t>>& partials) {
        std::vector<blz_msm*> hs;
        std::vector<uint8_t> flat;
        for (MSMClient* c : clients) hs.push_back(c->h_);
        for (const auto& p : partials) flat.insert(flat.end(), p.begin(), p.end());
        const size_t rs = clients.at(0)->result_size_;
        if (partials.size() != clients.size() || flat.size() != rs * clients.size()) throw DriverClientError(BLZ_ERR_INVALID_PARAM, "partials");
        std::vector<uint8_t> out(rs * clients.size());
        check(blz_msm_all_gather_combine_all(hs.data(), (int)hs.size(), flat.data(), out.data(), out.size()));
        std::vector<std::vector<uint8_t>> res;
        for (size_t i = 0; i < clients.size(); ++i) res.emplace_back(out.begin() + i * rs, out.begin() + (i + 1) * rs);
        return res;
    }
    std::vector<uint8_t> combine_partials(const std::vector<uint8_t>& partials, size_t count) {
        std::vector<uint8_t> out(result_size_);
        check(blz_msm_combine_partials(h_, partials.data(), count, out.data(), out.size()));
        return out;
    }
};

// ---------------------------------------------------------------- NTT (src/ingo_ntt)
enum class NTT { Ntt };                                             // ntt_api.rs:8-10
struct NttInit {};                                                  // ntt_api.rs:17
struct NTTInput { size_t buf_host; std::vector<uint8_t> data; };    // ntt_api.rs:19-23

class NTTClient : public DriverPrimitive<NTT, NttInit, NTTInput, std::vector<uint8_t>> {
    blz_ntt* h_ = nullptr;
    size_t nbytes_;

   public:
    DriverClient driver_client;
    // ntt_api.rs:26-31; 2^27 over BLS12-381 Fr, forward, is the reference shape.  `field` (a Curve: the
    // scalar field of that curve) and `inverse` have no reference counterpart.
    // flags: BLZ_NTT_NO_FACTOR_TABLE | BLZ_NTT_INVERSE | BLZ_NTT_BITREV_INPUT | BLZ_NTT_BITREV_OUTPUT; root: any primitive
    // 2^log_size-th root of unity (32 canonical little-endian bytes, checked on the device) instead of g^((r - 1) / 2^log_size) -
    // the transform's convention, which the reference leaves unstated (blaze_hip.h blz_ntt_new_ex3)
    NTTClient(NTT, DriverClient dclient, int log_size = 27, Curve field = Curve::BLS381, bool inverse = false, uint32_t flags = 0,
              const uint8_t* root = nullptr)
        : nbytes_(size_t(32) << log_size), driver_client(dclient) {
        check(blz_ntt_new_ex3(dclient.id, int(field), log_size, flags | (inverse ? BLZ_NTT_INVERSE : 0u), root, &h_));
    }
    ~NTTClient() override { blz_ntt_free(h_); }
    NTTClient(const NTTClient&) = delete;
    NTTClient& operator=(const NTTClient&) = delete;

    std::vector<uint32_t> loaded_binary_parameters() const override { throw std::logic_error("todo!() in the reference (ntt_api.rs:33-35)"); }
    void initialize(const NttInit&) override { check(blz_ntt_initialize(h_)); }                              // :37-56
    void set_data(const NTTInput& in) override { check(blz_ntt_set_data(h_, in.buf_host, in.data.data(), in.data.size())); }  // :72-87
    void start_process(std::optional<size_t> buf_kernel = std::nullopt) override { check(blz_ntt_start_process(h_, buf_kernel.value())); }  // :58-70
    void wait_result() override { check(blz_ntt_wait_result(h_)); }                                           // :89-108
    std::optional<std::vector<uint8_t>> result(std::optional<size_t> buf_num = std::nullopt) override {       // :110-124
        std::vector<uint8_t> out(nbytes_);
        check(blz_ntt_result(h_, buf_num.value(), out.data(), out.size()));
        return out;
    }
    // result(buf) into `out` and set_data({buf, next}) as one full-duplex call (blaze_hip.h blz_ntt_exchange): a cycle of the
    // reference's double-buffered loop (tests/integration_ntt.rs:102-136) on the buffer the kernel is not using
    void exchange(size_t buf, const std::vector<uint8_t>& next, std::vector<uint8_t>& out) {
        out.resize(nbytes_);
        check(blz_ntt_exchange(h_, buf, next.data(), next.size(), out.data(), out.size()));
    }
    // transforms started from now on run on the coset shift * <w> (blaze_hip.h blz_ntt_set_coset): shift = 32 canonical
    // little-endian bytes, 0 < shift < r; nullptr (or 1) = the plain transform again
    void set_coset(const uint8_t* shift) { check(blz_ntt_set_coset(h_, shift)); }
    std::array<uint8_t, 32> coset() {
        std::array<uint8_t, 32> v{};
        check(blz_ntt_get_coset(h_, v.data()));
        return v;
    }
    // element-wise op on the transform buffers (blaze_hip.h blz_ntt_vec_op): buffer dst = op(a, b, c), position by position;
    // enqueued like a transform - wait_result() finishes it.  Operands: buffer(i) names transform buffer i, words(p, count)
    // `count` 32-byte device words read periodically (count = 1: a scalar); nullptr for the operands the op does not take
    static blz_vec_arg buffer(uint32_t i) { return blz_vec_arg{nullptr, i, 0u, 0u}; }
    static blz_vec_arg words(const void* d_ptr, uint64_t count) { return blz_vec_arg{d_ptr, 0u, 0u, count}; }
    void vec_op(blz_vec_op op, size_t dst, const blz_vec_arg* a, const blz_vec_arg* b = nullptr, const blz_vec_arg* c = nullptr) {
        check(blz_ntt_vec_op(h_, (int)op, dst, a, b, c));
    }
    // folds along the buffer (blz_ntt_vec_reduce / blz_ntt_vec_scan), enqueued the same way.  vec_reduce: 32 bytes of device
    // memory d_out = sum a, sum a b, or sum a[p] z^p with z = the one-word operand b.  vec_scan: buffer dst = the running sum /
    // product of a (flags: BLZ_SCAN_EXCLUSIVE), d_total (nullable) = the fold of all n elements
    void vec_reduce(blz_fold_op op, const blz_vec_arg* a, const blz_vec_arg* b, void* d_out) {
        check(blz_ntt_vec_reduce(h_, (int)op, a, b, d_out));
    }
    void vec_scan(blz_scan_op op, uint32_t flags, size_t dst, const blz_vec_arg* a, void* d_total = nullptr) {
        check(blz_ntt_vec_scan(h_, (int)op, flags, dst, a, d_total));
    }
    // weighted scan (blz_ntt_vec_horner): buffer dst[p] = a[p] + z dst[p - 1] (flags: BLZ_HORNER_EXCLUSIVE | BLZ_HORNER_REVERSE), z one
    // device word, d_total (nullable) = the last inclusive value.  vec_divide: dst = the quotient of a(X) by X - z, d_rem = a(z)
    void vec_horner(uint32_t flags, size_t dst, const blz_vec_arg* a, const blz_vec_arg* z, void* d_total = nullptr) {
        check(blz_ntt_vec_horner(h_, flags, dst, a, z, d_total));
    }
    void vec_divide(size_t dst, const blz_vec_arg* a, const blz_vec_arg* z, void* d_rem = nullptr) {
        vec_horner(BLZ_HORNER_EXCLUSIVE | BLZ_HORNER_REVERSE, dst, a, z, d_rem);
    }
    // gather (blz_ntt_vec_gather): buffer dst[p] = a[(offset + stride p) mod count] for p < len, 0 above; a may hold up to 2^27
    // words, and may name dst (in place, through the handle's scratch at twice the traffic).  view(offset, stride, len) builds
    // the struct.  vec_rotate: dst[p] = a[(p + k) mod n], k of either sign, a of n words.  vec_extend: dst = the count <= n
    // device words at d_ptr, zero above
    static blz_vec_view view(uint64_t offset, uint64_t stride, uint64_t len) { return blz_vec_view{offset, stride, len}; }
    void vec_gather(size_t dst, const blz_vec_arg* a, const blz_vec_view& v) { check(blz_ntt_vec_gather(h_, dst, a, &v)); }
    void vec_rotate(size_t dst, const blz_vec_arg* a, int64_t k) {
        const int64_t n = int64_t(nbytes_ / 32);
        vec_gather(dst, a, view(uint64_t(((k % n) + n) % n), 1, uint64_t(n)));
    }
    void vec_extend(size_t dst, const void* d_ptr, uint64_t count) {
        const blz_vec_arg a = words(d_ptr, count);
        vec_gather(dst, &a, view(0, 1, count));
    }
    // scatter-add (blz_ntt_vec_scatter): buffer dst[t] = sum over k < nnz with d_idx[k] mod n == t of val[k] x[src(k) mod count],
    // src(k) = d_src ? d_src[k] : k; x null: ones (d_src null too), d_val null: coefficients 1; x may not name dst.  With
    // d_idx = col, d_src = the row of each nonzero and x = y: the transposed sparse product.  vec_count: dst[t] = the number of
    // entries of d_idx that name t, the multiplicities of a lookup argument
    static blz_vec_scatter scatter(const uint32_t* d_idx, const uint32_t* d_src, const void* d_val, uint64_t nnz) {
        return blz_vec_scatter{d_idx, d_src, d_val, nnz, 0};
    }
    void vec_scatter(size_t dst, const blz_vec_arg* x, const blz_vec_scatter& s) { check(blz_ntt_vec_scatter(h_, dst, x, &s)); }
    void vec_count(size_t dst, const uint32_t* d_idx, uint64_t nnz) { vec_scatter(dst, nullptr, scatter(d_idx, nullptr, nullptr, nnz)); }
    // sparse matrix times vector (blz_ntt_vec_spmv): buffer dst[p] = sum over the nonzeros k of row p of val[k] x[col[k] mod count],
    // 0 for an empty row and above rows; x may not name dst.  csr(row_ptr, col, val, rows, nnz) builds the struct from device
    // pointers (val null: coefficients 1).  vec_index: dst[p] = x[col[p] mod count] (times val[p]), the data-dependent gather
    static blz_vec_csr csr(const uint32_t* d_row_ptr, const uint32_t* d_col, const void* d_val, uint64_t rows, uint64_t nnz) {
        return blz_vec_csr{d_row_ptr, d_col, d_val, rows, nnz};
    }
    void vec_spmv(size_t dst, const blz_vec_arg* x, const blz_vec_csr& m) { check(blz_ntt_vec_spmv(h_, dst, x, &m)); }
    void vec_index(size_t dst, const blz_vec_arg* x, const uint32_t* d_col, uint64_t count, const void* d_val = nullptr) {
        vec_spmv(dst, x, csr(nullptr, d_col, d_val, count, count));
    }
    // multilinear tables (blz_ntt_vec_mle_fold / _round / _eq): the steps of a sumcheck round on tables of live length len = 2^m.
    // vec_mle_fold: dst[p] = lo + r (hi - lo), p < len / 2, pairs (a[p], a[p + len / 2]) or with BLZ_MLE_LOW (a[2p], a[2p + 1]); dst
    // is buffer(i) or words(p, count) and may be a (in place); r one device word.  vec_mle_round: d_out[t] = sum over the pairs of
    // the product over the operands given (a, b, c; nullptr: not taken) of lo + t (hi - lo), t < points (default: operands + 1).
    // vec_mle_eq: dst[p] = eq(point, p), p < 2^m, the point m device words.  Exactly the words named are written
    void vec_mle_fold(const blz_vec_arg* dst, const blz_vec_arg* a, const blz_vec_arg* r, uint64_t len, uint32_t flags = 0) {
        check(blz_ntt_vec_mle_fold(h_, flags, dst, a, r, len));
    }
    void vec_mle_round(const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c, uint64_t len, void* d_out, uint32_t points = 0,
                       uint32_t flags = 0) {
        check(blz_ntt_vec_mle_round(h_, flags, a, b, c, points ? points : 2u + (b ? 1u : 0u) + (c ? 1u : 0u), len, d_out));
    }
    void vec_mle_eq(const blz_vec_arg* dst, const void* d_point, uint32_t m) { check(blz_ntt_vec_mle_eq(h_, dst, d_point, m)); }
    // a sumcheck step in one pass (blz_ntt_sumcheck_step): with r (one device word) every table given (a, b, c, d; nullptr: not
    // taken) is folded in place - len / 2 words of each are written - and d_out[t], t < points, is the round polynomial of the gate
    // (BLZ_GATE_PRODUCT: a, a b, a b c; BLZ_GATE_R1CS: a (b c - d)) on the folded tables; without r the round polynomial of the
    // tables as they are.  points defaults to the gate's degree + 1; bind_only (r, no d_out) folds and takes no round
    void sumcheck_step(uint32_t gate, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c, const blz_vec_arg* d,
                       const blz_vec_arg* r, uint64_t len, void* d_out, uint32_t points = 0, bool bind_only = false) {
        const uint32_t degree = gate == BLZ_GATE_R1CS ? 3u : 1u + (b ? 1u : 0u) + (c ? 1u : 0u);
        check(blz_ntt_sumcheck_step(h_, gate, a, b, c, d, r, bind_only ? 0u : points ? points : degree + 1u, len, d_out));
    }
    // the same step for a caller-defined gate (blz_ntt_sumcheck_gate): G = tables[common] x sum of the gate's signed products of
    // tables; `tables` holds gate.ntables operands and with r EVERY one is folded in place.  points defaults to the gate's degree
    // + 1 (the longest term's factors, plus one for a common factor), at most BLZ_GATE_MAX_POINTS
    void sumcheck_gate(const blz_sum_gate& gate, const blz_vec_arg* tables, const blz_vec_arg* r, uint64_t len, void* d_out, uint32_t points = 0,
                       bool bind_only = false) {
        uint32_t degree = 0;
        for (uint32_t m = 0; m < gate.nterms && m < BLZ_GATE_MAX_TERMS; ++m) degree = gate.term[m].nfactors > degree ? gate.term[m].nfactors : degree;
        degree += gate.common >= 0 ? 1u : 0u;
        check(blz_ntt_sumcheck_gate(h_, &gate, tables, r, bind_only ? 0u : points ? points : degree + 1u, len, d_out));
    }
    // the gate step of a zerocheck (blz_ntt_zerocheck_gate): sumcheck_gate with eq out of the gate and the summed weight table
    // `weight` - device words, for round 0 vec_mle_eq over m - 1 variables - in its place.  Without r: d_out[t] = sum_p W[p] G(pair
    // p at t); with r every table is folded in place, W[q] += W[q + len / 4] for q < len / 4, and d_out is the weighted round of
    // the folded tables: u_i of s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X).  points defaults to the gate's degree + 1, nothing added
    // for the weight; there is no bind alone (that is sumcheck_gate's)
    void zerocheck_gate(const blz_sum_gate& gate, const blz_vec_arg* tables, const blz_vec_arg& weight, const blz_vec_arg* r, uint64_t len, void* d_out,
                        uint32_t points = 0) {
        uint32_t degree = 0;
        for (uint32_t m = 0; m < gate.nterms && m < BLZ_GATE_MAX_TERMS; ++m) degree = gate.term[m].nfactors > degree ? gate.term[m].nfactors : degree;
        degree += gate.common >= 0 ? 1u : 0u;
        check(blz_ntt_zerocheck_gate(h_, &gate, tables, &weight, r, points ? points : degree + 1u, len, d_out));
    }
    // the same description evaluated position by position (blz_ntt_gate_eval): dst[p] = the gate over table i read at
    // (p + rot[i]) mod its count, p < len (1 .. n, any value); rot: gate.ntables host values or nullptr for all zero.  dst is
    // buffer(i) or words(p, count) and may be a table that starts where it starts, holds len words and is not rotated; exactly
    // len words are written
    void gate_eval(const blz_sum_gate& gate, const blz_vec_arg* dst, const blz_vec_arg* tables, uint64_t len, const uint64_t* rot = nullptr) {
        check(blz_ntt_gate_eval(h_, &gate, dst, tables, rot, len));
    }
    // gate_eval with linear-form factors (blz_ntt_gate_eval_lin) - products of sums: a factor byte of a term, and common, is a
    // table index or BLZ_LIN_FORM | k, the value of gate.form[k] = sum of (+/-) [T[coef] x] T[table].  Up to 16 tables, one
    // rotation per table index whatever names it; dst, len and in place as for gate_eval
    void gate_eval_lin(const blz_lin_gate& gate, const blz_vec_arg* dst, const blz_vec_arg* tables, uint64_t len, const uint64_t* rot = nullptr) {
        check(blz_ntt_gate_eval_lin(h_, &gate, dst, tables, rot, len));
    }
    // every layer of the product (BLZ_TREE_PROD) or fraction (BLZ_TREE_FRAC) tree under the len = 2^m words of a
    // (blz_ntt_mle_tree): layer k, len / 2^k words, at word tree_layer(len, k) of dst, len - 1 words in all; pairs (L[p],
    // L[p + size / 2]), or (L[2p], L[2p + 1]) with BLZ_MLE_LOW.  FRAC carries (a, a_q) to (dst, dst_q) by (P_lo Q_hi + P_hi Q_lo,
    // Q_lo Q_hi); PROD takes neither _q.  A destination is buffer(i) or words(p, count) and meets no source and not the other one
    void mle_tree(uint32_t op, const blz_vec_arg* dst, const blz_vec_arg* a, uint64_t len, uint32_t flags = 0, const blz_vec_arg* dst_q = nullptr,
                  const blz_vec_arg* a_q = nullptr) {
        check(blz_ntt_mle_tree(h_, op, flags, dst, dst_q, a, a_q, len));
    }
    // the word offset of layer k (1 .. m) in a destination of mle_tree; the layer holds len >> k words
    static uint64_t tree_layer(uint64_t len, uint32_t k) { return len - (len >> (k - 1)); }
    // one step of the on-device Fiat-Shamir transcript (blz_ntt_fs_challenge): digest = SHA3-256(state || the first count words of
    // words, as stored), the digest back into d_state and, with every bit from bitlen(modulus) - 1 upward cleared, into d_r
    // (nullptr: absorb only).  count <= 32; words may be nullptr when count is 0
    void fs_challenge(void* d_state, const blz_vec_arg* words, uint32_t count, void* d_r) { check(blz_ntt_fs_challenge(h_, d_state, words, count, d_r)); }
    // a whole sumcheck in one call (blz_ntt_sumcheck_prove): the round alone, then per variable the transcript step over the round
    // just written and the step with that challenge, then the bind alone, with no host wait in between.  weight == nullptr: the
    // sum of the gate by sumcheck_gate's steps, else the weighted sum by zerocheck_gate's.  m = log2 len: d_rounds receives
    // m x points words, d_challenges m words, d_state is the transcript; points defaults to the gate's degree + 1
    void sumcheck_prove(const blz_sum_gate& gate, const blz_vec_arg* tables, const blz_vec_arg* weight, uint64_t len, void* d_state, void* d_rounds,
                        void* d_challenges, uint32_t points = 0) {
        uint32_t degree = 0;
        for (uint32_t m = 0; m < gate.nterms && m < BLZ_GATE_MAX_TERMS; ++m) degree = gate.term[m].nfactors > degree ? gate.term[m].nfactors : degree;
        degree += gate.common >= 0 ? 1u : 0u;
        check(blz_ntt_sumcheck_prove(h_, &gate, tables, weight, points ? points : degree + 1u, len, d_state, d_rounds, d_challenges));
    }
    // the GKR grand product over a product tree in one call (blz_ntt_gkr_prove): tree is what mle_tree(BLZ_TREE_PROD, tree, a, len)
    // left over the len = 2^m leaves a; from the root down each layer's sumcheck, its two final words and their transcript step,
    // with no host wait in between.  d_weight: max(len / 4, 1) words of scratch; d_rounds 3 m (m - 1) / 2 words, d_points
    // m (m + 1) / 2, d_claims 2 m (gkr_rounds_words and its neighbours); fused == false: BLZ_GKR_UNFUSED, the chain of single
    // launches.  Both tree and a are consumed
    void gkr_prove(const blz_vec_arg* tree, const blz_vec_arg* a, uint64_t len, void* d_weight, void* d_state, void* d_rounds, void* d_points,
                   void* d_claims, bool fused = true) {
        check(blz_ntt_gkr_prove(h_, BLZ_TREE_PROD, fused ? 0u : BLZ_GKR_UNFUSED, tree, a, len, d_weight, d_state, d_rounds, d_points, d_claims));
    }
    // the words of gkr_prove's outputs for a tree over 2^m leaves, and the word of layer j's round i, point row and claims row
    static uint64_t gkr_rounds_words(uint32_t m) { return 3ull * m * (m - 1) / 2; }
    static uint64_t gkr_points_words(uint32_t m) { return (uint64_t)m * (m + 1) / 2; }
    static uint64_t gkr_claims_words(uint32_t m) { return 2ull * m; }
    static uint64_t gkr_round(uint32_t j, uint32_t i) { return 3 * ((uint64_t)j * (j - 1) / 2 + i); }
    static uint64_t gkr_point_row(uint32_t j) { return (uint64_t)j * (j + 1) / 2; }
    static uint64_t gkr_claim_row(uint32_t j) { return 2ull * j; }
    // the GKR argument over a fraction tree (logUp-GKR) in one call (blz_ntt_gkr_prove_frac): tree_p, tree_q are what
    // mle_tree(BLZ_TREE_FRAC, tree_p, a_p, len, 0, tree_q, a_q) left over the len = 2^m numerators a_p and denominators a_q, none
    // periodic.  Layer j >= 1 draws lambda_j, writes T = P_hi + lambda_j Q_hi over P_hi and proves P_lo Q_hi + Q_lo T under the
    // weight; four final words a layer.  d_rounds and d_points as for gkr_prove, d_claims 4 m words, d_lambdas m (word 0 is never
    // written); fused == false: BLZ_GKR_UNFUSED.  All four operands are consumed
    void gkr_prove_frac(const blz_vec_arg* tree_p, const blz_vec_arg* tree_q, const blz_vec_arg* a_p, const blz_vec_arg* a_q, uint64_t len, void* d_weight,
                        void* d_state, void* d_rounds, void* d_points, void* d_claims, void* d_lambdas, bool fused = true) {
        check(blz_ntt_gkr_prove_frac(h_, fused ? 0u : BLZ_GKR_UNFUSED, tree_p, tree_q, a_p, a_q, len, d_weight, d_state, d_rounds, d_points, d_claims, d_lambdas));
    }
    // the words of gkr_prove_frac's claims and lambdas, and the word of layer j's claims row (rounds and points: gkr_prove's)
    static uint64_t gkr_frac_claims_words(uint32_t m) { return 4ull * m; }
    static uint64_t gkr_frac_lambdas_words(uint32_t m) { return m; }
    static uint64_t gkr_frac_claim_row(uint32_t j) { return 4ull * j; }
    // {device bytes held, pass 2 reads its factor table, pass 1 boundary table, log_size}
    std::array<uint64_t, 4> info() {
        std::array<uint64_t, 4> v{};
        check(blz_ntt_info(h_, v.data()));
        return v;
    }
};

// ---------------------------------------------------------------- Poseidon tree (src/ingo_hash)
enum class Hash { Poseidon };                                      // poseidon_api.rs:11-13
enum class TreeMode { TreeC = 0, TreeD = 1 };                      // utils.rs:18-30
inline uint32_t num_of_elements_oct_tree(uint32_t h) { uint32_t s = 0; for (uint32_t i = 0; i < h; ++i) s += 1u << (3 * (h - i - 1)); return s; }  // utils.rs:2-10
inline uint32_t num_of_elements_in_base_layer(uint32_t h) { return 1u << (3 * (h - 1)); }                                                          // utils.rs:12-14
struct PoseidonInitializeParameters { uint32_t tree_height; TreeMode tree_mode; std::string instruction_path; };   // poseidon_api.rs:19-24
struct PoseidonResult {                                                                                             // poseidon_api.rs:26-30
    std::array<uint8_t, 32> hash_byte;
    uint32_t hash_id, layer_id;
    // poseidon_api.rs:42-71: 64 bytes per record; hash_id in bits 0-29, layer_id in bits 30-39 of the second half
    static std::vector<PoseidonResult> parse_poseidon_hash_results(const std::vector<uint8_t>& data) {
        std::vector<PoseidonResult> out;
        for (size_t k = 0; k + 64 <= data.size(); k += 64) {
            PoseidonResult r{};
            for (int i = 0; i < 32; ++i) r.hash_byte[i] = data[k + i];
            const uint8_t* d = data.data() + k + 32;
            r.hash_id = (uint32_t(d[0]) | uint32_t(d[1]) << 8 | uint32_t(d[2]) << 16 | uint32_t(d[3]) << 24) & 0x3fffffffu;
            r.layer_id = (uint32_t(d[3]) | uint32_t(d[4]) << 8) >> 6;
            out.push_back(r);
        }
        return out;
    }
};

// The hash is the caller's: the instruction CSV carries the Poseidon instance (blaze_hip.h "THE INSTRUCTION STREAM").
class PoseidonClient : public DriverPrimitive<Hash, PoseidonInitializeParameters, std::vector<uint8_t>, std::vector<PoseidonResult>> {
    blz_poseidon* h_ = nullptr;

   public:
    DriverClient dclient;
    // poseidon_api.rs:77-79; `field` (a Curve: the scalar field of that curve) has no reference counterpart
    PoseidonClient(Hash, DriverClient dclient_, Curve field = Curve::BLS381) : dclient(dclient_) { check(blz_poseidon_new(dclient.id, int(field), &h_)); }
    ~PoseidonClient() override { blz_poseidon_free(h_); }
    PoseidonClient(const PoseidonClient&) = delete;
    PoseidonClient& operator=(const PoseidonClient&) = delete;

    std::vector<uint32_t> loaded_binary_parameters() const override {                                         // :81-94
        uint32_t v[2];
        check(blz_poseidon_loaded_binary_parameters(h_, v));
        return {v[0], v[1]};
    }
    void initialize(const PoseidonInitializeParameters& p) override {                                         // :96-111
        check(blz_poseidon_initialize(h_, p.tree_height, int(p.tree_mode), p.instruction_path.c_str()));
    }
    void set_data(const std::vector<uint8_t>& input) override { check(blz_poseidon_set_data(h_, input.data(), input.size())); }   // :117-122
    void start_process(std::optional<size_t> = std::nullopt) override { throw std::logic_error("todo!() in the reference (poseidon_api.rs:113-115)"); }
    void wait_result() override { check(blz_poseidon_wait_result(h_)); }       // todo!() in the reference; here: everything fed so far is hashed
    std::optional<std::vector<PoseidonResult>> result(std::optional<size_t> expected = std::nullopt) override {   // :128-145, bounded
        std::vector<uint8_t> raw(64 * expected.value());
        uint32_t n = 0;
        check(blz_poseidon_result(h_, uint32_t(expected.value()), raw.data(), raw.size(), &n));
        raw.resize(64 * size_t(n));
        return PoseidonResult::parse_poseidon_hash_results(raw);
    }
    uint32_t get_num_of_pending_results() {                                                                    // :156-161
        uint32_t v = 0;
        check(blz_poseidon_num_pending_results(h_, &v));
        return v;
    }
    std::vector<uint8_t> get_raw_results(uint32_t num_of_results) {                                            // :191-196
        std::vector<uint8_t> raw(64 * size_t(num_of_results));
        check(blz_poseidon_raw_results(h_, num_of_results, raw.data(), raw.size()));
        return raw;
    }
    std::array<uint32_t, 4> counters() {
        std::array<uint32_t, 4> v{};
        check(blz_poseidon_counters(h_, v.data()));
        return v;
    }
    uint32_t get_last_element_sent_to_ring() { return counters()[0]; }                                         // :149-154
    uint32_t get_last_hash_sent_to_host() { return counters()[1]; }                                            // :198-203
    void initialize_words(uint32_t tree_height, TreeMode mode, const std::vector<uint8_t>& words) {
        check(blz_poseidon_initialize_words(h_, tree_height, int(mode), words.data(), words.size()));
    }
    void reset() { check(blz_poseidon_reset(h_)); }
    void set_round_plan(bool enable) { check(blz_poseidon_set_round_plan(h_, enable ? 1 : 0)); }
    // derive and self-check the optimised partial rounds now: {in force, self-check state (1 equal, 2 refused: dense rounds)}
    std::array<uint32_t, 2> prepare_round_plan() {
        std::array<uint32_t, 2> v{};
        check(blz_poseidon_prepare_round_plan(h_, v.data()));
        return v;
    }
};

}  // namespace ingo_blaze
