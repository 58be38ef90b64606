// Radix-2^k NTT over a scalar field (BLS12-381 Fr by default; BLS12-377 / BN254 Fr on request) for gfx950 (device task of SURVEY.md a16: what the
// bitstream behind src/ingo_ntt/ntt_hw_code.rs:6-83 computes on one 2^27 x 32 B buffer).
//
//   X[k] = sum_i x[i] w^(ik),  natural order in and out,  w = 7^((r-1)/2^log_size)
//
// n = A*B*C (each <= 512).  With i = i0 + A i1 + AB i2 and k = k2 + C k1 + CB k0:
//   pass 1: C-point NTTs over i2 (stride AB), then * w^(A i1 k2)
//   pass 2: B-point NTTs over i1 (stride A),  then * w^(i0 (k2 + C k1))
//   pass 3: A-point NTTs over i0 (contiguous), written to the natural address k2 + C k1 + CB k0
// A pass stages a tile of COLS adjacent columns x radix rows in LDS (COLS*32 B contiguous per row
// access), runs the radix-2 stages there and applies the inter-pass twiddle on the way out.
// A handle with a coset shift g (blz_ntt_set_coset) computes X[k] = sum_i x[i] g^i w^(ik) - or the exact inverse - in the same three
// launches: the powers of g ride on the passes' own factors (ntt_engine.hpp NttCoset).
// Data stay in plain canonical form; only twiddles are in Montgomery form (mont_mul(x, tR) = x t),
// so there is no conversion pass.  Algorithmic traffic 2 x 4 GiB; this 3-pass form moves 3x that.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "ntt_engine.hpp"
#include "ntt_fs.hip.hpp"

namespace blz {


// NTTBanks::preprocess / postprocess (src/ingo_ntt/ntt_data.rs:80-156) as device permutations of
// 32-byte elements, from the closed forms of the reference loops:
//   preprocess : element e = 512 blk + j  ->  bank (blk%2)*8 + j%8, slot (blk/2)*64 + j/8
//   postprocess: output a = 512 isub + i, isub = ic*G + g + 2G*blk
//                <- bank ((ic ^ (g&1))*8 + i%8), slot (g*Bg + blk)*64 + i/8      (G groups, Bg blocks each)
__global__ __launch_bounds__(256) void k_ntt_banks_pre(const uint4* __restrict__ in, uint4* __restrict__ banks, uint64_t n) {
    uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    uint64_t blk = e >> 9, j = e & 511;
    uint64_t bank = (blk & 1) * 8 + (j & 7), slot = (blk >> 1) * 64 + (j >> 3);
    uint64_t dst = bank * (n >> 4) + slot;
    banks[2 * dst] = in[2 * e];
    banks[2 * dst + 1] = in[2 * e + 1];
}
__global__ __launch_bounds__(256) void k_ntt_banks_post(const uint4* __restrict__ banks, uint4* __restrict__ out, uint64_t n,
                                                        uint64_t G, uint64_t Bg) {
    uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    uint64_t isub = a >> 9, i = a & 511;
    uint64_t blk = isub / (2 * G), ic = (isub % (2 * G)) / G, g = isub % G;
    uint64_t bank = ((ic ^ (g & 1)) * 8) + (i & 7), slot = (g * Bg + blk) * 64 + (i >> 3);
    uint64_t src = bank * (n >> 4) + slot;
    out[2 * a] = banks[2 * src];
    out[2 * a + 1] = banks[2 * src + 1];
}

#ifdef BLZ_EXPERIMENT_KNOBS
__global__ __launch_bounds__(256) void k_copy16(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
#endif

}  // namespace blz

using namespace blz;

struct blz_ntt {
    int device = 0;
    int field = BLZ_BLS381;  // scalar field of this curve (enum blz_curve)
    const NttFieldOps* ops = nullptr;
    int logn = 27;
    int inverse = 0;
    bool force_generic = false;  // (experiment builds, BLAZE_NTT_GENERIC=1: radix-2-in-LDS kernel for every pass)
    NttGeom geom{};
    int cols_log[3] = {0, 0, 0};
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host<->buffer traffic, concurrent with the compute stream
    hipStream_t copy_stream2 = nullptr; // blz_ntt_exchange: the host -> device direction, while copy_stream carries device -> host
    uint32_t flags = 0;                 // blz_ntt_new_ex2 / _ex3
    bool has_root = false;              // blz_ntt_new_ex3: the caller's primitive 2^logn-th root (canonical little-endian words)
    uint8_t root[32] = {};
    hipEvent_t xchg_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // blz_ntt_exchange with pinned host buffers: piece k has left
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf buf[2], scratch, tables, tables_rr, table_b;
    NttTables T{};
    NttTablesRR TR{};
    // blz_ntt_set_coset: the shift in force (1 = the plain transform), its tables (allocated by the first shift that is not 1)
    bool coset = false;
    uint8_t shift[32] = {1};
    DevBuf tables_cs;
    NttCoset CS{};
    bool cs_wire = false;       // the 512-point kernel is the wire pass of a forward handle: CS.tG exists
    uint32_t* cs_stage = nullptr;   // device: s | the caller's shift | the check's flag
    bool in_flight = false;
    int in_flight_buf = -1;   // buffer under transform (or written by an element-wise op) while in_flight
    uint32_t in_flight_reads = 0;   // blz_ntt_vec_op in flight: bit b = transform buffer b is an operand it reads
    int in_flight_buf2 = -1;  // blz_ntt_sumcheck_step in flight: the second buffer it writes (both buffers may be tables), else -1
    float last_ms = 0.f;
    bool wedged = false;      // a wait ran into BLAZE_WAIT_TIMEOUT_MS: only reset / free are accepted (common.hpp)
};

#define BLZ_NTT_LIVE(h)                                                                                          \
    do {                                                                                                         \
        if ((h)->wedged)                                                                                         \
            return fail(BLZ_ERR_UNKNOWN, "handle is wedged: an earlier wait timed out (BLAZE_WAIT_TIMEOUT_MS); only " \
                                         "reset / free are accepted");                                           \
    } while (0)
#define BLZ_NTT_WAIT(h, expr)                      \
    do {                                           \
        blz::wait_clear();                         \
        int rc__ = (expr);                         \
        if (rc__ != BLZ_OK) {                      \
            if (blz::wait_timed_out()) (h)->wedged = true; \
            return rc__;                           \
        }                                          \
    } while (0)

namespace {

size_t ntt_bytes(const blz_ntt* h) { return (size_t)32 << h->logn; }
// what is in flight writes transform buffer `buf`
bool ntt_buf_in_flight(const blz_ntt* h, size_t buf) { return h->in_flight && (h->in_flight_buf == (int)buf || h->in_flight_buf2 == (int)buf); }

const NttFieldOps* ntt_ops_for(int field) {
    switch (field) {
        case BLZ_BLS377: return &ntt_ops_bls377();
        case BLZ_BLS381: return &ntt_ops_bls381();
        case BLZ_BN254: return &ntt_ops_bn254();
    }
    return nullptr;
}

int ntt_setup(blz_ntt* h) {
    // split logn into three radices, largest last-pass first so the contiguous pass is wide
    int l = h->logn;
    int la = l > 9 ? 9 : l;
    int lb = (l - la) > 9 ? 9 : (l - la);
    int lc = l - la - lb;
    if (lc > 9) return fail(BLZ_ERR_INVALID_PARAM, "log_size %d not supported (max 27)", l);
    h->geom = NttGeom{la, lb, lc, l, lc ? 1 : lb ? 2 : 3, (h->flags & BLZ_NTT_BITREV_INPUT) ? 1 : 0, (h->flags & BLZ_NTT_BITREV_OUTPUT) ? 1 : 0};
    // columns per tile: LDS = radix * (COLS + 1) * 32 B <= 160 KiB, and COLS <= extent of the column index
    auto pick = [](int lr, int lcols_avail) {
        int c = 17 - 5 - lr;  // log2(128 KiB / 32 B / radix)
        if (c > 3) c = 3;
        if (c > lcols_avail) c = lcols_avail;
        if (c < 0) c = 0;
        return c;
    };
    h->cols_log[0] = pick(lc, la);  // pass 1: cols i0 (< A)
    h->cols_log[1] = pick(lb, la);  // pass 2: cols i0 (< A)
    h->cols_log[2] = pick(la, lc);  // pass 3: cols k2 (< C)
    size_t tb = (size_t)(3 * 512 + 3 * 512 + 1 + 1 + 2) * 32;   // wpass x 3, t0..t2, ninv, wbase, (the caller's root | the root check's flag)
    BLZ_TRY(h->tables.reserve(tb));
    uint32_t* p = h->tables.as<uint32_t>();
    for (int i = 0; i < 3; ++i) { h->T.wpass[i] = p; p += 512 * 8; }
    h->T.t0 = p; p += 512 * 8;
    h->T.t1 = p; p += 512 * 8;
    h->T.t2 = p; p += 512 * 8;
    h->T.ninv = h->inverse ? p : nullptr; p += 8;
    h->T.wbase = p; p += 8;
    uint32_t* const d_user_root = p; p += 8;
    uint32_t* const d_root_flag = p; p += 8;
    BLZ_HIP(hipMemsetAsync(d_root_flag, 0, 4, h->stream), BLZ_ERR_UNKNOWN);
    if (h->has_root) BLZ_HIP(hipMemcpyAsync(d_user_root, h->root, 32, hipMemcpyHostToDevice, h->stream), BLZ_ERR_WRITE);
    // the boundary table exists only where all three passes run the 512-point kernel (2^27), so that the factor it
    // splits off is re-joined by the same kernel in pass 2
    const bool want_ta = lc == 9 && !h->force_generic && exp_knob("BLAZE_NTT_TABLE", 1) != 0;
    BLZ_TRY(h->tables_rr.reserve(NTT_RR_TABLE_BYTES + (want_ta ? NTT_RR_BOUNDARY_BYTES : 0)));
    {
        uint32_t* q = h->tables_rr.as<uint32_t>();
        for (int i = 0; i < 3; ++i) { h->TR.wpass[i] = q; q += 2 * 512 * NTT_RR_ENTRY_DWORDS; }   // Shoup entries
        h->TR.t0 = q; q += 512 * NTT_RR_ENTRY_DWORDS;
        h->TR.t1 = q; q += 512 * NTT_RR_ENTRY_DWORDS;
        h->TR.t2 = q; q += 512 * NTT_RR_ENTRY_DWORDS;
        h->TR.fin = h->inverse ? q : nullptr; q += NTT_RR_ENTRY_DWORDS;
        h->TR.ts2 = q; q += 2 * 512 * NTT_RR_ENTRY_DWORDS;   // Shoup entries
        h->TR.tA = want_ta ? q : nullptr;
        // pass 2's boundary factors, one per element (4 GiB at 2^27: the transform's buffers are 8): only beside tA, whose
        // split of pass 1's factor it completes
        const bool want_tb = want_ta && !(h->flags & BLZ_NTT_NO_FACTOR_TABLE) && exp_knob("BLAZE_NTT_TB", 1) != 0;
        h->TR.tB = nullptr;
        if (want_tb) {
            // (an optimisation, not a need: a device too full for it steps the factors as smaller transforms do)
            if (h->table_b.reserve(ntt_bytes(h), true) == BLZ_OK) h->TR.tB = h->table_b.as<uint32_t>();
            else BLZ_LOG(1, "NTT: no memory for the boundary-factor table (%zu bytes): pass 2 steps its factors", ntt_bytes(h));
        }
        // pass 1 tile order (ntt_rr.hip.hpp): 0 plain, 1 + s: 2^s adjacent column groups back to back (s = 3), + 16 b: b bits of
        // i1 walked first (default 7)
        h->TR.swz = (la == 9 && lb == 9) ? (uint32_t)exp_knob("BLAZE_NTT_SWZ", 4) : 0u;
        if ((h->TR.swz & 15u) > 6u) h->TR.swz = 6u;
    }
    BLZ_TRY(h->ops->setup(h->stream, h->T, h->TR, h->geom, h->inverse, h->has_root ? d_user_root : nullptr, d_root_flag));
    if (h->has_root) {
        // the caller's root was checked on the device ahead of the tables built from it (k_ntt_root)
        uint32_t bad = 0;
        BLZ_TRY(sync_stream_bounded(h->stream, "NTT set-up: root check"));
        BLZ_HIP(hipMemcpy(&bad, d_root_flag, 4, hipMemcpyDeviceToHost), BLZ_ERR_READ);
        if (bad)
            return fail(BLZ_ERR_INVALID_PARAM, bad == 1 ? "the root is not a canonical element of the field (>= r)"
                                                        : "the root is not a primitive 2^%d-th root of unity (root^(2^%d) != -1)", h->logn, h->logn - 1);
    }
    // both transform buffers exist from the start, zero-filled, like the card's two HBM buffers: the reference's
    // double-buffer loop opens with start_process on a buffer nobody wrote and result on the other
    // (tests/integration_ntt.rs:102-136, cycle 0)
    for (int b = 0; b < 2; ++b) {
        BLZ_TRY(h->buf[b].reserve(ntt_bytes(h), true));   // (a transform's size is fixed: no growth slack - it was 1.5 GiB at 2^27)
        BLZ_HIP(hipMemsetAsync(h->buf[b].p, 0, ntt_bytes(h), h->stream), BLZ_ERR_UNKNOWN);
    }
    BLZ_TRY(h->scratch.reserve(ntt_bytes(h), true));
    BLZ_TRY(sync_stream_bounded(h->stream, "NTT set-up: tables and zero-filled buffers"));
    return BLZ_OK;
}

int launch_pass(blz_ntt* h, int pass, const void* in, void* out) {
    return h->ops->pass(pass, h->stream, in, out, h->geom, h->T, h->TR, h->cols_log[pass - 1], h->force_generic, h->coset ? &h->CS : nullptr);
}

}  // namespace

extern "C" {

int blz_ntt_new(int device_id, int log_size, blz_ntt** out) { return blz_ntt_new_ex(device_id, log_size, 0, out); }

int blz_ntt_new_ex(int device_id, int log_size, int inverse, blz_ntt** out) {
    return blz_ntt_new_field(device_id, BLZ_BLS381, log_size, inverse, out);
}

int blz_ntt_new_field(int device_id, int field, int log_size, int inverse, blz_ntt** out) {
    return blz_ntt_new_ex2(device_id, field, log_size, inverse, 0u, out);
}

int blz_ntt_new_ex2(int device_id, int field, int log_size, int inverse, uint32_t flags, blz_ntt** out) {
    if (flags & ~(uint32_t)BLZ_NTT_NO_FACTOR_TABLE) return fail(BLZ_ERR_INVALID_PARAM, "unknown NTT flags 0x%x", flags);
    return blz_ntt_new_ex3(device_id, field, log_size, flags | (inverse ? BLZ_NTT_INVERSE : 0u), nullptr, out);
}

int blz_ntt_new_ex3(int device_id, int field, int log_size, uint32_t flags, const uint8_t* root, blz_ntt** out) {
    if (!out) return fail(BLZ_ERR_INVALID_PARAM, "null out");
    *out = nullptr;
    if (flags & ~(uint32_t)(BLZ_NTT_NO_FACTOR_TABLE | BLZ_NTT_INVERSE | BLZ_NTT_BITREV_INPUT | BLZ_NTT_BITREV_OUTPUT))
        return fail(BLZ_ERR_INVALID_PARAM, "unknown NTT flags 0x%x", flags);
    const int inverse = (flags & BLZ_NTT_INVERSE) ? 1 : 0;
    const NttFieldOps* ops = ntt_ops_for(field);
    if (!ops) return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
    if (log_size < 1 || log_size > NTT_MAX_LOG) return fail(BLZ_ERR_INVALID_PARAM, "log_size %d out of range [1,%d]", log_size, NTT_MAX_LOG);
    if (log_size > ops->two_adicity)
        return fail(BLZ_ERR_INVALID_PARAM, "log_size %d exceeds the two-adicity %d of the field", log_size, ops->two_adicity);
    BLZ_TRY(use_device(device_id));
    blz_ntt* h = new blz_ntt();
    h->device = device_id;
    h->field = field;
    h->ops = ops;
    h->logn = log_size;
    h->inverse = inverse ? 1 : 0;
    h->flags = flags;
    if (root) {
        h->has_root = true;
        memcpy(h->root, root, 32);
    }
    h->force_generic = exp_knob("BLAZE_NTT_GENERIC", 0) != 0;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->copy_stream2, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->xchg_ev[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    int rc = e == hipSuccess ? ntt_setup(h) : fail_hip(BLZ_ERR_UNKNOWN, "stream/event creation failed: %s", hipGetErrorString(e));
    if (rc != BLZ_OK) {
        blz_ntt_free(h);
        return rc;
    }
    *out = h;
    return BLZ_OK;
}

void blz_ntt_free(blz_ntt* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream && (sync_stream_bounded(h->stream, "free: NTT stream") != BLZ_OK ||
                      sync_stream_bounded(h->copy_stream, "free: NTT copy stream") != BLZ_OK ||
                      (h->copy_stream2 && sync_stream_bounded(h->copy_stream2, "free: NTT copy stream") != BLZ_OK))) {
        BLZ_LOG(0, "NTT handle freed while its device work is wedged: buffers and streams are leaked");
        delete h;
        return;
    }
    h->buf[0].release(); h->buf[1].release(); h->scratch.release(); h->tables.release(); h->tables_rr.release(); h->table_b.release(); h->tables_cs.release();
    for (auto& e : h->xchg_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->copy_stream2) (void)hipStreamDestroy(h->copy_stream2);
    delete h;
}

int blz_ntt_initialize(blz_ntt* h) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    return BLZ_OK;  // ntt_api.rs:37-56 writes debug-program registers; nothing to program here
}

static int ntt_set_data_common(blz_ntt* h, size_t buf_host, const void* data, size_t len, bool on_device) {
    if (!h || !data) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (buf_host > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_host must be 0 or 1");
    if (len != ntt_bytes(h)) return fail(BLZ_ERR_INVALID_PARAM, "data length %zu != %zu", len, ntt_bytes(h));
    BLZ_NTT_LIVE(h);
    if (ntt_buf_in_flight(h, buf_host))
        return fail(BLZ_ERR_INVALID_PARAM, "buffer %zu is being transformed; call wait_result first", buf_host);
    if (h->in_flight && ((h->in_flight_reads >> buf_host) & 1u))
        return fail(BLZ_ERR_INVALID_PARAM, "buffer %zu is read by the element-wise op in flight; call wait_result first", buf_host);
    BLZ_TRY(use_device(h->device));
    // a dedicated copy stream: the compute stream may be busy on the other buffer (double-buffer
    // contract, tests/integration_ntt.rs:102-136).  Synchronised before returning: set_data is
    // blocking, and a device-to-device hipMemcpy alone is not ordered against other streams.
    BLZ_HIP(hipMemcpyAsync(h->buf[buf_host].p, data, len, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           h->copy_stream), BLZ_ERR_WRITE);
    BLZ_NTT_WAIT(h, sync_stream_bounded(h->copy_stream, "set_data: copy into the NTT buffer"));
    return BLZ_OK;
}

int blz_ntt_set_data(blz_ntt* h, size_t buf_host, const uint8_t* data, size_t len) {
    return ntt_set_data_common(h, buf_host, data, len, false);
}
int blz_ntt_set_data_device(blz_ntt* h, size_t buf_host, const void* d_data, size_t len) {
    return ntt_set_data_common(h, buf_host, d_data, len, true);
}

int blz_ntt_start_process(blz_ntt* h, size_t buf_kernel) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (buf_kernel > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_kernel must be 0 or 1");
    BLZ_NTT_LIVE(h);
    if (h->in_flight) return fail(BLZ_ERR_INVALID_PARAM, "a transform is already running; call wait_result first");
    BLZ_TRY(use_device(h->device));
    h->in_flight_reads = 0;
    void* b = h->buf[buf_kernel].p;
    void* s = h->scratch.p;
    BLZ_HIP(hipEventRecord(h->ev0, h->stream), BLZ_ERR_UNKNOWN);
    const void* cur = b;
    if (h->geom.logC) { BLZ_TRY(launch_pass(h, 1, cur, s)); cur = s; }
    if (h->geom.logB) { BLZ_TRY(launch_pass(h, 2, cur, s)); cur = s; }
    if (cur == b) {  // single pass: keep it out of place through the scratch
        BLZ_HIP(hipMemcpyAsync(s, b, ntt_bytes(h), hipMemcpyDeviceToDevice, h->stream), BLZ_ERR_UNKNOWN);
        cur = s;
    }
    BLZ_TRY(launch_pass(h, 3, cur, b));
    BLZ_HIP(hipEventRecord(h->ev1, h->stream), BLZ_ERR_UNKNOWN);
    h->in_flight = true;
    h->in_flight_buf = (int)buf_kernel;
    h->in_flight_buf2 = -1;
    return BLZ_OK;
}

int blz_ntt_wait_result(blz_ntt* h) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_NTT_LIVE(h);
    if (!h->in_flight) return fail(BLZ_ERR_INVALID_PARAM, "wait_result with no transform in flight");
    BLZ_TRY(use_device(h->device));
    // bounded (BLAZE_WAIT_TIMEOUT_MS): the reference polls the status register without a deadline (ntt_api.rs:89-108)
    BLZ_NTT_WAIT(h, sync_event_bounded(h->ev1, "wait_result: NTT"));
    (void)hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1);
    h->in_flight = false;
    return BLZ_OK;
}

static int ntt_result_common(blz_ntt* h, size_t buf, void* out, size_t out_cap, bool on_device) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (buf > 1) return fail(BLZ_ERR_INVALID_PARAM, "buffer index must be 0 or 1");
    if (ntt_buf_in_flight(h, buf))
        return fail(BLZ_ERR_INVALID_PARAM, "buffer %zu is being transformed; call wait_result first", buf);
    if (out_cap < ntt_bytes(h)) return fail(BLZ_ERR_INVALID_PARAM, "output buffer too small");
    BLZ_NTT_LIVE(h);
    BLZ_TRY(use_device(h->device));
    BLZ_HIP(hipMemcpyAsync(out, h->buf[buf].p, ntt_bytes(h), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           h->copy_stream), BLZ_ERR_READ);
    BLZ_NTT_WAIT(h, sync_stream_bounded(h->copy_stream, "result: copy out of the NTT buffer"));
    return BLZ_OK;
}
int blz_ntt_result(blz_ntt* h, size_t buf, uint8_t* out, size_t out_cap) { return ntt_result_common(h, buf, out, out_cap, false); }
int blz_ntt_result_device(blz_ntt* h, size_t buf, void* d_out, size_t out_cap) { return ntt_result_common(h, buf, d_out, out_cap, true); }

// result(buf) and set_data(buf) of the reference's double-buffered loop (tests/integration_ntt.rs:102-136: while the kernel runs
// on the other buffer the host READS the previous result out of `buf` and WRITES the next input into it) as ONE call that uses
// the link in both directions at once.  Called one after the other, the two copies are the whole cycle - 76 + 76.5 ms around a
// hidden 14 ms kernel at 2^27 - and each leaves the opposite direction of the full-duplex link idle.  Here the buffer goes in
// pieces: piece k leaves for prev_out on copy_stream, and as soon as it has, piece k of next_in lands in its place on
// copy_stream2, while piece k + 1 is already leaving.
//   * host buffers the runtime knows as pinned (blz_host_malloc, hipHostMalloc, hipHostRegister): every copy is a true
//     asynchronous DMA; the pieces are chained with events and the caller waits once, at the end;
//   * pageable host memory: hipMemcpyAsync returns only when the runtime has staged the copy, so the two directions are driven
//     by two host threads (the caller's: device -> host; a helper: host -> device, which waits for a piece's departure
//     through a counter).
static bool host_ptr_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary malloc'ed pointer: "invalid value"
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

int blz_ntt_exchange(blz_ntt* h, size_t buf, const uint8_t* next_in, size_t in_len, uint8_t* prev_out, size_t out_cap) {
    if (!h || !next_in || !prev_out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (buf > 1) return fail(BLZ_ERR_INVALID_PARAM, "buffer index must be 0 or 1");
    const size_t total = ntt_bytes(h);
    if (in_len != total) return fail(BLZ_ERR_INVALID_PARAM, "data length %zu != %zu", in_len, total);
    if (out_cap < total) return fail(BLZ_ERR_INVALID_PARAM, "output buffer too small");
    BLZ_NTT_LIVE(h);
    if (ntt_buf_in_flight(h, buf))
        return fail(BLZ_ERR_INVALID_PARAM, "buffer %zu is being transformed; call wait_result first", buf);
    if (h->in_flight && ((h->in_flight_reads >> buf) & 1u))
        return fail(BLZ_ERR_INVALID_PARAM, "buffer %zu is read by the element-wise op in flight; call wait_result first", buf);
    BLZ_TRY(use_device(h->device));
    char* dbuf = (char*)h->buf[buf].p;
    // Pieces of 64 MiB (1.2 ms of link; smaller ones pay more per-copy overhead than they hide: 16 MiB 93.3 ms per cycle, 64 MiB
    // 91.3, 256 MiB 93.6, 1 GiB 105.6), except at the ends: the host -> device direction can only start once the first piece has
    // left and runs alone behind the last one, so the first and the last pieces ramp 8 / 16 / 32 MiB.
    const size_t piece = (size_t)exp_knob("BLAZE_NTT_XCHG_MB", 64) << 20;
    std::vector<size_t> cut;   // piece k = bytes [cut[k], cut[k + 1])
    {
        const size_t ramp0 = exp_knob("BLAZE_NTT_XCHG_RAMP", 1) != 0 ? (size_t)8 << 20 : piece;
        std::vector<size_t> head, tail;
        size_t lo = 0, hi = total;
        for (size_t r = ramp0; r < piece && hi - lo > 4 * piece; r <<= 1) {
            head.push_back(lo);
            lo += r;
            hi -= r;
            tail.push_back(hi);
        }
        cut = head;
        for (size_t o = lo; o < hi; o += piece) cut.push_back(o);
        for (size_t i = tail.size(); i-- > 0;) cut.push_back(tail[i]);
        cut.push_back(total);
    }
    const size_t npieces = cut.size() - 1;
#ifdef BLZ_EXPERIMENT_KNOBS
    // (experiments, profiles/r05_ntt_exchange_variants.txt: a copy KERNEL for one direction instead of the copy engine)
    if (exp_knob("BLAZE_NTT_XCHG_KERNEL", 0) != 0 && host_ptr_is_pinned(next_in) && host_ptr_is_pinned(prev_out)) {
        const int mode = exp_knob("BLAZE_NTT_XCHG_KERNEL", 0);   // 1: host -> device by kernel, 2: device -> host by kernel, 3: both
        const int blocks = exp_knob("BLAZE_NTT_XCHG_BLOCKS", 64);
        for (size_t k = 0; k < npieces; ++k) {
            const size_t o = cut[k], len = cut[k + 1] - cut[k];
            hipEvent_t ev = h->xchg_ev[k % 4];
            if (mode & 2) hipLaunchKernelGGL(k_copy16, dim3(blocks), dim3(256), 0, h->copy_stream, (uint4*)(prev_out + o), (const uint4*)(dbuf + o), len / 16);
            else BLZ_HIP(hipMemcpyAsync(prev_out + o, dbuf + o, len, hipMemcpyDeviceToHost, h->copy_stream), BLZ_ERR_READ);
            BLZ_HIP(hipEventRecord(ev, h->copy_stream), BLZ_ERR_READ);
            BLZ_HIP(hipStreamWaitEvent(h->copy_stream2, ev, 0), BLZ_ERR_WRITE);
            if (mode & 1) hipLaunchKernelGGL(k_copy16, dim3(blocks), dim3(256), 0, h->copy_stream2, (uint4*)(dbuf + o), (const uint4*)(next_in + o), len / 16);
            else BLZ_HIP(hipMemcpyAsync(dbuf + o, next_in + o, len, hipMemcpyHostToDevice, h->copy_stream2), BLZ_ERR_WRITE);
        }
        BLZ_NTT_WAIT(h, sync_stream_bounded(h->copy_stream, "exchange: copy out of the NTT buffer"));
        BLZ_NTT_WAIT(h, sync_stream_bounded(h->copy_stream2, "exchange: copy into the NTT buffer"));
        return BLZ_OK;
    }
#endif
    if (exp_knob("BLAZE_NTT_XCHG_PINNED", 1) != 0 && host_ptr_is_pinned(next_in) && host_ptr_is_pinned(prev_out)) {
        // Whatever goes wrong while the pieces are being enqueued, BOTH copy streams are drained (bounded) before the call
        // returns: the header lets the caller drop next_in / prev_out on return, and pieces already enqueued keep moving bytes
        // between them and the device until they are through.
        int rc = BLZ_OK;
        std::string err;
        auto step = [&](hipError_t e, int code, const char* what) {
            if (e == hipSuccess) return true;
            (void)hipGetLastError();
            rc = code;
            err = std::string("exchange: ") + what + " failed: " + hipGetErrorString(e);
            return false;
        };
        for (size_t k = 0; k < npieces && rc == BLZ_OK; ++k) {
            const size_t o = cut[k], len = cut[k + 1] - cut[k];
            hipEvent_t ev = h->xchg_ev[k % 4];
            if (!step(hipMemcpyAsync(prev_out + o, dbuf + o, len, hipMemcpyDeviceToHost, h->copy_stream), BLZ_ERR_READ, "device -> host copy")) break;
            if (!step(hipEventRecord(ev, h->copy_stream), BLZ_ERR_READ, "event record")) break;
            if (!step(hipStreamWaitEvent(h->copy_stream2, ev, 0), BLZ_ERR_WRITE, "stream wait")) break;   // (captures this record: the event is free to be re-recorded)
            if (!step(hipMemcpyAsync(dbuf + o, next_in + o, len, hipMemcpyHostToDevice, h->copy_stream2), BLZ_ERR_WRITE, "host -> device copy")) break;
        }
        bool timed_out = false;
        std::string werr;
        int wrc = BLZ_OK;
        for (hipStream_t st : {h->copy_stream, h->copy_stream2}) {
            blz::wait_clear();
            const int r = sync_stream_bounded(st, st == h->copy_stream ? "exchange: copy out of the NTT buffer" : "exchange: copy into the NTT buffer");
            if (r != BLZ_OK) {
                if (blz::wait_timed_out()) timed_out = true;
                if (wrc == BLZ_OK) { wrc = r; werr = blz_last_error_message(); }
            }
        }
        if (timed_out) h->wedged = true;   // (bytes may still be moving: reset / free only)
        if (rc != BLZ_OK) return fail(rc, "%s", err.c_str());
        if (wrc != BLZ_OK) return fail(wrc, "%s", werr.c_str());
        return BLZ_OK;
    }
    std::atomic<size_t> departed{0};     // pieces [0, departed) are in prev_out
    std::atomic<bool> abort_in{false};
    int rc_in = BLZ_OK;
    bool timed_out_in = false;
    std::string err_in;
    const int dev = h->device;
    hipStream_t st_in = h->copy_stream2;
    auto writer_fn = [&, dev, st_in] {
        if (hipSetDevice(dev) != hipSuccess) { rc_in = BLZ_ERR_FILE; err_in = "hipSetDevice failed on the exchange's helper thread"; return; }
        for (size_t k = 0; k < npieces; ++k) {
            while (departed.load(std::memory_order_acquire) <= k) {
                if (abort_in.load(std::memory_order_acquire)) return;
                std::this_thread::yield();
            }
            const size_t o = cut[k], len = cut[k + 1] - cut[k];
            if (hipMemcpyAsync(dbuf + o, next_in + o, len, hipMemcpyHostToDevice, st_in) != hipSuccess) {
                (void)hipGetLastError();
                rc_in = BLZ_ERR_WRITE;
                err_in = "exchange: host -> device copy failed";
                return;
            }
        }
        blz::wait_clear();
        rc_in = sync_stream_bounded(st_in, "exchange: copy into the NTT buffer");
        if (rc_in != BLZ_OK) { err_in = blz_last_error_message(); timed_out_in = blz::wait_timed_out(); }
    };
    std::thread writer;
    try {
        writer = std::thread(writer_fn);
    } catch (...) {
        // no helper thread to be had (the process is at its thread limit): the two-call sequence, one direction after the other -
        // nothing may unwind across the C ABI
        BLZ_LOG(1, "exchange: no helper thread: result and set_data one after the other");
        BLZ_TRY(ntt_result_common(h, buf, prev_out, out_cap, false));
        return ntt_set_data_common(h, buf, next_in, in_len, false);
    }
    int rc_out = BLZ_OK;
    bool timed_out_out = false;
    for (size_t k = 0; k < npieces && rc_out == BLZ_OK; ++k) {
        const size_t o = cut[k], len = cut[k + 1] - cut[k];
        if (hipMemcpyAsync(prev_out + o, dbuf + o, len, hipMemcpyDeviceToHost, h->copy_stream) != hipSuccess) {
            (void)hipGetLastError();
            rc_out = fail_hip(BLZ_ERR_READ, "exchange: device -> host copy failed");
            break;
        }
        // the piece must have LEFT before its place is overwritten: a host-side wait (bounded), which pageable copies have paid already
        blz::wait_clear();
        rc_out = sync_stream_bounded(h->copy_stream, "exchange: copy out of the NTT buffer");
        if (rc_out != BLZ_OK) { timed_out_out = blz::wait_timed_out(); break; }
        departed.store(k + 1, std::memory_order_release);
    }
    if (rc_out != BLZ_OK) abort_in.store(true, std::memory_order_release);
    writer.join();
    if (timed_out_in || timed_out_out) h->wedged = true;
    if (rc_out != BLZ_OK) return rc_out;
    if (rc_in != BLZ_OK) return fail(rc_in, "%s", err_in.c_str());
    return BLZ_OK;
}

// out = {device bytes this handle holds (two transform buffers, scratch, twiddle and factor tables, a coset handle's tables), 1 when pass 2 READS its
// boundary factors from the per-element table (2^27 transforms with memory for it) / 0 when it steps them, 1 when pass 1 reads the
// column-independent boundary table, log_size}
int blz_ntt_info(blz_ntt* h, uint64_t out[4]) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    out[0] = (uint64_t)(h->buf[0].cap + h->buf[1].cap + h->scratch.cap + h->tables.cap + h->tables_rr.cap + h->table_b.cap + h->tables_cs.cap);
    out[1] = h->TR.tB ? 1u : 0u;
    out[2] = h->TR.tA ? 1u : 0u;
    out[3] = (uint64_t)h->logn;
    return BLZ_OK;
}

// Coset transforms (include/blaze_hip.h).  The shift is checked on the device (k_ntt_cs_base) BEFORE any table is touched; the
// tables that carry it - NttCoset's, and pass 2's ts2 / tB where that pass owes a part of it (ntt_engine.hpp) - are rebuilt on the
// compute stream, which is idle: a transform in flight refuses the call.
static int ntt_coset_carve(blz_ntt* h) {
    if (h->tables_cs.p) return BLZ_OK;
    NttCoset probe{};
    h->cs_wire = h->ops->coset_plan(h->geom, h->inverse, h->force_generic, probe);
    BLZ_TRY(h->tables_cs.reserve(NTT_CS_SMALL_BYTES + (h->cs_wire ? NTT_CS_WIRE_BYTES : 0), true));
    uint32_t* p = h->tables_cs.as<uint32_t>();
    h->CS.d0 = p; p += 2 * 512 * 8;   // (an inverse handle's: with n^-1, then the pure powers)
    h->CS.d1 = p; p += 512 * 8;
    h->CS.d2 = p; p += 512 * 8;
    h->CS.u0 = p; p += 512 * NTT_RR_ENTRY_DWORDS;
    h->CS.u1 = p; p += 512 * NTT_RR_ENTRY_DWORDS;
    h->CS.u2 = p; p += 512 * NTT_RR_ENTRY_DWORDS;
    h->CS.finr = p; p += 512 * NTT_RR_ENTRY_DWORDS;
    h->cs_stage = p; p += 4 * 8;
    h->CS.tG = h->cs_wire ? p : nullptr;
    return BLZ_OK;
}

int blz_ntt_set_coset(blz_ntt* h, const uint8_t* shift) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_NTT_LIVE(h);
    if (h->in_flight) return fail(BLZ_ERR_INVALID_PARAM, "a transform is running (its kernels read the tables); call wait_result first");
    static const uint8_t one[32] = {1};
    const bool plain = !shift || memcmp(shift, one, 32) == 0;
    BLZ_TRY(use_device(h->device));
    if (plain) {
        if (!h->coset) return BLZ_OK;
        if (h->CS.mode[1] == 2) {
            BLZ_TRY(h->ops->coset_unfold(h->stream, h->T, h->TR, h->geom));
            BLZ_NTT_WAIT(h, sync_stream_bounded(h->stream, "set_coset: the plain transform's tables"));
        }
        h->coset = false;
        memcpy(h->shift, one, 32);
        return BLZ_OK;
    }
    const bool fresh = !h->tables_cs.p;
    BLZ_TRY(ntt_coset_carve(h));
    uint32_t* const d_s = h->cs_stage;
    uint32_t* const d_shift = h->cs_stage + 8;
    uint32_t* const d_flag = h->cs_stage + 16;
    BLZ_HIP(hipMemsetAsync(d_flag, 0, 4, h->stream), BLZ_ERR_UNKNOWN);
    BLZ_HIP(hipMemcpyAsync(d_shift, shift, 32, hipMemcpyHostToDevice, h->stream), BLZ_ERR_WRITE);
    BLZ_TRY(h->ops->coset_check(h->stream, d_shift, d_s, d_flag, h->inverse));
    BLZ_NTT_WAIT(h, sync_stream_bounded(h->stream, "set_coset: shift check"));
    uint32_t bad = 0;
    BLZ_HIP(hipMemcpy(&bad, d_flag, 4, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    if (bad) {
        if (fresh) {   // a refused call changes nothing: not the bytes blz_ntt_info reports either
            h->tables_cs.release();
            h->CS = NttCoset{};
            h->cs_stage = nullptr;
        }
        return fail(BLZ_ERR_INVALID_PARAM, "the coset shift is not a non-zero canonical element of the field (0 < shift < r)");
    }
    (void)h->ops->coset_plan(h->geom, h->inverse, h->force_generic, h->CS);
    BLZ_TRY(h->ops->coset_tables(h->stream, h->T, h->TR, h->geom, h->CS, d_s));
    BLZ_NTT_WAIT(h, sync_stream_bounded(h->stream, "set_coset: tables"));
    h->coset = true;
    memcpy(h->shift, shift, 32);
    return BLZ_OK;
}

int blz_ntt_get_coset(blz_ntt* h, uint8_t out[32]) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_NTT_LIVE(h);
    memcpy(out, h->shift, 32);
    return BLZ_OK;
}

int blz_ntt_reset(blz_ntt* h) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_TRY(use_device(h->device));
    BLZ_TRY(sync_stream_bounded(h->stream, "reset: NTT stream"));
    BLZ_TRY(sync_stream_bounded(h->copy_stream, "reset: NTT copy stream"));
    BLZ_TRY(sync_stream_bounded(h->copy_stream2, "reset: NTT copy stream"));
    h->in_flight = false;
    h->in_flight_reads = 0;
    h->in_flight_buf2 = -1;
    h->wedged = false;
    return BLZ_OK;
}

// Ops on the transform buffers (include/blaze_hip.h: blz_ntt_vec_op, _reduce, _scan, _horner, _gather, _scatter, _spmv, _mle_*; kernels and their workspace:
// ntt_vec.hip.hpp, ntt_fold.hip.hpp, ntt_horner.hip.hpp, ntt_gather.hip.hpp, ntt_scatter.hip.hpp, ntt_spmv.hip.hpp, ntt_mle.hip.hpp).  An op runs like a transform: compute stream, ev0 .. ev1, finished by
// blz_ntt_wait_result.  Everything is checked before anything is enqueued and nothing waits for the device.  The workspace is
// `scratch`, n x 32 bytes that only a transform or an op of this handle uses - and none can be in flight.  An entry point
// checks its own arguments, then walks this protocol: begin, resolve, enqueue.
extern "C++" {   // (enqueue is a template)
struct NttVecCall {
    blz_ntt* h;
    const uint64_t n = 1ull << h->logn;
    uint32_t* const ws = h->scratch.as<uint32_t>();
    uint32_t reads = 0;   // bit b = transform buffer b is an operand
    // v == nullptr: the op does not take it; max_count: the most device words it may hold, 0: the handle's n
    struct Operand { const char* name; const blz_vec_arg* v; NttVecArg* out; uint64_t max_count = 0; };

    int begin() {
        BLZ_NTT_LIVE(h);
        if (h->in_flight) return fail(BLZ_ERR_INVALID_PARAM, "a transform or an op on the buffers is already running; call wait_result first");
        return use_device(h->device);
    }

    // The pointer half of every check: `bytes` bytes at p are device memory of the handle's device, inside one allocation, and p
    // is aligned.  who / field name the argument ("operand a" / "d_ptr"); units x unit is what would run past the end
    int device_range(const char* who, const char* field, const void* p, uint64_t bytes, unsigned align, uint64_t units, const char* unit) {
        if (((uintptr_t)p & (align - 1u)) != 0) return fail(BLZ_ERR_INVALID_PARAM, "%s: %s is not %u-byte aligned", who, field, align);
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BLZ_ERR_INVALID_PARAM, "%s: %s is not memory the runtime knows", who, field);
        }
        if (at.type != hipMemoryTypeDevice || at.device != h->device)
            return fail(BLZ_ERR_INVALID_PARAM, "%s: %s is not device memory of device %d", who, field, h->device);
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BLZ_ERR_INVALID_PARAM, "%s: %s is not inside a device allocation", who, field);
        }
        if ((const char*)p + bytes > (const char*)base + size)
            return fail(BLZ_ERR_INVALID_PARAM, "%s: %llu %s run past the end of the allocation %s points into", who,
                        (unsigned long long)units, unit, field);
        return BLZ_OK;
    }

    int operand(const char* name, const blz_vec_arg* v, NttVecArg& out, uint64_t max_count) {
        if (v->reserved != 0) return fail(BLZ_ERR_INVALID_PARAM, "operand %s: reserved must be 0", name);
        if (!v->d_ptr) {
            if (v->buf > 1) return fail(BLZ_ERR_INVALID_PARAM, "operand %s: buf must be 0 or 1", name);
            if (v->count != 0 && v->count != n)
                return fail(BLZ_ERR_INVALID_PARAM, "operand %s: a transform buffer holds %llu elements, count says %llu", name,
                            (unsigned long long)n, (unsigned long long)v->count);
            out = NttVecArg{h->buf[v->buf].as<uint32_t>(), n - 1};
            reads |= 1u << v->buf;
            return BLZ_OK;
        }
        if (v->count == 0 || (v->count & (v->count - 1)) != 0 || v->count > max_count)
            return fail(BLZ_ERR_INVALID_PARAM, "operand %s: count %llu is not a power of two in [1, %llu]", name,
                        (unsigned long long)v->count, (unsigned long long)max_count);
        char who[48];
        snprintf(who, sizeof who, "operand %s", name);
        BLZ_TRY(device_range(who, "d_ptr", v->d_ptr, v->count * 32, 16, v->count, "elements"));
        out = NttVecArg{(const uint32_t*)v->d_ptr, v->count - 1};
        return BLZ_OK;
    }

    // The operands in order, then the output words (d_out / d_total; nullptr: none): out_words x 32 bytes checked like an
    // operand's d_ptr, and kept off the words of every d_ptr operand.
    int resolve(const Operand* ops, size_t count, const char* out_name = nullptr, void* d_out = nullptr, uint64_t out_words = 1) {
        for (size_t i = 0; i < count; ++i)
            if (ops[i].v) BLZ_TRY(operand(ops[i].name, ops[i].v, *ops[i].out, ops[i].max_count ? ops[i].max_count : n));
        if (!d_out) return BLZ_OK;
        char who[48];
        snprintf(who, sizeof who, "operand %s", out_name);
        BLZ_TRY(device_range(who, "d_ptr", d_out, out_words * 32, 16, out_words, "elements"));
        for (size_t i = 0; i < count; ++i) {
            const Operand& o = ops[i];
            if (!o.v || !o.v->d_ptr) continue;
            const char *lo = (const char*)o.v->d_ptr, *hi = lo + o.v->count * 32, *q = (const char*)d_out;
            if (q < hi && q + out_words * 32 > lo) return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps the words of a d_ptr operand", out_name);
        }
        return BLZ_OK;
    }
    int resolve(std::initializer_list<Operand> ops, const char* out_name = nullptr, void* d_out = nullptr, uint64_t out_words = 1) {
        return resolve(ops.begin(), ops.size(), out_name, d_out, out_words);
    }

    // A destination that may be the caller's device words (the multilinear ops): an operand's checks - a transform buffer, or
    // `count` device words, a power of two up to n - and room for the out_len words the op writes from its start.  buf: the
    // transform buffer it names, -1 for device words; name: what the messages call it (an op with a second destination)
    int destination(const blz_vec_arg* v, uint64_t out_len, uint32_t*& words, int& buf, const char* name = "dst") {
        NttVecArg d{};
        BLZ_TRY(operand(name, v, d, n));
        if (d.mask + 1 < out_len)
            return fail(BLZ_ERR_INVALID_PARAM, "operand %s: count %llu is below the %llu words the op writes", name, (unsigned long long)(d.mask + 1),
                        (unsigned long long)out_len);
        words = const_cast<uint32_t*>(d.p);
        buf = v->d_ptr ? -1 : (int)v->buf;
        return BLZ_OK;
    }
    // the live length of a multilinear op: 2^m words, at least one pair, at most the handle's n
    int live_length(uint64_t len) const {
        if (len < 2 || (len & (len - 1)) != 0 || len > n)
            return fail(BLZ_ERR_INVALID_PARAM, "len %llu: the live length is 2^m with 2 <= len <= %llu", (unsigned long long)len, (unsigned long long)n);
        return BLZ_OK;
    }
    // [p, p + words x 32 bytes) meets [q, q + qwords x 32 bytes)
    static bool words_meet(const void* p, uint64_t words, const void* q, uint64_t qwords) {
        const char *a = (const char*)p, *b = (const char*)q;
        return a < b + qwords * 32 && b < a + words * 32;
    }

    // buf_dst: the transform buffer the op writes (dispatch is handed its words), -1: none; buf_dst2: a second one (a sumcheck
    // step whose tables are both buffers)
    template <class Dispatch>
    int enqueue(int buf_dst, Dispatch&& dispatch, int buf_dst2 = -1) {
        BLZ_HIP(hipEventRecord(h->ev0, h->stream), BLZ_ERR_UNKNOWN);
        BLZ_TRY(dispatch(buf_dst < 0 ? nullptr : h->buf[buf_dst].as<uint32_t>()));
        BLZ_HIP(hipEventRecord(h->ev1, h->stream), BLZ_ERR_UNKNOWN);
        h->in_flight = true;
        h->in_flight_buf = buf_dst;
        h->in_flight_buf2 = buf_dst2;
        // read-ONLY buffers: the written one is in_flight_buf's to refuse; a reduce writes none and keeps all its read bits
        h->in_flight_reads = buf_dst < 0 ? reads : reads & ~(1u << buf_dst);
        if (buf_dst2 >= 0) h->in_flight_reads &= ~(1u << buf_dst2);
        return BLZ_OK;
    }
};

// What blz_ntt_sumcheck_step and blz_ntt_sumcheck_gate share, behind each one's checks of its gate: the shape of points, d_out
// and r, the live length, begin, ONE resolve (the tables in order, then r, then d_out), the bind rules - with r every table is
// folded in place, so none is periodic, no two meet in their first len words, r is outside the len / 2 words a table receives
// and d_out outside a table's live words - and the enqueue with both written buffers.  tables: the k tables, none NULL, each with
// its name in a message ("a" / "tables[1]") and the slot it resolves to; one, two: what stands in front of one name and of a pair
// ("table ", "tables " / nothing).  dispatch(r's word, or nullptr) launches.
// blz_ntt_vec_mle_round does not come here: its points range, its flags and its operand rule are its own, and it binds nothing.
// extra: one more operand that is no table (blz_ntt_zerocheck_gate's weight), resolved behind r and kept off d_out as every
// operand is, or NULL; after(r's word, or nullptr): its owner's rules, checked behind the tables' and before the enqueue.
struct NttStepNoExtra {
    int operator()(const uint32_t*) const { return BLZ_OK; }
};
template <class Dispatch, class After = NttStepNoExtra>
int ntt_step_protocol(NttVecCall& call, const NttVecCall::Operand* tables, int k, const char* one, const char* two, const blz_vec_arg* r,
                      uint32_t points, uint32_t max_points, uint64_t len, void* d_out, Dispatch&& dispatch, const NttVecCall::Operand* extra = nullptr,
                      After&& after = After{}) {
    if (points > max_points) return fail(BLZ_ERR_INVALID_PARAM, "points %u is not in [0, %u]", points, max_points);
    if (points == 0 && (!r || d_out)) return fail(BLZ_ERR_INVALID_PARAM, "points 0 is a bind alone: it takes r and a NULL d_out");
    if (points > 0 && !d_out) return fail(BLZ_ERR_INVALID_PARAM, "null d_out");
    if (r && (!r->d_ptr || r->count != 1))
        return fail(BLZ_ERR_INVALID_PARAM, "a sumcheck step takes the challenge as one device word: r.d_ptr != NULL, r.count == 1");
    BLZ_TRY(call.live_length(len));
    if (r && points > 0 && len < 4) return fail(BLZ_ERR_INVALID_PARAM, "len %llu: a bind and a round need len >= 4", (unsigned long long)len);
    BLZ_TRY(call.begin());
    NttVecCall::Operand ops[BLZ_GATE_MAX_TABLES + 2];   // the tables, r and the extra operand; blz_ntt_sumcheck_step's four fit
    NttVecArg vr{};
    std::copy_n(tables, k, ops);
    ops[k] = {"r", r, &vr};
    if (extra) ops[k + 1] = *extra;
    BLZ_TRY(call.resolve(ops, (size_t)k + (extra ? 2 : 1), "d_out", d_out, points));
    int wbuf[2] = {-1, -1};
    if (r) {
        const uint64_t half = len >> 1;
        for (int j = 0; j < k; ++j) {
            const NttVecArg& tj = *ops[j].out;
            if (tj.mask + 1 < len)
                return fail(BLZ_ERR_INVALID_PARAM, "operand %s: %llu words, read periodically over len %llu: a periodic table cannot be folded in place", ops[j].name,
                            (unsigned long long)(tj.mask + 1), (unsigned long long)len);
            for (int i = 0; i < j; ++i)
                if (NttVecCall::words_meet(ops[i].out->p, len, tj.p, len))
                    return fail(BLZ_ERR_INVALID_PARAM, "%s%s and %s overlap in their first len words: each is folded in place", two, ops[i].name, ops[j].name);
            if (NttVecCall::words_meet(vr.p, 1, tj.p, half)) return fail(BLZ_ERR_INVALID_PARAM, "r lies in the words %s%s receives", one, ops[j].name);
            if (d_out && NttVecCall::words_meet(d_out, points, tj.p, len))
                return fail(BLZ_ERR_INVALID_PARAM, "d_out lies in the live words of %s%s", one, ops[j].name);
            if (!ops[j].v->d_ptr) wbuf[wbuf[0] < 0 ? 0 : 1] = (int)ops[j].v->buf;
        }
    }
    BLZ_TRY(after(r ? vr.p : nullptr));
    return call.enqueue(wbuf[0], [&](uint32_t*) { return dispatch(r ? vr.p : nullptr); }, wbuf[1]);
}
}  // extern "C++"

int blz_ntt_vec_op(blz_ntt* h, int op, size_t buf_dst, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (op < 0 || op >= NTT_VEC_OPS) return fail(BLZ_ERR_INVALID_PARAM, "unknown element-wise op %d", op);
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    const bool takes_b = op != BLZ_VEC_INV, takes_c = op == BLZ_VEC_MULADD || op == BLZ_VEC_MULSUB;
    if (!a || (b != nullptr) != takes_b || (c != nullptr) != takes_c)
        return fail(BLZ_ERR_INVALID_PARAM, "element-wise op %d takes operands a%s%s, and the others must be NULL", op, takes_b ? ", b" : "",
                    takes_c ? ", c" : "");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg va{}, vb{}, vc{};
    BLZ_TRY(call.resolve({{"a", a, &va}, {"b", b, &vb}, {"c", c, &vc}}));
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) {
        return h->ops->vec_op(h->stream, op, dst, va, takes_b ? vb : va, takes_c ? vc : va, call.n, call.ws);
    });
}

int blz_ntt_vec_reduce(blz_ntt* h, int op, const blz_vec_arg* a, const blz_vec_arg* b, void* d_out) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (op < 0 || op >= NTT_FOLD_OPS) return fail(BLZ_ERR_INVALID_PARAM, "unknown reduction %d", op);
    const bool takes_b = op != BLZ_FOLD_SUM;
    if (!a || (b != nullptr) != takes_b)
        return fail(BLZ_ERR_INVALID_PARAM, "reduction %d takes operands a%s, and the other must be NULL", op, takes_b ? ", b" : "");
    if (op == BLZ_FOLD_EVAL && (!b->d_ptr || b->count != 1))
        return fail(BLZ_ERR_INVALID_PARAM, "BLZ_FOLD_EVAL takes the point as one device word: b.d_ptr != NULL, b.count == 1");
    if (!d_out) return fail(BLZ_ERR_INVALID_PARAM, "null d_out");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg va{}, vb{};
    BLZ_TRY(call.resolve({{"a", a, &va}, {"b", b, &vb}}, "d_out", d_out));
    return call.enqueue(-1, [&](uint32_t*) { return h->ops->vec_reduce(h->stream, op, (uint32_t*)d_out, va, takes_b ? vb : va, call.n, call.ws); });
}

int blz_ntt_vec_scan(blz_ntt* h, int op, uint32_t flags, size_t buf_dst, const blz_vec_arg* a, void* d_total) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (op < 0 || op >= NTT_SCAN_OPS) return fail(BLZ_ERR_INVALID_PARAM, "unknown scan %d", op);
    if (flags & ~BLZ_SCAN_EXCLUSIVE) return fail(BLZ_ERR_INVALID_PARAM, "unknown scan flags 0x%x", flags);
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    if (!a) return fail(BLZ_ERR_INVALID_PARAM, "a scan takes operand a");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg va{};
    BLZ_TRY(call.resolve({{"a", a, &va}}, "d_total", d_total));
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) { return h->ops->vec_scan(h->stream, op, flags, dst, va, call.n, (uint32_t*)d_total, call.ws); });
}

int blz_ntt_vec_horner(blz_ntt* h, uint32_t flags, size_t buf_dst, const blz_vec_arg* a, const blz_vec_arg* z, void* d_total) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (flags & ~(BLZ_HORNER_EXCLUSIVE | BLZ_HORNER_REVERSE)) return fail(BLZ_ERR_INVALID_PARAM, "unknown weighted-scan flags 0x%x", flags);
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    if (!a || !z) return fail(BLZ_ERR_INVALID_PARAM, "a weighted scan takes operands a and z");
    if (!z->d_ptr || z->count != 1)
        return fail(BLZ_ERR_INVALID_PARAM, "a weighted scan takes the multiplier as one device word: z.d_ptr != NULL, z.count == 1");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg va{}, vz{};
    BLZ_TRY(call.resolve({{"a", a, &va}, {"z", z, &vz}}, "d_total", d_total));
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) { return h->ops->vec_horner(h->stream, flags, dst, va, vz, call.n, (uint32_t*)d_total, call.ws); });
}

// In place (a's words overlap the destination buffer) a lane would overwrite what another still reads: the gather goes into
// `scratch` and a copy on the same stream brings it back - twice the traffic, no allocation, the buffers stay where they are.
int blz_ntt_vec_gather(blz_ntt* h, size_t buf_dst, const blz_vec_arg* a, const blz_vec_view* v) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    if (!a || !v) return fail(BLZ_ERR_INVALID_PARAM, "a gather takes operand a and a view");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg va{};
    BLZ_TRY(call.resolve({{"a", a, &va, 1ull << NTT_MAX_LOG}}));
    const uint64_t count = va.mask + 1;
    if (v->offset >= count)
        return fail(BLZ_ERR_INVALID_PARAM, "view: offset %llu is not below the source's %llu elements", (unsigned long long)v->offset,
                    (unsigned long long)count);
    if (v->len > call.n)
        return fail(BLZ_ERR_INVALID_PARAM, "view: len %llu is above the handle's %llu positions", (unsigned long long)v->len,
                    (unsigned long long)call.n);
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) -> int {
        const bool in_place = va.p < dst + call.n * 8 && dst < va.p + count * 8;
        BLZ_TRY(h->ops->vec_gather(h->stream, in_place ? call.ws : dst, va, v->offset, v->stride & va.mask, v->len, call.n));
        if (in_place) BLZ_HIP(hipMemcpyAsync(dst, call.ws, ntt_bytes(h), hipMemcpyDeviceToDevice, h->stream), BLZ_ERR_UNKNOWN);
        return BLZ_OK;
    });
}

// The matrix is the caller's device memory and the host never reads it: the three arrays are checked as pointers (device_range),
// their contents are the kernels' to survive (ntt_spmv.hip.hpp).  `scratch` is the op's workspace, so x may not name buf_dst: the
// gather's detour is taken.  CSR mode zeroes the destination first - rows without a nonzero are visited by no tile.
int blz_ntt_vec_spmv(blz_ntt* h, size_t buf_dst, const blz_vec_arg* x, const blz_vec_csr* m) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    if (!x || !m) return fail(BLZ_ERR_INVALID_PARAM, "a sparse product takes operand x and a matrix m");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    const uint64_t max_nnz = std::min<uint64_t>(std::max<uint64_t>(1024, 256 * call.n), 1ull << 31);
    if (m->rows > call.n)
        return fail(BLZ_ERR_INVALID_PARAM, "matrix m: rows %llu is above the handle's %llu positions", (unsigned long long)m->rows,
                    (unsigned long long)call.n);
    if (m->nnz > max_nnz)
        return fail(BLZ_ERR_INVALID_PARAM, "matrix m: nnz %llu is above %llu (max(1024, 256 n), at most 2^31)", (unsigned long long)m->nnz,
                    (unsigned long long)max_nnz);
    if (!m->d_row_ptr && m->rows != m->nnz)
        return fail(BLZ_ERR_INVALID_PARAM, "matrix m: without d_row_ptr row p is nonzero p, but rows %llu != nnz %llu",
                    (unsigned long long)m->rows, (unsigned long long)m->nnz);
    if (!m->d_col && m->nnz > 0) return fail(BLZ_ERR_INVALID_PARAM, "matrix m: d_col is NULL with nnz %llu", (unsigned long long)m->nnz);
    NttVecArg vx{};
    BLZ_TRY(call.resolve({{"x", x, &vx, 1ull << NTT_MAX_LOG}}));
    const uint32_t* const dst_words = h->buf[buf_dst].as<uint32_t>();
    if (vx.p < dst_words + call.n * 8 && dst_words < vx.p + (vx.mask + 1) * 8)
        return fail(BLZ_ERR_INVALID_PARAM, "operand x names or overlaps buffer %zu, the destination: a sparse product cannot run in place", buf_dst);
    if (m->d_row_ptr) BLZ_TRY(call.device_range("matrix m", "d_row_ptr", m->d_row_ptr, (m->rows + 1) * 4, 4, m->rows + 1, "entries"));
    if (m->nnz > 0) BLZ_TRY(call.device_range("matrix m", "d_col", m->d_col, m->nnz * 4, 4, m->nnz, "entries"));
    if (m->d_val && m->nnz > 0) BLZ_TRY(call.device_range("matrix m", "d_val", m->d_val, m->nnz * 32, 16, m->nnz, "elements"));
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) -> int {
        const bool csr = m->d_row_ptr != nullptr;
        if (csr || m->nnz == 0) BLZ_HIP(hipMemsetAsync(dst, 0, ntt_bytes(h), h->stream), BLZ_ERR_UNKNOWN);
        if (m->nnz == 0 || m->rows == 0) return BLZ_OK;
        return h->ops->vec_spmv(h->stream, dst, vx, m->d_row_ptr, m->d_col, (const uint32_t*)m->d_val, m->rows, m->nnz, call.n, call.ws);
    });
}

// The other way round: a nonzero names the position it is added to (ntt_scatter.hip.hpp).  The arrays are the caller's device
// memory, checked as pointers like the matrix above; the destination is the accumulator and `scratch` its upper half, so x may
// not name buf_dst.  The kernels' dispatch zeroes what its mode accumulates into; without a nonzero the zeros are the result.
int blz_ntt_vec_scatter(blz_ntt* h, size_t buf_dst, const blz_vec_arg* x, const blz_vec_scatter* s) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!s) return fail(BLZ_ERR_INVALID_PARAM, "a scatter-add takes a scatter s");
    if (buf_dst > 1) return fail(BLZ_ERR_INVALID_PARAM, "buf_dst must be 0 or 1");
    if (s->reserved != 0) return fail(BLZ_ERR_INVALID_PARAM, "scatter s: reserved must be 0");
    if (s->nnz > (1ull << 31)) return fail(BLZ_ERR_INVALID_PARAM, "scatter s: nnz %llu is above 2^31", (unsigned long long)s->nnz);
    if (!s->d_idx && s->nnz > 0) return fail(BLZ_ERR_INVALID_PARAM, "scatter s: d_idx is NULL with nnz %llu", (unsigned long long)s->nnz);
    if (s->d_src && !x) return fail(BLZ_ERR_INVALID_PARAM, "scatter s: d_src is given without operand x, whose words it selects");
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg vx{};
    BLZ_TRY(call.resolve({{"x", x, &vx, 1ull << NTT_MAX_LOG}}));
    const uint32_t* const dst_words = h->buf[buf_dst].as<uint32_t>();
    if (x && vx.p < dst_words + call.n * 8 && dst_words < vx.p + (vx.mask + 1) * 8)
        return fail(BLZ_ERR_INVALID_PARAM, "operand x names or overlaps buffer %zu, the destination: a scatter-add cannot run in place", buf_dst);
    if (s->nnz > 0) BLZ_TRY(call.device_range("scatter s", "d_idx", s->d_idx, s->nnz * 4, 4, s->nnz, "entries"));
    if (s->d_src && s->nnz > 0) BLZ_TRY(call.device_range("scatter s", "d_src", s->d_src, s->nnz * 4, 4, s->nnz, "entries"));
    if (s->d_val && s->nnz > 0) BLZ_TRY(call.device_range("scatter s", "d_val", s->d_val, s->nnz * 32, 16, s->nnz, "elements"));
    return call.enqueue((int)buf_dst, [&](uint32_t* dst) -> int {
        if (s->nnz == 0) {
            BLZ_HIP(hipMemsetAsync(dst, 0, ntt_bytes(h), h->stream), BLZ_ERR_UNKNOWN);
            return BLZ_OK;
        }
        return h->ops->vec_scatter(h->stream, dst, vx, s->d_idx, s->d_src, (const uint32_t*)s->d_val, s->nnz, call.n, call.ws);
    });
}

// Multilinear tables (ntt_mle.hip.hpp).  The first ops whose destination may be the caller's device words, and the first that
// write less than a buffer: out_len words from the start of the destination and not a byte more.  In place (the destination
// starts where the source starts) the default pairing needs nothing; BLZ_MLE_LOW takes the gather's detour through `scratch`,
// len / 2 words each way.
int blz_ntt_vec_mle_fold(blz_ntt* h, uint32_t flags, const blz_vec_arg* dst, const blz_vec_arg* a, const blz_vec_arg* r, uint64_t len) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (flags & ~BLZ_MLE_LOW) return fail(BLZ_ERR_INVALID_PARAM, "unknown multilinear flags 0x%x", flags);
    if (!dst || !a || !r) return fail(BLZ_ERR_INVALID_PARAM, "a multilinear fold takes dst, a and r");
    if (!r->d_ptr || r->count != 1)
        return fail(BLZ_ERR_INVALID_PARAM, "a multilinear fold takes the challenge as one device word: r.d_ptr != NULL, r.count == 1");
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    NttVecArg va{}, vr{};
    BLZ_TRY(call.resolve({{"a", a, &va}, {"r", r, &vr}}));
    const uint64_t half = len >> 1, count = va.mask + 1;
    uint32_t* d = nullptr;
    int buf = -1;
    BLZ_TRY(call.destination(dst, half, d, buf));
    const bool in_place = d == va.p;
    if (!in_place && NttVecCall::words_meet(d, half, va.p, std::min(count, len)))
        return fail(BLZ_ERR_INVALID_PARAM, "dst overlaps the words of a without starting where they start");
    if (in_place && count < len)
        return fail(BLZ_ERR_INVALID_PARAM, "dst names a's %llu words, read periodically over len %llu: a periodic source cannot be folded in place",
                    (unsigned long long)count, (unsigned long long)len);
    if (NttVecCall::words_meet(vr.p, 1, d, half)) return fail(BLZ_ERR_INVALID_PARAM, "r lies in the words dst receives");
    return call.enqueue(buf, [&](uint32_t*) -> int {
        const bool detour = in_place && (flags & BLZ_MLE_LOW);
        BLZ_TRY(h->ops->vec_mle_fold(h->stream, flags, detour ? call.ws : d, va, vr.p, len));
        if (detour) BLZ_HIP(hipMemcpyAsync(d, call.ws, half * 32, hipMemcpyDeviceToDevice, h->stream), BLZ_ERR_UNKNOWN);
        return BLZ_OK;
    });
}

int blz_ntt_vec_mle_round(blz_ntt* h, uint32_t flags, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c, uint32_t points,
                          uint64_t len, void* d_out) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (flags & ~BLZ_MLE_LOW) return fail(BLZ_ERR_INVALID_PARAM, "unknown multilinear flags 0x%x", flags);
    if (!a || (c && !b)) return fail(BLZ_ERR_INVALID_PARAM, "a round polynomial takes operands a, then b, then c: %s", !a ? "a is NULL" : "b is NULL while c is set");
    if (points < 1 || points > 4) return fail(BLZ_ERR_INVALID_PARAM, "points %u is not in [1, 4]", points);
    if (!d_out) return fail(BLZ_ERR_INVALID_PARAM, "null d_out");
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    NttVecArg va{}, vb{}, vc{};
    BLZ_TRY(call.resolve({{"a", a, &va}, {"b", b, &vb}, {"c", c, &vc}}, "d_out", d_out, points));
    const int k = c ? 3 : b ? 2 : 1;
    const NttVecArg vt[3] = {va, vb, vc};
    return call.enqueue(-1, [&](uint32_t*) {
        return h->ops->sumcheck_step(h->stream, BLZ_GATE_PRODUCT, flags, k, vt, nullptr, points, len, (uint32_t*)d_out, call.ws);
    });
}

int blz_ntt_vec_mle_eq(blz_ntt* h, const blz_vec_arg* dst, const void* d_point, uint32_t m) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!dst) return fail(BLZ_ERR_INVALID_PARAM, "an equality table takes dst");
    if (m > (uint32_t)h->logn) return fail(BLZ_ERR_INVALID_PARAM, "m %u is above the handle's log_size %d", m, h->logn);
    if (!d_point && m > 0) return fail(BLZ_ERR_INVALID_PARAM, "null d_point with m %u", m);
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    const uint64_t out_len = 1ull << m;
    uint32_t* d = nullptr;
    int buf = -1;
    BLZ_TRY(call.destination(dst, out_len, d, buf));
    if (m > 0) {
        BLZ_TRY(call.device_range("the point", "d_point", d_point, (uint64_t)m * 32, 16, m, "elements"));
        if (NttVecCall::words_meet(d_point, m, d, out_len)) return fail(BLZ_ERR_INVALID_PARAM, "d_point lies in the words dst receives");
    }
    return call.enqueue(buf, [&](uint32_t*) { return h->ops->vec_mle_eq(h->stream, d, (const uint32_t*)d_point, m, call.ws); });
}

int blz_ntt_stream(blz_ntt* h, void** hip_stream, int* device_id) {
    if (!h || !hip_stream) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (device_id) *device_id = h->device;
    *hip_stream = (void*)h->stream;
    return BLZ_OK;
}

// A sumcheck step (ntt_sumcheck.hip.hpp): with r every table is folded in place and the round polynomial is taken of the
// folded tables in the same pass; without r the round alone; points == 0 the folds alone.  With r BOTH transform buffers may be
// tables and are then both written: the second is recorded in in_flight_buf2.
int blz_ntt_sumcheck_step(blz_ntt* h, uint32_t gate, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c, const blz_vec_arg* d,
                          const blz_vec_arg* r, uint32_t points, uint64_t len, void* d_out) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (gate != BLZ_GATE_PRODUCT && gate != BLZ_GATE_R1CS) return fail(BLZ_ERR_INVALID_PARAM, "unknown gate %u", gate);
    const blz_vec_arg* const tv[4] = {a, b, c, d};
    int k = 0;
    while (k < 4 && tv[k]) ++k;
    for (int j = k; j < 4; ++j)
        if (tv[j]) return fail(BLZ_ERR_INVALID_PARAM, "a gate takes its tables as a, then b, then c, then d: %c is NULL while %c is set", 'a' + k, 'a' + j);
    if (gate == BLZ_GATE_R1CS ? k != 4 : (k < 1 || k > 3))
        return fail(BLZ_ERR_INVALID_PARAM, "%s, %d given", gate == BLZ_GATE_R1CS ? "BLZ_GATE_R1CS takes the four tables a, b, c, d" : "BLZ_GATE_PRODUCT takes 1 to 3 tables (d must be NULL)", k);
    NttVecCall call{h};
    NttVecArg vt[4]{};
    const NttVecCall::Operand tables[4] = {{"a", a, &vt[0]}, {"b", b, &vt[1]}, {"c", c, &vt[2]}, {"d", d, &vt[3]}};
    return ntt_step_protocol(call, tables, k, "table ", "tables ", r, points, 4, len, d_out, [&](const uint32_t* rw) {
        return h->ops->sumcheck_step(h->stream, gate, 0, k, vt, rw, points, len, (uint32_t*)d_out, call.ws);
    });
}

// A caller-defined gate's description (blz_sum_gate), checked and packed for the kernels - the longest term's length F, each
// term's deficit F - nfactors, the close power - for both entry points that take one: blz_ntt_sumcheck_gate and
// blz_ntt_gate_eval.  g's tables are the caller's to resolve.
extern "C++" {
static int ntt_gate_describe(const blz_sum_gate* gate, NttGate& g) {
    if (gate->ntables < 1 || gate->ntables > BLZ_GATE_MAX_TABLES) return fail(BLZ_ERR_INVALID_PARAM, "gate: ntables %u is not in [1, %d]", gate->ntables, BLZ_GATE_MAX_TABLES);
    if (gate->nterms < 1 || gate->nterms > BLZ_GATE_MAX_TERMS) return fail(BLZ_ERR_INVALID_PARAM, "gate: nterms %u is not in [1, %d]", gate->nterms, BLZ_GATE_MAX_TERMS);
    if (gate->common < -1 || gate->common >= (int32_t)gate->ntables)
        return fail(BLZ_ERR_INVALID_PARAM, "gate: common %d is neither -1 nor a table index below ntables %u", gate->common, gate->ntables);
    if (gate->reserved != 0) return fail(BLZ_ERR_INVALID_PARAM, "gate: reserved must be 0");
    g = NttGate{};
    g.ntables = gate->ntables;
    g.nterms = gate->nterms;
    g.common = gate->common;
    uint32_t longest = 0;
    for (uint32_t m = 0; m < gate->nterms; ++m) {
        const blz_gate_term& t = gate->term[m];
        if (t.nfactors < 1 || t.nfactors > BLZ_GATE_MAX_FACTORS) return fail(BLZ_ERR_INVALID_PARAM, "gate: term %u: nfactors %u is not in [1, %d]", m, t.nfactors, BLZ_GATE_MAX_FACTORS);
        if (t.negate > 1) return fail(BLZ_ERR_INVALID_PARAM, "gate: term %u: negate %u is not 0 or 1", m, t.negate);
        if (t.reserved[0] != 0 || t.reserved[1] != 0) return fail(BLZ_ERR_INVALID_PARAM, "gate: term %u: reserved must be 0", m);
        for (uint32_t j = 0; j < t.nfactors; ++j)
            if (t.factor[j] >= gate->ntables)
                return fail(BLZ_ERR_INVALID_PARAM, "gate: term %u: factor %u names table %u, ntables is %u", m, j, t.factor[j], gate->ntables);
        if (t.nfactors > longest) longest = t.nfactors;
    }
    for (uint32_t m = 0; m < gate->nterms; ++m) {
        const blz_gate_term& t = gate->term[m];
        g.term[m] = t.nfactors | (uint32_t)t.negate << 3 | (longest - t.nfactors) << 4;
        for (uint32_t j = 0; j < t.nfactors; ++j) g.term[m] |= (uint32_t)t.factor[j] << (8 + 4 * j);
    }
    g.close_k = longest + (gate->common >= 0 ? 1u : 0u);
    return BLZ_OK;
}
// blz_ntt_zerocheck_gate's gate is blz_ntt_sumcheck_gate's - same struct, same limits, same messages: the same function under the
// name of the third entry point that takes one
static constexpr auto ntt_zerocheck_describe = &ntt_gate_describe;
// the gate's tables as operands "tables[j]" that resolve into g.t[j]
struct NttGateTables {
    char name[BLZ_LIN_MAX_TABLES][16];
    NttVecCall::Operand ops[BLZ_LIN_MAX_TABLES];
    NttGateTables(NttGate& g, const blz_vec_arg* tables) : NttGateTables(g.t, g.ntables, tables) {}
    NttGateTables(NttVecArg* t, uint32_t ntables, const blz_vec_arg* tables) {
        for (uint32_t j = 0; j < ntables; ++j) {
            snprintf(name[j], sizeof name[j], "tables[%u]", j);
            ops[j] = {name[j], tables + j, &t[j]};
        }
    }
};
// An evaluated gate's in-place rule, for blz_ntt_gate_eval and blz_ntt_gate_eval_lin: rots[j] = rot[j] (rot NULL: 0), and a table
// that meets the len words at d starts there, holds them all and is not rotated
static int ntt_gate_in_place(const uint32_t* d, uint64_t len, const NttVecArg* t, const NttGateTables& names, uint32_t ntables, const uint64_t* rot,
                             uint64_t* rots) {
    for (uint32_t j = 0; j < ntables; ++j) {
        rots[j] = rot ? rot[j] : 0;
        const uint64_t count = t[j].mask + 1;
        if (!NttVecCall::words_meet(d, len, t[j].p, count)) continue;
        if (t[j].p != d) return fail(BLZ_ERR_INVALID_PARAM, "dst overlaps the words of %s without starting where they start", names.name[j]);
        if (count < len)
            return fail(BLZ_ERR_INVALID_PARAM, "dst names the %llu words of %s, read periodically over len %llu: a periodic table cannot be written in place",
                        (unsigned long long)count, names.name[j], (unsigned long long)len);
        if (rots[j] != 0)
            return fail(BLZ_ERR_INVALID_PARAM, "dst names the words of %s, which is rotated by %llu: a table written in place has rot 0", names.name[j],
                        (unsigned long long)rots[j]);
    }
    return BLZ_OK;
}

// A gate with linear-form factors (blz_lin_gate), checked and packed for k_lineval (NttLinGate).  Every form is checked, named
// by a term or not; coef_tables gathers the coefficients of the forms that are named.  g's tables are the caller's to resolve.
static int ntt_lin_gate_describe(const blz_lin_gate* gate, NttLinGate& g) {
    if (gate->ntables < 1 || gate->ntables > BLZ_LIN_MAX_TABLES)
        return fail(BLZ_ERR_INVALID_PARAM, "lin gate: ntables %u is outside [1, %d]", gate->ntables, BLZ_LIN_MAX_TABLES);
    if (gate->nterms < 1 || gate->nterms > BLZ_GATE_MAX_TERMS)
        return fail(BLZ_ERR_INVALID_PARAM, "lin gate: nterms %u is outside [1, %d]", gate->nterms, BLZ_GATE_MAX_TERMS);
    if (gate->nforms > BLZ_LIN_MAX_FORMS) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: nforms %u is above %d", gate->nforms, BLZ_LIN_MAX_FORMS);
    // a factor byte or common: a table index below ntables, or BLZ_LIN_FORM | k with k below nforms
    auto names = [&](uint32_t f) { return f < BLZ_LIN_FORM ? f < gate->ntables : f - BLZ_LIN_FORM < gate->nforms; };
    if (gate->common != -1 && (gate->common < 0 || gate->common > 0xFF || !names((uint32_t)gate->common)))
        return fail(BLZ_ERR_INVALID_PARAM, "lin gate: common %d is not -1, a table index below ntables %u or BLZ_LIN_FORM | k with k below nforms %u",
                    gate->common, gate->ntables, gate->nforms);
    g = NttLinGate{};
    g.ntables = gate->ntables;
    g.nterms = gate->nterms;
    g.common = gate->common;
    uint32_t used = gate->common >= (int32_t)BLZ_LIN_FORM ? 1u << (gate->common - BLZ_LIN_FORM) : 0u;   // the forms that are evaluated
    for (uint32_t m = 0; m < gate->nterms; ++m) {
        const blz_gate_term& t = gate->term[m];
        if (t.nfactors < 1 || t.nfactors > BLZ_GATE_MAX_FACTORS)
            return fail(BLZ_ERR_INVALID_PARAM, "lin gate: term[%u]: nfactors %u is outside [1, %d]", m, t.nfactors, BLZ_GATE_MAX_FACTORS);
        if (t.negate > 1) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: term[%u]: negate %u is neither 0 nor 1", m, t.negate);
        if (t.reserved[0] != 0 || t.reserved[1] != 0) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: term[%u]: a reserved byte is not 0", m);
        g.term_hdr[m] = t.nfactors | (uint32_t)t.negate << 3;
        for (uint32_t j = 0; j < t.nfactors; ++j) {
            const uint32_t f = t.factor[j];
            if (!names(f))
                return f < BLZ_LIN_FORM ? fail(BLZ_ERR_INVALID_PARAM, "lin gate: term[%u]: factor %u names tables[%u], ntables is %u", m, j, f, gate->ntables)
                                        : fail(BLZ_ERR_INVALID_PARAM, "lin gate: term[%u]: factor %u names form[%u], nforms is %u", m, j, f - BLZ_LIN_FORM, gate->nforms);
            if (f >= BLZ_LIN_FORM) used |= 1u << (f - BLZ_LIN_FORM);
            g.term_fac[m] |= f << (8 * j);
        }
    }
    for (uint32_t k = 0; k < gate->nforms; ++k) {
        const blz_lin_form& l = gate->form[k];
        if (l.nsummands < 1 || l.nsummands > BLZ_LIN_MAX_SUMMANDS)
            return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: nsummands %u is outside [1, %d]", k, l.nsummands, BLZ_LIN_MAX_SUMMANDS);
        if (l.reserved[0] != 0 || l.reserved[1] != 0 || l.reserved[2] != 0) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: a reserved byte is not 0", k);
        g.form_n[k] = l.nsummands;
        for (uint32_t s = 0; s < l.nsummands; ++s) {
            const blz_lin_summand& x = l.summand[s];
            if (x.table >= gate->ntables)
                return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: summand %u names tables[%u], ntables is %u", k, s, x.table, gate->ntables);
            if (x.coef != BLZ_LIN_NO_COEF && x.coef >= gate->ntables)
                return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: summand %u takes its coefficient from tables[%u], ntables is %u", k, s, x.coef, gate->ntables);
            if (x.negate > 1) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: summand %u: negate %u is neither 0 nor 1", k, s, x.negate);
            if (x.reserved != 0) return fail(BLZ_ERR_INVALID_PARAM, "lin gate: form[%u]: summand %u: the reserved byte is not 0", k, s);
            g.form[k][s] = x.table | (uint32_t)x.coef << 8 | (uint32_t)x.negate << 16;
            if (x.coef != BLZ_LIN_NO_COEF && ((used >> k) & 1u)) g.coef_tables |= 1u << x.coef;
        }
    }
    return BLZ_OK;
}
}  // extern "C++"

// The step for a caller-defined gate (ntt_gate.hip.hpp).  The description travels to the kernel by value; the tables then walk
// blz_ntt_sumcheck_step's protocol as tables[0 .. ntables).
int blz_ntt_sumcheck_gate(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* r, uint32_t points, uint64_t len,
                          void* d_out) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!gate || !tables) return fail(BLZ_ERR_INVALID_PARAM, "a gate step takes %s", !gate ? "a gate: gate is NULL" : "the gate's tables: tables is NULL");
    NttGate g;
    BLZ_TRY(ntt_gate_describe(gate, g));
    const int nt = (int)gate->ntables;
    NttGateTables t(g, tables);
    NttVecCall call{h};
    return ntt_step_protocol(call, t.ops, nt, "", "", r, points, BLZ_GATE_MAX_POINTS, len, d_out, [&](const uint32_t* rw) {
        return h->ops->sumcheck_gate(h->stream, g, rw, points, len, (uint32_t*)d_out, call.ws);
    });
}

// The gate step of a zerocheck (ntt_zerocheck.hip.hpp): blz_ntt_sumcheck_gate's walk with the weight as the protocol's extra
// operand.  The weight is the caller's device words and no table: it is summed, not folded, so its rules are checked here, behind
// the tables' - with r it holds the len / 2 words the step reads, they meet no table's first len words, and r is outside the
// len / 4 it receives.  (d_out is off all its words in every mode: the protocol's d_ptr-operand rule.)
int blz_ntt_zerocheck_gate(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* weight, const blz_vec_arg* r,
                           uint32_t points, uint64_t len, void* d_out) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!gate || !tables || !weight)
        return fail(BLZ_ERR_INVALID_PARAM, "a zerocheck step takes %s",
                    !gate ? "a gate: gate is NULL" : !tables ? "the gate's tables: tables is NULL" : "a weight table: weight is NULL");
    NttGate g;
    BLZ_TRY(ntt_zerocheck_describe(gate, g));
    if (points == 0)
        return fail(BLZ_ERR_INVALID_PARAM, "points 0: a zerocheck step takes a round; the bind alone has no weight and is blz_ntt_sumcheck_gate's");
    if (!weight->d_ptr) return fail(BLZ_ERR_INVALID_PARAM, "operand weight: the weight is device words (d_ptr != NULL), not a transform buffer");
    const int nt = (int)gate->ntables;
    NttGateTables t(g, tables);
    NttVecCall call{h};
    NttVecArg vw{};
    const NttVecCall::Operand w{"weight", weight, &vw};
    return ntt_step_protocol(
        call, t.ops, nt, "", "", r, points, BLZ_GATE_MAX_POINTS, len, d_out,
        [&](const uint32_t* rw) { return h->ops->zerocheck_gate(h->stream, g, vw, rw, points, len, (uint32_t*)d_out, call.ws); }, &w,
        [&](const uint32_t* rw) {
            if (!rw) return (int)BLZ_OK;
            if (vw.mask + 1 < len / 2)
                return fail(BLZ_ERR_INVALID_PARAM, "operand weight: %llu words, a step with r sums len / 2 = %llu", (unsigned long long)(vw.mask + 1),
                            (unsigned long long)(len / 2));
            for (int j = 0; j < nt; ++j)
                if (NttVecCall::words_meet(vw.p, len / 2, g.t[j].p, len))
                    return fail(BLZ_ERR_INVALID_PARAM, "the weight's first len / 2 words meet the first len words of %s, which is folded in place", t.name[j]);
            if (NttVecCall::words_meet(rw, 1, vw.p, len / 4)) return fail(BLZ_ERR_INVALID_PARAM, "r lies in the words the weight receives");
            return (int)BLZ_OK;
        });
}

// The same description evaluated at every position (ntt_geval.hip.hpp): the first op that writes a destination from up to twelve
// operands.  dst follows blz_ntt_vec_mle_fold's destination rule and may be one of the tables where a lane reads only the
// position it writes: the table starts where dst starts, holds the len words and is not rotated.
int blz_ntt_gate_eval(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* dst, const blz_vec_arg* tables, const uint64_t* rot, uint64_t len) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!gate || !dst || !tables)
        return fail(BLZ_ERR_INVALID_PARAM, "a gate evaluation takes %s", !gate ? "a gate: gate is NULL" : !dst ? "a destination: dst is NULL" : "the gate's tables: tables is NULL");
    NttGate g;
    BLZ_TRY(ntt_gate_describe(gate, g));
    NttGateTables t(g, tables);
    NttVecCall call{h};
    if (len < 1 || len > call.n)
        return fail(BLZ_ERR_INVALID_PARAM, "len %llu: a gate evaluation writes 1 <= len <= %llu words", (unsigned long long)len, (unsigned long long)call.n);
    BLZ_TRY(call.begin());
    BLZ_TRY(call.resolve(t.ops, g.ntables));
    uint32_t* d = nullptr;
    int buf = -1;
    BLZ_TRY(call.destination(dst, len, d, buf));
    uint64_t rots[BLZ_GATE_MAX_TABLES] = {};
    BLZ_TRY(ntt_gate_in_place(d, len, g.t, t, g.ntables, rot, rots));
    return call.enqueue(buf, [&](uint32_t*) { return h->ops->gate_eval(h->stream, d, g, rots, len); });
}

// A gate whose factors may be linear forms, evaluated at every position (ntt_lineval.hip.hpp): blz_ntt_gate_eval's walk over
// blz_lin_gate and up to sixteen tables.  The in-place rule looks at every table, whatever names it.
int blz_ntt_gate_eval_lin(blz_ntt* h, const blz_lin_gate* gate, const blz_vec_arg* dst, const blz_vec_arg* tables, const uint64_t* rot, uint64_t len) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!gate || !dst || !tables)
        return fail(BLZ_ERR_INVALID_PARAM, "a gate evaluation with linear forms takes %s",
                    !gate ? "a gate: gate is NULL" : !dst ? "a destination: dst is NULL" : "the gate's tables: tables is NULL");
    NttLinGate g;
    BLZ_TRY(ntt_lin_gate_describe(gate, g));
    NttGateTables t(g.t, g.ntables, tables);
    NttVecCall call{h};
    if (len < 1 || len > call.n)
        return fail(BLZ_ERR_INVALID_PARAM, "len %llu: a gate evaluation with linear forms writes 1 <= len <= %llu words", (unsigned long long)len,
                    (unsigned long long)call.n);
    BLZ_TRY(call.begin());
    BLZ_TRY(call.resolve(t.ops, g.ntables));
    uint32_t* d = nullptr;
    int buf = -1;
    BLZ_TRY(call.destination(dst, len, d, buf));
    uint64_t rots[BLZ_LIN_MAX_TABLES] = {};
    BLZ_TRY(ntt_gate_in_place(d, len, g.t, t, g.ntables, rot, rots));
    return call.enqueue(buf, [&](uint32_t*) { return h->ops->gate_eval_lin(h->stream, d, g, rots, len); });
}

// Product and fraction trees (ntt_tree.hip.hpp): every layer under len words, len - 1 words into each destination by
// blz_ntt_vec_mle_fold's destination rule.  The first op with two destinations: both may be transform buffers (enqueue's
// buf_dst2).  A later launch reads what an earlier one wrote, so there is no in-place form: a destination meets neither the words
// read of a source nor the other destination.
int blz_ntt_mle_tree(blz_ntt* h, uint32_t op, uint32_t flags, const blz_vec_arg* dst, const blz_vec_arg* dst_q, const blz_vec_arg* a,
                     const blz_vec_arg* a_q, uint64_t len) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (op != BLZ_TREE_PROD && op != BLZ_TREE_FRAC) return fail(BLZ_ERR_INVALID_PARAM, "unknown tree op %u", op);
    if (flags & ~BLZ_MLE_LOW) return fail(BLZ_ERR_INVALID_PARAM, "unknown multilinear flags 0x%x", flags);
    const bool frac = op == BLZ_TREE_FRAC;
    if (!dst || !a || (dst_q != nullptr) != frac || (a_q != nullptr) != frac)
        return fail(BLZ_ERR_INVALID_PARAM, "%s", frac ? "a fraction tree takes dst, dst_q, a and a_q" : "a product tree takes dst and a, and dst_q and a_q must be NULL");
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    NttVecArg src[2] = {};
    BLZ_TRY(call.resolve({{"a", a, &src[0]}, {"a_q", a_q, &src[1]}}));
    const uint64_t out_len = len - 1;
    const int k = frac ? 2 : 1;
    const blz_vec_arg* const dv[2] = {dst, dst_q};
    static const char* const dname[2] = {"dst", "dst_q"};
    static const char* const sname[2] = {"a", "a_q"};
    uint32_t* d[2] = {nullptr, nullptr};
    int buf[2] = {-1, -1};
    for (int i = 0; i < k; ++i) {
        BLZ_TRY(call.destination(dv[i], out_len, d[i], buf[i], dname[i]));
        for (int j = 0; j < k; ++j)
            if (NttVecCall::words_meet(d[i], out_len, src[j].p, std::min(src[j].mask + 1, len)))
                return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps the words read of %s: a tree is not built in place", dname[i], sname[j]);
    }
    if (frac && NttVecCall::words_meet(d[0], out_len, d[1], out_len)) return fail(BLZ_ERR_INVALID_PARAM, "dst and dst_q overlap in the words they receive");
    // enqueue's first buffer is the one it hands out and may not be -1 beside a second: a lone buffer goes first
    if (buf[0] < 0) std::swap(buf[0], buf[1]);
    return call.enqueue(buf[0], [&](uint32_t*) { return h->ops->mle_tree(h->stream, op, flags, d[0], d[1], src[0], src[1], len); }, buf[1]);
}

// The transcript step (ntt_fs.hip.hpp): SHA3-256 of the state and `count` words as stored, the digest back into the state and,
// masked below the modulus' top bit, into d_r.  An op like any other: it reads `words` (a buffer it names is read-only while it
// is in flight) and writes no transform buffer.
static uint32_t ntt_fs_keep_bits(int field) { return field == BLZ_BLS377 ? 252u : field == BLZ_BN254 ? 253u : 254u; }

int blz_ntt_fs_challenge(blz_ntt* h, void* d_state, const blz_vec_arg* words, uint32_t count, void* d_r) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!d_state) return fail(BLZ_ERR_INVALID_PARAM, "null d_state");
    if (count > FS_MAX_WORDS) return fail(BLZ_ERR_INVALID_PARAM, "count %u is not in [0, %u]", count, FS_MAX_WORDS);
    if (count > 0 && !words) return fail(BLZ_ERR_INVALID_PARAM, "a transcript step that absorbs %u words takes them: words is NULL", count);
    NttVecCall call{h};
    BLZ_TRY(call.begin());
    NttVecArg vw{};
    if (count > 0) {
        BLZ_TRY(call.resolve({{"words", words, &vw}}));
        if (vw.mask + 1 < count)
            return fail(BLZ_ERR_INVALID_PARAM, "operand words: %llu words, the transcript absorbs the first %u as stored", (unsigned long long)(vw.mask + 1), count);
    }
    BLZ_TRY(call.device_range("the transcript", "d_state", d_state, 32, 16, 1, "elements"));
    if (d_r) {
        BLZ_TRY(call.device_range("the challenge", "d_r", d_r, 32, 16, 1, "elements"));
        if (NttVecCall::words_meet(d_r, 1, d_state, 1)) return fail(BLZ_ERR_INVALID_PARAM, "d_r overlaps d_state");
    }
    if (count > 0) {
        if (NttVecCall::words_meet(d_state, 1, vw.p, count)) return fail(BLZ_ERR_INVALID_PARAM, "d_state lies in the words absorbed");
        if (d_r && NttVecCall::words_meet(d_r, 1, vw.p, count)) return fail(BLZ_ERR_INVALID_PARAM, "d_r lies in the words absorbed");
    }
    return call.enqueue(-1, [&](uint32_t*) { return ntt_fs_absorb(h->stream, d_state, vw.p, count, d_r, ntt_fs_keep_bits(h->field)); });
}

// A whole sumcheck in one enqueue: the round alone, then per variable the transcript step over the row just written and - but
// for the last - the step with that challenge, then the bind alone; weight == NULL takes blz_ntt_sumcheck_gate's steps, else
// blz_ntt_zerocheck_gate's.  Every launch goes to the compute stream behind the one before it, so nothing waits for the host.
// Every rule a step of the chain would check is checked here, for the whole chain, before the first launch: the bind rules hold
// from round 0 (no periodic table, no two tables meeting in their first len words), the weight's are the zerocheck step's, and
// the three outputs - which are every step's d_out and r - lie off every table, off the weight and off each other.
// (the description check is blz_ntt_sumcheck_gate's own function, reached as blz_ntt_zerocheck_gate reaches it)
static constexpr auto ntt_prove_describe = &ntt_gate_describe;
int blz_ntt_sumcheck_prove(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* weight, uint32_t points, uint64_t len,
                           void* d_state, void* d_rounds, void* d_challenges) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (!gate || !tables || !d_state || !d_rounds || !d_challenges)
        return fail(BLZ_ERR_INVALID_PARAM, "a one-call prover takes %s",
                    !gate ? "a gate: gate is NULL" : !tables ? "the gate's tables: tables is NULL" : !d_state ? "a transcript: d_state is NULL"
                    : !d_rounds ? "room for the rounds: d_rounds is NULL" : "room for the challenges: d_challenges is NULL");
    NttGate g;
    BLZ_TRY(ntt_prove_describe(gate, g));
    if (points < 1 || points > BLZ_GATE_MAX_POINTS) return fail(BLZ_ERR_INVALID_PARAM, "points %u is not in [1, %u]", points, BLZ_GATE_MAX_POINTS);
    if (weight && !weight->d_ptr) return fail(BLZ_ERR_INVALID_PARAM, "operand weight: the weight is device words (d_ptr != NULL), not a transform buffer");
    const int nt = (int)gate->ntables;
    NttGateTables t(g, tables);
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    NttVecArg vw{};
    NttVecCall::Operand ops[BLZ_GATE_MAX_TABLES + 1];
    std::copy_n(t.ops, nt, ops);
    ops[nt] = {"weight", weight, &vw};
    BLZ_TRY(call.resolve(ops, (size_t)nt + 1));
    uint32_t m = 0;   // log2 len
    while ((len >> m) > 1) ++m;
    int wbuf[2] = {-1, -1};
    for (int j = 0; j < nt; ++j) {
        if (g.t[j].mask + 1 < len)
            return fail(BLZ_ERR_INVALID_PARAM, "operand %s: %llu words, read periodically over len %llu: the chain folds every table in place, so none is periodic", t.name[j],
                        (unsigned long long)(g.t[j].mask + 1), (unsigned long long)len);
        for (int i = 0; i < j; ++i)
            if (NttVecCall::words_meet(g.t[i].p, len, g.t[j].p, len))
                return fail(BLZ_ERR_INVALID_PARAM, "%s and %s meet in their first len words: the chain folds each in place", t.name[i], t.name[j]);
        if (!tables[j].d_ptr) wbuf[wbuf[0] < 0 ? 0 : 1] = (int)tables[j].buf;
    }
    if (weight) {
        if (vw.mask + 1 < len / 2)
            return fail(BLZ_ERR_INVALID_PARAM, "operand weight: %llu words, a step with r sums len / 2 = %llu", (unsigned long long)(vw.mask + 1),
                        (unsigned long long)(len / 2));
        for (int j = 0; j < nt; ++j)
            if (NttVecCall::words_meet(vw.p, len / 2, g.t[j].p, len))
                return fail(BLZ_ERR_INVALID_PARAM, "the weight's first len / 2 words meet the first len words of %s, which is folded in place", t.name[j]);
    }
    struct Output { const char* name; void* p; uint64_t words; };
    const Output out[3] = {{"d_state", d_state, 1}, {"d_rounds", d_rounds, (uint64_t)m * points}, {"d_challenges", d_challenges, m}};
    for (int o = 0; o < 3; ++o) {
        BLZ_TRY(call.device_range(out[o].name, "the pointer", out[o].p, out[o].words * 32, 16, out[o].words, "elements"));
        for (int j = 0; j < nt; ++j)
            if (NttVecCall::words_meet(out[o].p, out[o].words, g.t[j].p, len))
                return fail(BLZ_ERR_INVALID_PARAM, "%s lies in the live words of %s", out[o].name, t.name[j]);
        if (weight && NttVecCall::words_meet(out[o].p, out[o].words, vw.p, vw.mask + 1))
            return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps the words of the weight", out[o].name);
        for (int i = 0; i < o; ++i)
            if (NttVecCall::words_meet(out[i].p, out[i].words, out[o].p, out[o].words))
                return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps %s", out[o].name, out[i].name);
    }
    uint32_t* const rounds = (uint32_t*)d_rounds;
    uint32_t* const chal = (uint32_t*)d_challenges;
    const uint32_t keep = ntt_fs_keep_bits(h->field);
    auto step = [&](const uint32_t* r, uint32_t pts, uint64_t live, uint32_t* to) {
        return weight && pts ? h->ops->zerocheck_gate(h->stream, g, vw, r, pts, live, to, call.ws) : h->ops->sumcheck_gate(h->stream, g, r, pts, live, to, call.ws);
    };
    return call.enqueue(wbuf[0], [&](uint32_t*) {
        BLZ_TRY(step(nullptr, points, len, rounds));
        for (uint32_t i = 0; i < m; ++i) {
            BLZ_TRY(ntt_fs_absorb(h->stream, d_state, rounds + (size_t)i * points * 8, points, chal + (size_t)i * 8, keep));
            if (i + 1 < m) BLZ_TRY(step(chal + (size_t)i * 8, points, len >> i, rounds + (size_t)(i + 1) * points * 8));
        }
        return step(chal + (size_t)(m - 1) * 8, 0, 2, nullptr);
    }, wbuf[1]);
}

// The GKR grand product over blz_ntt_mle_tree's layers in one enqueue (include/blaze_hip.h, THE ONE-CALL GKR PROVER; kernels:
// ntt_gkr.hip.hpp).  From the root down, layer j's tables are the two halves of layer m - 1 - j of the tree (of the leaves for
// j = m - 1), its point is row j - 1 of d_points and its weight eq over that point's first j - 1 words; its sumcheck is the chain
// blz_ntt_sumcheck_prove enqueues under a weight, with the challenges written backwards into row j of d_points, and behind it the
// two final words go to d_claims and through one more transcript step.  Every launch goes to the compute stream behind the one
// before it.  BLZ_GKR_UNFUSED takes the existing launchers alone (and k_gkr_claims, a copy of two words); without it the rounds
// at live lengths of 512 and below - all of them for m <= 10 - run inside one block, h->ops->gkr_tail.  Every check stands before
// the first launch.
// (the layer gate lo hi is packed by blz_ntt_sumcheck_gate's own function, reached as blz_ntt_sumcheck_prove reaches it)
static constexpr auto ntt_gkr_describe = &ntt_gate_describe;
int blz_ntt_gkr_prove(blz_ntt* h, uint32_t op, uint32_t flags, const blz_vec_arg* tree, const blz_vec_arg* a, uint64_t len, void* d_weight,
                      void* d_state, void* d_rounds, void* d_points, void* d_claims) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (op == BLZ_TREE_FRAC)
        return fail(BLZ_ERR_INVALID_PARAM, "BLZ_TREE_FRAC is not built: the one-call GKR prover takes BLZ_TREE_PROD (a fraction tree's layer gate needs a scalar that is not folded)");
    if (op != BLZ_TREE_PROD) return fail(BLZ_ERR_INVALID_PARAM, "unknown tree op %u", op);
    if (flags & ~BLZ_GKR_UNFUSED) return fail(BLZ_ERR_INVALID_PARAM, "unknown GKR flags 0x%x", flags);
    if (!tree || !a || !d_weight || !d_state || !d_rounds || !d_points || !d_claims)
        return fail(BLZ_ERR_INVALID_PARAM, "a one-call GKR prover takes %s",
                    !tree ? "the product tree: tree is NULL" : !a ? "the leaves: a is NULL" : !d_weight ? "room for the weight: d_weight is NULL"
                    : !d_state ? "a transcript: d_state is NULL" : !d_rounds ? "room for the rounds: d_rounds is NULL"
                    : !d_points ? "room for the points: d_points is NULL" : "room for the claims: d_claims is NULL");
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    NttVecArg vt{}, va{};
    BLZ_TRY(call.resolve({{"tree", tree, &vt}, {"a", a, &va}}));
    if (vt.mask + 1 < len - 1)
        return fail(BLZ_ERR_INVALID_PARAM, "operand tree: %llu words, a tree over len %llu holds len - 1", (unsigned long long)(vt.mask + 1), (unsigned long long)len);
    if (va.mask + 1 < len)
        return fail(BLZ_ERR_INVALID_PARAM, "operand a: %llu words, read periodically over len %llu: the leaves are folded in place, so they are not periodic",
                    (unsigned long long)(va.mask + 1), (unsigned long long)len);
    uint32_t m = 0;   // log2 len
    while ((len >> m) > 1) ++m;
    // what the op names, in the order of the checks: the two operands, the weight, the four outputs
    struct Range { const char* name; const void* p; uint64_t words; };
    const Range rg[7] = {{"tree", vt.p, len - 1}, {"a", va.p, len}, {"d_weight", d_weight, std::max<uint64_t>(len / 4, 1)}, {"d_state", d_state, 1},
                         {"d_rounds", d_rounds, (uint64_t)3 * m * (m - 1) / 2}, {"d_points", d_points, (uint64_t)m * (m + 1) / 2}, {"d_claims", d_claims, (uint64_t)2 * m}};
    for (int o = 2; o < 7; ++o) BLZ_TRY(call.device_range(rg[o].name, "the pointer", rg[o].p, rg[o].words * 32, 16, rg[o].words, "elements"));
    for (int o = 1; o < 7; ++o)
        for (int i = 0; i < o; ++i)
            if (rg[i].words && rg[o].words && NttVecCall::words_meet(rg[i].p, rg[i].words, rg[o].p, rg[o].words))
                return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps %s: %llu words against %llu", rg[o].name, rg[i].name, (unsigned long long)rg[o].words,
                            (unsigned long long)rg[i].words);
    int wbuf[2] = {-1, -1};   // the tree's layers and the leaves are folded in place: a buffer either names is written
    if (!tree->d_ptr) wbuf[0] = (int)tree->buf;
    if (!a->d_ptr) wbuf[wbuf[0] < 0 ? 0 : 1] = (int)a->buf;
    const bool fused = !(flags & BLZ_GKR_UNFUSED);
    const uint32_t keep = ntt_fs_keep_bits(h->field);
    uint32_t* const weight = (uint32_t*)d_weight;
    uint32_t* const points = (uint32_t*)d_points;
    NttGate g;
    {
        blz_sum_gate product{};   // + lo hi
        product.ntables = 2, product.nterms = 1, product.common = -1;
        product.term[0].nfactors = 2, product.term[0].factor[1] = 1;
        BLZ_TRY(ntt_gkr_describe(&product, g));
    }
    NttGkrTail tail{vt.p, va.p, weight, (uint32_t*)d_state, (uint32_t*)d_rounds, points, (uint32_t*)d_claims, m, 0, 0, 0, 0, keep};
    return call.enqueue(wbuf[0], [&](uint32_t*) {
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t live = 1ull << j;   // words of lo and of hi
            if (fused && live <= GKR_TAIL_LEN) {   // every whole layer that fits, in one launch
                tail.first = j;
                while (j + 1 < m && (2ull << j) <= GKR_TAIL_LEN) ++j;
                tail.last = j + 1, tail.tail = 0, tail.claims_only = 0;
                BLZ_TRY(h->ops->gkr_tail(h->stream, tail));
                continue;
            }
            const uint32_t* const lo = j + 1 == m ? va.p : vt.p + (len - 4 * live) * 8;
            uint32_t* const rows = (uint32_t*)d_rounds + (size_t)3 * ((size_t)j * (j - 1) / 2) * 8;
            uint32_t* const row = points + ((size_t)j * (j + 1) / 2) * 8;   // row j of the points; row j - 1 ends where it starts
            tail.first = j, tail.last = j + 1;
            if (j >= 1) {
                g.t[0] = NttVecArg{lo, live - 1};
                g.t[1] = NttVecArg{lo + live * 8, live - 1};
                const NttVecArg vw{weight, std::max<uint64_t>(live / 2, 1) - 1};
                BLZ_TRY(h->ops->vec_mle_eq(h->stream, weight, row - (size_t)j * 8, j - 1, call.ws));
                BLZ_TRY(h->ops->zerocheck_gate(h->stream, g, vw, nullptr, 3, live, rows, call.ws));
                // the pairs (transcript step, step with r): all but the last variable's, or down to the live length the block takes
                const uint32_t chain = fused ? j - GKR_TAIL_LOG : j;
                for (uint32_t i = 0; i < chain; ++i) {
                    uint32_t* const r = row + (size_t)(j - 1 - i) * 8;   // backwards: the row ends up in bit order
                    BLZ_TRY(ntt_fs_absorb(h->stream, d_state, rows + (size_t)i * 3 * 8, 3, r, keep));
                    if (i + 1 < j) BLZ_TRY(h->ops->zerocheck_gate(h->stream, g, vw, r, 3, live >> i, rows + (size_t)(i + 1) * 3 * 8, call.ws));
                    else BLZ_TRY(h->ops->sumcheck_gate(h->stream, g, r, 0, 2, nullptr, call.ws));
                }
                if (fused) {
                    tail.tail = 1, tail.claims_only = 0;
                    BLZ_TRY(h->ops->gkr_tail(h->stream, tail));
                    continue;
                }
            }
            tail.tail = 0, tail.claims_only = 1;
            BLZ_TRY(h->ops->gkr_tail(h->stream, tail));
            BLZ_TRY(ntt_fs_absorb(h->stream, d_state, (uint32_t*)d_claims + (size_t)2 * j * 8, 2, row + (size_t)j * 8, keep));
        }
        return (int)BLZ_OK;
    }, wbuf[1]);
}

// The GKR argument over blz_ntt_mle_tree's FRACTION trees in one enqueue (include/blaze_hip.h, THE ONE-CALL FRACTION GKR PROVER;
// kernels: ntt_fgkr.hip.hpp).  blz_ntt_gkr_prove's walk over four tables a layer: P_lo, P_hi, Q_lo, Q_hi, the halves of layer
// m - 1 - j of the two trees (of the leaves for j = m - 1).  Below the root a layer starts with its batching challenge lambda_j
// (a transcript step that absorbs nothing) and T = P_hi + lambda_j Q_hi written over P_hi by gate_eval: T is folded like a table,
// so the layer gate P_lo Q_hi + Q_lo T needs no scalar and is zerocheck_gate's as it stands.  Behind the sumcheck the four final
// words - P_hi's recovered from T's - go to d_claims and through one transcript step.  BLZ_GKR_UNFUSED takes the existing
// launchers alone (and the claims kernel, one wave); without it the rounds at live lengths of 256 and below - all of them for
// m <= 9 - run inside one block, h->ops->fgkr_tail.  Every check stands before the first launch.
// (the gates are packed by blz_ntt_sumcheck_gate's own function, reached as blz_ntt_sumcheck_prove reaches it)
static constexpr auto ntt_fgkr_describe = &ntt_gate_describe;
int blz_ntt_gkr_prove_frac(blz_ntt* h, uint32_t flags, const blz_vec_arg* tree_p, const blz_vec_arg* tree_q, const blz_vec_arg* a_p,
                           const blz_vec_arg* a_q, uint64_t len, void* d_weight, void* d_state, void* d_rounds, void* d_points, void* d_claims,
                           void* d_lambdas) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (flags & ~BLZ_GKR_UNFUSED) return fail(BLZ_ERR_INVALID_PARAM, "unknown GKR flags 0x%x", flags);
    if (!tree_p || !tree_q || !a_p || !a_q || !d_weight || !d_state || !d_rounds || !d_points || !d_claims || !d_lambdas)
        return fail(BLZ_ERR_INVALID_PARAM, "a one-call fraction GKR prover takes %s",
                    !tree_p ? "the numerator tree: tree_p is NULL" : !tree_q ? "the denominator tree: tree_q is NULL" : !a_p ? "the numerators: a_p is NULL"
                    : !a_q ? "the denominators: a_q is NULL" : !d_weight ? "room for the weight: d_weight is NULL" : !d_state ? "a transcript: d_state is NULL"
                    : !d_rounds ? "room for the rounds: d_rounds is NULL" : !d_points ? "room for the points: d_points is NULL"
                    : !d_claims ? "room for the claims: d_claims is NULL" : "room for the layer challenges: d_lambdas is NULL");
    NttVecCall call{h};
    BLZ_TRY(call.live_length(len));
    BLZ_TRY(call.begin());
    static const char* const oname[4] = {"tree_p", "tree_q", "a_p", "a_q"};
    const blz_vec_arg* const ov[4] = {tree_p, tree_q, a_p, a_q};
    NttVecArg v[4] = {};
    BLZ_TRY(call.resolve({{oname[0], ov[0], &v[0]}, {oname[1], ov[1], &v[1]}, {oname[2], ov[2], &v[2]}, {oname[3], ov[3], &v[3]}}));
    for (int o = 0; o < 2; ++o)
        if (v[o].mask + 1 < len - 1)
            return fail(BLZ_ERR_INVALID_PARAM, "operand %s: %llu words, a tree over len %llu holds len - 1", oname[o], (unsigned long long)(v[o].mask + 1),
                        (unsigned long long)len);
    for (int o = 2; o < 4; ++o)
        if (v[o].mask + 1 < len)
            return fail(BLZ_ERR_INVALID_PARAM, "operand %s: %llu words, read periodically over len %llu: the leaves are folded in place, so they are not periodic",
                        oname[o], (unsigned long long)(v[o].mask + 1), (unsigned long long)len);
    uint32_t m = 0;   // log2 len
    while ((len >> m) > 1) ++m;
    // what the op names, in the order of the checks: the four operands, the weight, the five outputs
    struct Range { const char* name; const void* p; uint64_t words; };
    const Range rg[10] = {{oname[0], v[0].p, len - 1}, {oname[1], v[1].p, len - 1}, {oname[2], v[2].p, len}, {oname[3], v[3].p, len},
                          {"d_weight", d_weight, std::max<uint64_t>(len / 4, 1)}, {"d_state", d_state, 1}, {"d_rounds", d_rounds, (uint64_t)3 * m * (m - 1) / 2},
                          {"d_points", d_points, (uint64_t)m * (m + 1) / 2}, {"d_claims", d_claims, (uint64_t)4 * m}, {"d_lambdas", d_lambdas, m}};
    for (int o = 4; o < 10; ++o) BLZ_TRY(call.device_range(rg[o].name, "the pointer", rg[o].p, rg[o].words * 32, 16, rg[o].words, "elements"));
    for (int o = 1; o < 10; ++o)
        for (int i = 0; i < o; ++i)
            if (rg[i].words && rg[o].words && NttVecCall::words_meet(rg[i].p, rg[i].words, rg[o].p, rg[o].words))
                return fail(BLZ_ERR_INVALID_PARAM, "%s overlaps %s: %llu words against %llu", rg[o].name, rg[i].name, (unsigned long long)rg[o].words,
                            (unsigned long long)rg[i].words);
    int wbuf[2] = {-1, -1};   // the layers and the leaves are folded in place: a buffer any of the four names is written
    for (int o = 0; o < 4; ++o)
        if (!ov[o]->d_ptr && wbuf[0] != (int)ov[o]->buf && wbuf[1] != (int)ov[o]->buf) wbuf[wbuf[0] < 0 ? 0 : 1] = (int)ov[o]->buf;
    const bool fused = !(flags & BLZ_GKR_UNFUSED);
    const uint32_t keep = ntt_fs_keep_bits(h->field);
    uint32_t* const weight = (uint32_t*)d_weight;
    uint32_t* const points = (uint32_t*)d_points;
    uint32_t* const lambdas = (uint32_t*)d_lambdas;
    NttGate g, gt;
    {
        blz_sum_gate layer{};   // + P_lo Q_hi + Q_lo T over [P_lo, T, Q_lo, Q_hi]
        layer.ntables = 4, layer.nterms = 2, layer.common = -1;
        layer.term[0].nfactors = 2, layer.term[0].factor[0] = 0, layer.term[0].factor[1] = 3;
        layer.term[1].nfactors = 2, layer.term[1].factor[0] = 2, layer.term[1].factor[1] = 1;
        BLZ_TRY(ntt_fgkr_describe(&layer, g));
        blz_sum_gate lin{};   // T = + P_hi + lambda Q_hi over [P_hi, lambda, Q_hi]
        lin.ntables = 3, lin.nterms = 2, lin.common = -1;
        lin.term[0].nfactors = 1, lin.term[0].factor[0] = 0;
        lin.term[1].nfactors = 2, lin.term[1].factor[0] = 1, lin.term[1].factor[1] = 2;
        BLZ_TRY(ntt_fgkr_describe(&lin, gt));
    }
    NttFgkrTail tail{v[0].p, v[1].p, v[2].p, v[3].p, weight, (uint32_t*)d_state, (uint32_t*)d_rounds, points, (uint32_t*)d_claims, lambdas, m, 0, 0, 0, 0, keep};
    return call.enqueue(wbuf[0], [&](uint32_t*) {
        const uint64_t no_rot[BLZ_GATE_MAX_TABLES] = {};
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t live = 1ull << j;   // words of each of the four tables
            if (fused && live <= FGKR_TAIL_LEN) {   // every whole layer that fits, in one launch
                tail.first = j;
                while (j + 1 < m && (2ull << j) <= FGKR_TAIL_LEN) ++j;
                tail.last = j + 1, tail.tail = 0, tail.claims_only = 0;
                BLZ_TRY(h->ops->fgkr_tail(h->stream, tail));
                continue;
            }
            const uint32_t* const plo = j + 1 == m ? v[2].p : v[0].p + (len - 4 * live) * 8;
            const uint32_t* const qlo = j + 1 == m ? v[3].p : v[1].p + (len - 4 * live) * 8;
            uint32_t* const rows = (uint32_t*)d_rounds + (size_t)3 * ((size_t)j * (j - 1) / 2) * 8;
            uint32_t* const row = points + ((size_t)j * (j + 1) / 2) * 8;   // row j of the points; row j - 1 ends where it starts
            tail.first = j, tail.last = j + 1;
            if (j >= 1) {
                uint32_t* const lambda = lambdas + (size_t)j * 8;
                uint32_t* const phi = const_cast<uint32_t*>(plo) + live * 8;
                BLZ_TRY(ntt_fs_absorb(h->stream, d_state, nullptr, 0, lambda, keep));
                gt.t[0] = NttVecArg{phi, live - 1};
                gt.t[1] = NttVecArg{lambda, 0};
                gt.t[2] = NttVecArg{qlo + live * 8, live - 1};
                BLZ_TRY(h->ops->gate_eval(h->stream, phi, gt, no_rot, live));
                g.t[0] = NttVecArg{plo, live - 1};
                g.t[1] = NttVecArg{phi, live - 1};
                g.t[2] = NttVecArg{qlo, live - 1};
                g.t[3] = NttVecArg{qlo + live * 8, live - 1};
                const NttVecArg vw{weight, std::max<uint64_t>(live / 2, 1) - 1};
                BLZ_TRY(h->ops->vec_mle_eq(h->stream, weight, row - (size_t)j * 8, j - 1, call.ws));
                BLZ_TRY(h->ops->zerocheck_gate(h->stream, g, vw, nullptr, 3, live, rows, call.ws));
                // the pairs (transcript step, step with r): all but the last variable's, or down to the live length the block takes
                const uint32_t chain = fused ? j - FGKR_TAIL_LOG : j;
                for (uint32_t i = 0; i < chain; ++i) {
                    uint32_t* const r = row + (size_t)(j - 1 - i) * 8;   // backwards: the row ends up in bit order
                    BLZ_TRY(ntt_fs_absorb(h->stream, d_state, rows + (size_t)i * 3 * 8, 3, r, keep));
                    if (i + 1 < j) BLZ_TRY(h->ops->zerocheck_gate(h->stream, g, vw, r, 3, live >> i, rows + (size_t)(i + 1) * 3 * 8, call.ws));
                    else BLZ_TRY(h->ops->sumcheck_gate(h->stream, g, r, 0, 2, nullptr, call.ws));
                }
                if (fused) {
                    tail.tail = 1, tail.claims_only = 0;
                    BLZ_TRY(h->ops->fgkr_tail(h->stream, tail));
                    continue;
                }
            }
            tail.tail = 0, tail.claims_only = 1;
            BLZ_TRY(h->ops->fgkr_tail(h->stream, tail));
            BLZ_TRY(ntt_fs_absorb(h->stream, d_state, (uint32_t*)d_claims + (size_t)4 * j * 8, 4, row + (size_t)j * 8, keep));
        }
        return (int)BLZ_OK;
    }, wbuf[1]);
}

int blz_ntt_last_kernel_ms(blz_ntt* h, float* out) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    *out = h->last_ms;
    return BLZ_OK;
}

static int banks_geometry(blz_ntt* h, uint64_t& n, uint64_t& G, uint64_t& Bg) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (h->logn < 10) return fail(BLZ_ERR_INVALID_PARAM, "bank layout needs log_size >= 10 (512-element blocks in pairs)");
    n = 1ull << h->logn;
    G = n >= (1ull << 18) ? n >> 18 : 1;   // the reference shape: 2^27 -> 512 groups of 256 block pairs
    Bg = (n >> 10) / G;
    return BLZ_OK;
}
int blz_ntt_banks_preprocess_device(blz_ntt* h, const void* d_in, void* d_banks) {
    uint64_t n, G, Bg;
    BLZ_TRY(banks_geometry(h, n, G, Bg));
    if (!d_in || !d_banks) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_TRY(use_device(h->device));
    hipLaunchKernelGGL(k_ntt_banks_pre, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->copy_stream, (const uint4*)d_in,
                       (uint4*)d_banks, n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_TRY(sync_stream_bounded(h->copy_stream, "banks preprocess"));
    return BLZ_OK;
}
int blz_ntt_banks_postprocess_device(blz_ntt* h, const void* d_banks, void* d_out) {
    uint64_t n, G, Bg;
    BLZ_TRY(banks_geometry(h, n, G, Bg));
    if (!d_out || !d_banks) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_TRY(use_device(h->device));
    hipLaunchKernelGGL(k_ntt_banks_post, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->copy_stream, (const uint4*)d_banks,
                       (uint4*)d_out, n, G, Bg);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    BLZ_TRY(sync_stream_bounded(h->copy_stream, "banks postprocess"));
    return BLZ_OK;
}

}  // extern "C"
