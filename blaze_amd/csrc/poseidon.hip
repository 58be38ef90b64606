// Poseidon octal Merkle-tree client for gfx950: the device behind src/ingo_hash/poseidon_api.rs (the reference's third
// DriverPrimitive).  include/blaze_hip.h "Poseidon" states the hash, the tree, the record and the instruction stream;
// DESIGN.md section 8 the kernel.  This file is the host side: the stream's parser and checks, the element FIFO, the layer
// schedule (one launch per layer for a tree that arrives in one call), the record queue, and the preparation of the optimised
// partial rounds (derived and self-checked on the device: this file has no field arithmetic, it only compares words with r).
#include <algorithm>
#include <deque>
#include <fstream>
#include <string>
#include <vector>

#include "poseidon_engine.hpp"

namespace blz {

const PoseidonFieldOps* poseidon_ops_for(int field) {
    switch (field) {
        case BLZ_BLS377: return &poseidon_ops_bls377();
        case BLZ_BLS381: return &poseidon_ops_bls381();
        case BLZ_BN254: return &poseidon_ops_bn254();
    }
    return nullptr;
}

namespace {

constexpr size_t WORD = 32;
// "BLZPOSEIDON01", ASCII, as a little-endian integer: a CSV made for the card's microcode is refused instead of misread
const uint8_t POS_MAGIC[WORD] = {'B', 'L', 'Z', 'P', 'O', 'S', 'E', 'I', 'D', 'O', 'N', '0', '1'};

bool word_below(const uint8_t* w, const uint32_t (&m)[8]) {   // little-endian w < m
    for (int i = 7; i >= 0; --i) {
        const uint32_t x = (uint32_t)w[4 * i] | ((uint32_t)w[4 * i + 1] << 8) | ((uint32_t)w[4 * i + 2] << 16) | ((uint32_t)w[4 * i + 3] << 24);
        if (x != m[i]) return x < m[i];
    }
    return false;
}
// the word as a small integer; false when it does not fit 32 bits
bool word_small(const uint8_t* w, uint32_t& v) {
    for (size_t i = 4; i < WORD; ++i)
        if (w[i]) return false;
    v = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
    return true;
}

int load_fail(const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fail(BLZ_ERR_LOAD_FAILED, "Poseidon instruction stream: %s", buf);
}

// decimal text -> 32-byte little-endian word; false: not a decimal number, or >= 2^256
bool parse_decimal(const std::string& s, uint8_t out[WORD]) {
    uint32_t v[8] = {};
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '"')) ++a;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '"')) --b;
    if (a == b) return false;
    for (size_t i = a; i < b; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        uint64_t carry = (uint64_t)(s[i] - '0');
        for (int k = 0; k < 8; ++k) {
            const uint64_t t = (uint64_t)v[k] * 10u + carry;
            v[k] = (uint32_t)t;
            carry = t >> 32;
        }
        if (carry) return false;
    }
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 4; ++j) out[4 * k + j] = (uint8_t)(v[k] >> (8 * j));
    return true;
}

// load_instructions (poseidon_api.rs:205-243): a CSV whose first line is a header; every record sends its LAST column, then its
// SECOND-TO-LAST, as 32-byte little-endian words
int read_instruction_csv(const char* path, std::vector<uint8_t>& words) {
    if (!path || !*path) return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"\" }: no instruction path");
    std::ifstream f(path);
    if (!f) return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"%s\" }: cannot open the file", path);
    std::string line;
    if (!std::getline(f, line)) return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"%s\" }: empty file", path);
    size_t lineno = 1;
    while (std::getline(f, line)) {
        ++lineno;
        if (line.empty() || line == "\r") continue;
        const size_t c1 = line.rfind(',');
        if (c1 == std::string::npos || c1 == 0) return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"%s\" }: line %zu has fewer than two columns", path, lineno);
        const size_t c0 = line.rfind(',', c1 - 1);
        const std::string last = line.substr(c1 + 1), prev = line.substr(c0 == std::string::npos ? 0 : c0 + 1, c1 - (c0 == std::string::npos ? 0 : c0 + 1));
        uint8_t w[WORD];
        for (const std::string* s : {&last, &prev}) {
            if (!parse_decimal(*s, w)) return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"%s\" }: line %zu: not a decimal number below 2^256", path, lineno);
            words.insert(words.end(), w, w + WORD);
        }
    }
    return BLZ_OK;
}

}  // namespace

int poseidon_parse(int field, uint32_t need_mask, const uint8_t* words, size_t len, PoseidonStream& out) {
    const PoseidonFieldOps* ops = poseidon_ops_for(field);
    if (!ops) return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
    if (!words) return fail(BLZ_ERR_INVALID_PARAM, "null word stream");
    if (len % WORD) return load_fail("%zu bytes is not a whole number of 32-byte words", len);
    const size_t n = len / WORD;
    for (size_t i = 0; i < n; ++i)
        if (!word_below(words + i * WORD, ops->modulus)) return load_fail("word %zu is not below the field's modulus", i);
    if (n < 3) return load_fail("truncated header (%zu words)", n);
    if (memcmp(words, POS_MAGIC, WORD) != 0) return load_fail("wrong magic word: not a parameter stream of this library");
    uint32_t v = 0;
    if (!word_small(words + WORD, v) || (int)v != field) return load_fail("made for another field (word 1 does not name field %d)", field);
    uint32_t K = 0;
    if (!word_small(words + 2 * WORD, K) || K < 1 || K > (uint32_t)(POS_T_MAX - POS_T_MIN + 1)) return load_fail("block count out of range");
    out = PoseidonStream{};
    size_t pos = 3;
    for (uint32_t k = 0; k < K; ++k) {
        if (n - pos < 5) return load_fail("block %u is truncated (header)", k);
        uint32_t t = 0, alpha = 0, rf = 0, rp = 0;
        if (!word_small(words + pos * WORD, t) || t < (uint32_t)POS_T_MIN || t > (uint32_t)POS_T_MAX) return load_fail("block %u: width out of range [%d, %d]", k, POS_T_MIN, POS_T_MAX);
        if (!word_small(words + (pos + 1) * WORD, alpha) || alpha != 5) return load_fail("block %u: alpha must be 5", k);
        if (!word_small(words + (pos + 2) * WORD, rf) || rf < 2 || (rf & 1u) || rf > (uint32_t)POS_ROUNDS_MAX) return load_fail("block %u: R_F must be even and in [2, %d]", k, POS_ROUNDS_MAX);
        if (!word_small(words + (pos + 3) * WORD, rp) || rp > (uint32_t)POS_ROUNDS_MAX || rf + rp > (uint32_t)POS_ROUNDS_MAX) return load_fail("block %u: R_F + R_P must be at most %d", k, POS_ROUNDS_MAX);
        if (out.width_mask & (1u << t)) return load_fail("block %u: width %u appears twice", k, t);
        PoseidonBlock b;
        b.t = (int)t; b.rf = (int)rf; b.rp = (int)rp;
        b.tag = pos + 4;
        b.rc = pos + 5;
        b.mds = b.rc + (size_t)t * (rf + rp);
        const size_t end = b.mds + (size_t)t * t;
        if (end > n) return load_fail("block %u (t = %u) is truncated: %zu words needed, %zu present", k, t, end, n);
        out.blocks.push_back(b);
        out.width_mask |= 1u << t;
        pos = end;
    }
    out.consumed = pos;
    // an odd word count is padded with one zero word (a CSV record carries two words)
    if (n != pos && !(n == pos + 1 && (pos & 1u))) return load_fail("%zu words follow the last block", n - pos);
    if (n == pos + 1) {
        uint32_t pad = 1;
        if (!word_small(words + pos * WORD, pad) || pad != 0) return load_fail("the pad word behind the last block is not zero");
    }
    if ((out.width_mask & need_mask) != need_mask)
        return load_fail("a width the tree mode needs is missing (needed: mask 0x%x, present: mask 0x%x)", need_mask, out.width_mask);
    return BLZ_OK;
}

// upload the whole stream (waited for: `words` is free on return, whatever happens next), convert it on `st`, point w[] into
// `consts`; the caller waits for the conversion
int poseidon_upload(const PoseidonFieldOps* ops, hipStream_t st, const PoseidonStream& ps, const uint8_t* words, DevBuf& raw, DevBuf& consts,
                           PoseidonWidth (&w)[POS_T_MAX + 1]) {
    const size_t n = ps.consumed;
    BLZ_TRY(raw.reserve(n * WORD, true));
    BLZ_TRY(consts.reserve(n * POS_SD * 4, true));
    BLZ_HIP(hipMemcpyAsync(raw.p, words, n * WORD, hipMemcpyHostToDevice, st), BLZ_ERR_WRITE);
    BLZ_TRY(sync_stream_bounded(st, "Poseidon constants: upload"));
    BLZ_TRY(ops->prep(st, raw.as<uint32_t>(), consts.as<uint32_t>(), (uint32_t)n));
    for (auto& x : w) x = PoseidonWidth{};
    for (const auto& b : ps.blocks) {
        PoseidonWidth& x = w[b.t];
        x.t = b.t; x.rf = b.rf; x.rp = b.rp;
        x.tag = consts.as<uint32_t>() + b.tag * POS_SD;
        x.rc = consts.as<uint32_t>() + b.rc * POS_SD;
        x.mds = consts.as<uint32_t>() + b.mds * POS_SD;
    }
    return BLZ_OK;
}

}  // namespace blz

using namespace blz;

struct blz_poseidon {
    int device = 0;
    int field = BLZ_BLS381;
    const PoseidonFieldOps* ops = nullptr;
    hipStream_t stream = nullptr;        // the layer kernels
    hipStream_t copy_stream = nullptr;   // elements into the FIFO, records out
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_in = nullptr;
    // initialize()
    bool initialized = false;
    uint32_t height = 0;
    int mode = BLZ_TREE_C;
    uint32_t width_mask = 0;
    PoseidonWidth w[POS_T_MAX + 1];
    std::vector<PoseidonBlock> blocks;   // where each width's words are inside `raw`
    DevBuf raw, consts, input, layers, records;
    // the optimised partial rounds: the switch (kept across initialize), their tables and the state of their self-check (per
    // loaded instruction set: 0 not prepared yet, HADES_OK, HADES_REFUSED - then every width runs the dense rounds)
    int plan_setting = 1;
    uint32_t plan_state = 0;
    DevBuf plan;
    HadesPlan pl[POS_T_MAX + 1];
    uint64_t n_in = 0;                    // elements of one tree's FIFO
    int first_layer = 0;                  // lowest layer that is hashed (0 TreeC, 1 TreeD)
    std::vector<uint64_t> lay_n, lay_off, rec_off;   // nodes of layer l; its first digest / record (in nodes; layers below first_layer: unused)
    uint64_t tree_records = 0;
    // the FIFO and the schedule
    uint64_t received = 0;                // elements of the current tree
    std::vector<uint64_t> done;           // nodes of layer l hashed (enqueued) so far
    bool tree_finished = false;           // the current tree's last element has arrived and every layer is enqueued
    bool in_busy = false;                 // ev_in is recorded: a kernel that reads the FIFO buffer may still run
    uint64_t total_elements = 0;
    // records: ranges of the record buffer in the order they were enqueued, and the records of earlier trees moved to the host
    struct Range { uint64_t first, n; };
    std::deque<Range> pending;
    uint64_t pending_n = 0, popped_of_tree = 0;
    std::vector<uint8_t> stash;
    size_t stash_pos = 0;
    uint32_t last_hash_id = 0, last_layer = 0;
    bool timing_open = false, timing_valid = false;
    float last_ms = 0.f;
    bool wedged = false;
};

#define BLZ_POS_LIVE(h)                                                                                          \
    do {                                                                                                         \
        if ((h)->wedged)                                                                                         \
            return fail(BLZ_ERR_UNKNOWN, "handle is wedged: an earlier wait timed out (BLAZE_WAIT_TIMEOUT_MS); only " \
                                         "reset / free are accepted");                                           \
    } while (0)
#define BLZ_POS_WAIT(h, expr)                      \
    do {                                           \
        blz::wait_clear();                         \
        int rc__ = (expr);                         \
        if (rc__ != BLZ_OK) {                      \
            if (blz::wait_timed_out()) (h)->wedged = true; \
            return rc__;                           \
        }                                          \
    } while (0)

namespace {

constexpr uint64_t POS_BATCH = 1024;   // hashes worth a launch of their own while a tree is still arriving

void pos_drop_stream_state(blz_poseidon* h) {
    h->received = 0;
    std::fill(h->done.begin(), h->done.end(), 0);
    h->tree_finished = false;
    h->pending.clear();
    h->pending_n = 0;
    h->popped_of_tree = 0;
    h->stash.clear();
    h->stash_pos = 0;
    h->timing_open = false;
}

bool pos_plan_in_force(const blz_poseidon* h) { return h->plan_setting == 1 && h->plan_state == HADES_OK; }

// The self-check's inputs for one width: n hashes of t - 1 words.  Fixed: the words 0, r - 1, r, r + 1, 2^256 - 1 in every
// position of a hash of their own, then words of a xorshift generator (any 256-bit words: about half of them are >= r).
void pos_check_batch(const uint32_t (&modulus)[8], int t, size_t n, std::vector<uint32_t>& out) {
    const size_t a = (size_t)t - 1;
    out.assign(n * a * 8, 0u);
    uint64_t sx = 0x9E3779B97F4A7C15ull ^ ((uint64_t)t << 32);
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < a; ++k) {
            uint32_t* wd = out.data() + (i * a + k) * 8;
            if (i == 0) continue;                                              // 0
            if (i <= 3) {                                                      // r - 1, r, r + 1  (r is odd and its low word is not 0)
                for (int q = 0; q < 8; ++q) wd[q] = modulus[q];
                wd[0] += (uint32_t)i - 2u;
            } else if (i == 4) {
                for (int q = 0; q < 8; ++q) wd[q] = 0xffffffffu;
            } else {
                for (int q = 0; q < 8; ++q) {
                    sx ^= sx << 13; sx ^= sx >> 7; sx ^= sx << 17;
                    wd[q] = (uint32_t)(sx >> 16);
                }
            }
        }
}

constexpr size_t POS_CHECK_HASHES = 320;   // per derived width: 64 waves' worth at t = 12, a ragged last block at every width

// Derive the tables of the widths the tree mode hashes with, then hash a fixed batch per width with both kernels and compare.
// Leaves plan_state at HADES_OK or HADES_REFUSED; a refusal is not an error.  Blocking, every wait bounded.
int pos_prepare_plan(blz_poseidon* h) {
    if (h->plan_state != 0) return BLZ_OK;
    const uint32_t need = poseidon_need_mask(h->mode);
    size_t elements = 0, nw = 0;
    for (const auto& b : h->blocks)
        if (need & (1u << b.t)) { elements += hades_plan_elements(b.t, b.rp); ++nw; }
    const size_t status_at = elements * POS_SD * 4;
    BLZ_TRY(h->plan.reserve(status_at + POS_T_MAX * 4 + 16, true));
    uint32_t* const tables = h->plan.as<uint32_t>();
    uint32_t* const d_status = tables + elements * POS_SD;
    BLZ_HIP(hipMemsetAsync(d_status, 0, nw * 4, h->stream), BLZ_ERR_UNKNOWN);
    size_t at = 0, k = 0;
    for (const auto& b : h->blocks) {
        if (!(need & (1u << b.t))) continue;
        uint32_t* const tb = tables + at * POS_SD;
        BLZ_TRY(h->ops->derive(h->stream, h->raw.as<uint32_t>() + b.tag * 8, b.t, b.rf, b.rp, tb, d_status + k));
        h->pl[b.t] = hades_plan_at(tb, b.t, b.rp);
        at += hades_plan_elements(b.t, b.rp);
        ++k;
    }
    uint32_t status[POS_T_MAX] = {};
    BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "round plan: derivation"));
    BLZ_HIP(hipMemcpy(status, d_status, nw * 4, hipMemcpyDeviceToHost), BLZ_ERR_READ);
    uint32_t state = HADES_OK;
    for (size_t i = 0; i < nw; ++i)
        if (status[i] != HADES_OK) state = HADES_REFUSED;
    // the self-check: both kernels on the same inputs, digests compared word for word
    DevBuf in, dig;
    std::vector<uint32_t> words, got(2 * POS_CHECK_HASHES * 8);
    int rc = BLZ_OK;
    for (const auto& b : h->blocks) {
        if (state != HADES_OK || rc != BLZ_OK) break;
        if (!(need & (1u << b.t))) continue;
        pos_check_batch(h->ops->modulus, b.t, POS_CHECK_HASHES, words);
        if ((rc = in.reserve(words.size() * 4, true)) != BLZ_OK) break;
        if ((rc = dig.reserve(got.size() * 4, true)) != BLZ_OK) break;
        if (hipMemcpyAsync(in.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) { rc = fail(BLZ_ERR_WRITE, "round plan: self-check inputs"); break; }
        PoseidonJob job;
        job.in = in.as<uint32_t>();
        job.dig = dig.as<uint32_t>();
        job.n = POS_CHECK_HASHES;
        if ((rc = h->ops->hash(h->stream, h->w[b.t], job)) != BLZ_OK) break;
        job.dig += POS_CHECK_HASHES * 8;
        if ((rc = h->ops->hash_plan(h->stream, h->w[b.t], h->pl[b.t], job)) != BLZ_OK) break;
        blz::wait_clear();
        if ((rc = sync_stream_bounded(h->stream, "round plan: self-check")) != BLZ_OK) {
            if (blz::wait_timed_out()) h->wedged = true;   // (the buffers stay: the kernels may still write them)
            return rc;
        }
        if (hipMemcpy(got.data(), dig.p, got.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(BLZ_ERR_READ, "round plan: self-check digests"); break; }
        if (memcmp(got.data(), got.data() + POS_CHECK_HASHES * 8, POS_CHECK_HASHES * 32) != 0) state = HADES_REFUSED;
    }
    in.release();
    dig.release();
    BLZ_TRY(rc);
    h->plan_state = state;
    BLZ_LOG(1, "Poseidon round plan: %s", state == HADES_OK ? "optimised partial rounds, self-check equal" : "refused (singular matrix or self-check): dense rounds");
    return BLZ_OK;
}

// hash what can be hashed: every layer's nodes whose inputs exist, lowest layer first.  force: whatever the batch size.
int pos_advance(blz_poseidon* h, bool force) {
    const bool last = h->received == h->n_in;
    for (int l = h->first_layer; l < (int)h->height; ++l) {
        const uint64_t below = l == 0 ? h->received / 11u : (l == 1 && h->first_layer == 1 ? h->received : h->done[l - 1]) / 8u;
        const uint64_t todo = below - h->done[l];
        if (!todo) continue;
        if (!force && !last && todo < POS_BATCH) break;
        PoseidonJob job;
        const uint64_t d0 = h->done[l];
        if (l == 0) job.in = h->input.as<uint32_t>() + d0 * 11u * 8u;
        else if (l == 1 && h->first_layer == 1) job.in = h->input.as<uint32_t>() + d0 * 8u * 8u;
        else job.in = h->layers.as<uint32_t>() + (h->lay_off[l - 1] + d0 * 8u) * 8u;
        job.dig = h->layers.as<uint32_t>() + (h->lay_off[l] + d0) * 8u;
        job.rec = h->records.as<uint32_t>() + (h->rec_off[l] + d0) * 16u;
        job.n = todo;
        job.id0 = d0;
        job.layer = (uint32_t)l;
        if (!h->timing_open) {
            // the round plan is prepared before a tree's first launch, outside the timed window (a switch set in mid-tree
            // finds it at the next tree)
            if (h->plan_setting == 1) BLZ_TRY(pos_prepare_plan(h));
            BLZ_HIP(hipEventRecord(h->ev0, h->stream), BLZ_ERR_UNKNOWN);
            h->timing_open = true;
            h->timing_valid = false;
        }
        const int t = l == 0 ? 12 : 9;
        if (pos_plan_in_force(h)) BLZ_TRY(h->ops->hash_plan(h->stream, h->w[t], h->pl[t], job));
        else BLZ_TRY(h->ops->hash(h->stream, h->w[t], job));
        if (l == h->first_layer) {   // the launches that read the FIFO buffer
            BLZ_HIP(hipEventRecord(h->ev_in, h->stream), BLZ_ERR_UNKNOWN);
            h->in_busy = true;
        }
        h->pending.push_back({h->rec_off[l] + d0, todo});
        h->pending_n += todo;
        h->done[l] = below;
    }
    if (last && !h->tree_finished) {
        h->tree_finished = true;
        if (h->timing_open) {
            BLZ_HIP(hipEventRecord(h->ev1, h->stream), BLZ_ERR_UNKNOWN);
            h->timing_open = false;
            h->timing_valid = true;
        }
    }
    return BLZ_OK;
}

// the next element opens a new tree: records of the finished one that nobody has read yet move to the host, the buffers are reused
int pos_open_next_tree(blz_poseidon* h) {
    uint64_t on_device = 0;
    for (const auto& r : h->pending) on_device += r.n;
    if (on_device) {
        BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "set_data: records of the finished tree"));
        size_t at = h->stash.size();
        if (h->stash_pos == at) { h->stash.clear(); h->stash_pos = 0; at = 0; }
        h->stash.resize(at + on_device * 64u);
        for (const auto& r : h->pending) {
            BLZ_HIP(hipMemcpy(h->stash.data() + at, h->records.as<uint8_t>() + r.first * 64u, r.n * 64u, hipMemcpyDeviceToHost), BLZ_ERR_READ);
            at += r.n * 64u;
        }
        h->pending.clear();
        // (pending_n keeps counting them: they are pending, on the host side of the queue now)
    }
    h->received = 0;
    std::fill(h->done.begin(), h->done.end(), 0);
    h->tree_finished = false;
    h->popped_of_tree = 0;
    return BLZ_OK;
}

uint64_t pos_stashed(const blz_poseidon* h) { return (h->stash.size() - h->stash_pos) / 64u; }

int pos_set_data_common(blz_poseidon* h, const void* data, size_t len, bool on_device) {
    if (!h || !data) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_POS_LIVE(h);
    if (!h->initialized) return fail(BLZ_ERR_INVALID_PARAM, "set_data before initialize");
    uint8_t one[WORD] = {};
    uint64_t k;
    if (len % WORD == 0) k = len / WORD;
    else if (len < WORD && !on_device) {   // the reference's tests write 4-byte and to_bytes_le() buffers: one element, zero-extended
        memcpy(one, data, len);
        data = one;
        k = 1;
    } else return fail(BLZ_ERR_INVALID_PARAM, "set_data of %zu bytes: a multiple of 32, or one element of fewer than 32 bytes (host memory)", len);
    BLZ_TRY(use_device(h->device));
    const uint8_t* src = (const uint8_t*)data;
    while (k) {
        if (h->tree_finished) BLZ_TRY(pos_open_next_tree(h));
        if (h->received == 0 && h->in_busy) {   // the tree before may still be reading the buffer
            BLZ_HIP(hipStreamWaitEvent(h->copy_stream, h->ev_in, 0), BLZ_ERR_UNKNOWN);
            h->in_busy = false;
        }
        const uint64_t take = std::min<uint64_t>(k, h->n_in - h->received);
        BLZ_HIP(hipMemcpyAsync(h->input.as<uint8_t>() + h->received * WORD, src, take * WORD, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               h->copy_stream), BLZ_ERR_WRITE);
        // blocking, like the other set_datas: the caller's buffer is free on return, and the kernels enqueued below find the elements
        BLZ_POS_WAIT(h, sync_stream_bounded(h->copy_stream, "set_data: elements into the Poseidon FIFO"));
        h->received += take;
        h->total_elements += take;
        src += take * WORD;
        k -= take;
        BLZ_TRY(pos_advance(h, false));
    }
    return BLZ_OK;
}

int pos_pop(blz_poseidon* h, uint64_t n, uint8_t* out) {
    if (!n) return BLZ_OK;
    uint8_t* o = out;
    uint64_t left = n;
    const uint64_t from_stash = std::min<uint64_t>(left, pos_stashed(h));
    if (from_stash) {
        memcpy(o, h->stash.data() + h->stash_pos, from_stash * 64u);
        h->stash_pos += from_stash * 64u;
        o += from_stash * 64u;
        left -= from_stash;
    }
    if (left) {
        BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "results: the layer kernels"));
        uint64_t want = left;
        for (auto it = h->pending.begin(); it != h->pending.end() && want; ++it) {
            const uint64_t m = std::min<uint64_t>(want, it->n);
            BLZ_HIP(hipMemcpyAsync(o, h->records.as<uint8_t>() + it->first * 64u, m * 64u, hipMemcpyDeviceToHost, h->copy_stream), BLZ_ERR_READ);
            o += m * 64u;
            want -= m;
        }
        BLZ_POS_WAIT(h, sync_stream_bounded(h->copy_stream, "results: records to the host"));
        while (left) {
            auto& r = h->pending.front();
            const uint64_t m = std::min<uint64_t>(left, r.n);
            r.first += m;
            r.n -= m;
            left -= m;
            h->popped_of_tree += m;
            if (!r.n) h->pending.pop_front();
        }
    }
    h->pending_n -= n;
    const uint8_t* lastrec = out + (n - 1) * 64u + 32u;
    const uint64_t tagw = (uint64_t)lastrec[0] | ((uint64_t)lastrec[1] << 8) | ((uint64_t)lastrec[2] << 16) | ((uint64_t)lastrec[3] << 24) | ((uint64_t)lastrec[4] << 32);
    h->last_hash_id = (uint32_t)(tagw & 0x3fffffffu);
    h->last_layer = (uint32_t)(tagw >> 30) & 0x3ffu;
    return BLZ_OK;
}

int pos_initialize_core(blz_poseidon* h, uint32_t tree_height, int tree_mode, const uint8_t* words, size_t len) {
    PoseidonStream ps;
    BLZ_TRY(poseidon_parse(h->field, poseidon_need_mask(tree_mode), words, len, ps));
    BLZ_TRY(use_device(h->device));
    // sizes of the tree
    const int first_layer = tree_mode == BLZ_TREE_C ? 0 : 1;
    std::vector<uint64_t> lay_n(tree_height), lay_off(tree_height, 0), rec_off(tree_height, 0);
    uint64_t nodes = 0;
    for (uint32_t l = 0; l < tree_height; ++l) {
        lay_n[l] = 1ull << (3 * (tree_height - 1 - l));
        if ((int)l >= first_layer) {
            lay_off[l] = rec_off[l] = nodes;
            nodes += lay_n[l];
        }
    }
    const uint64_t n_in = (tree_mode == BLZ_TREE_C ? 11ull : 1ull) * lay_n[0];
    const uint64_t bytes_in = n_in * WORD, bytes_lay = nodes * WORD, bytes_rec = nodes * 64u;
    size_t free_b = 0, total_b = 0;
    BLZ_HIP(hipMemGetInfo(&free_b, &total_b), BLZ_ERR_UNKNOWN);
    const uint64_t held = h->input.cap + h->layers.cap + h->records.cap;   // (released below, before the new ones are taken)
    if (bytes_in + bytes_lay + bytes_rec + (64ull << 20) > (uint64_t)free_b + held)
        return fail(BLZ_ERR_INVALID_PARAM, "a tree of height %u needs %llu bytes of device memory, %llu are free", tree_height,
                    (unsigned long long)(bytes_in + bytes_lay + bytes_rec), (unsigned long long)((uint64_t)free_b + held));
    // DriverClient::reset first (poseidon_api.rs:97): nothing of an earlier tree survives.  From here on a failure (an allocation,
    // a transfer) leaves the handle UNINITIALISED - the old tree is gone - which the header says
    BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "initialize: Poseidon stream"));
    BLZ_POS_WAIT(h, sync_stream_bounded(h->copy_stream, "initialize: Poseidon copy stream"));
    h->initialized = false;
    h->input.release(); h->layers.release(); h->records.release(); h->raw.release(); h->consts.release(); h->plan.release();
    h->plan_state = 0;
    for (auto& x : h->pl) x = HadesPlan{};
    BLZ_TRY(poseidon_upload(h->ops, h->stream, ps, words, h->raw, h->consts, h->w));
    BLZ_TRY(h->input.reserve(bytes_in, true));
    BLZ_TRY(h->layers.reserve(bytes_lay ? bytes_lay : WORD, true));
    BLZ_TRY(h->records.reserve(bytes_rec ? bytes_rec : 64u, true));
    BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "initialize: Poseidon constants"));
    h->height = tree_height;
    h->mode = tree_mode;
    h->width_mask = ps.width_mask;
    h->blocks = ps.blocks;
    h->n_in = n_in;
    h->first_layer = first_layer;
    h->lay_n = lay_n; h->lay_off = lay_off; h->rec_off = rec_off;
    h->tree_records = nodes;
    h->done.assign(tree_height, 0);
    pos_drop_stream_state(h);
    h->in_busy = false;
    h->total_elements = 0;
    h->last_hash_id = h->last_layer = 0;
    h->timing_valid = false;
    h->initialized = true;
    BLZ_LOG(1, "Poseidon: height %u, %s, widths 0x%x, round plan %d (prepared before the first tree), %llu bytes", tree_height,
            tree_mode == BLZ_TREE_C ? "TreeC" : "TreeD", ps.width_mask, h->plan_setting, (unsigned long long)(bytes_in + bytes_lay + bytes_rec));
    return BLZ_OK;
}

int pos_check_init_args(blz_poseidon* h, uint32_t tree_height, int tree_mode) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_POS_LIVE(h);
    if (tree_mode != BLZ_TREE_C && tree_mode != BLZ_TREE_D) return fail(BLZ_ERR_INVALID_PARAM, "unknown tree mode %d", tree_mode);
    // layer_id has 10 bits and hash_id 30: 8^(h - 1) <= 2^30
    if (tree_height < 1 || tree_height > 11) return fail(BLZ_ERR_INVALID_PARAM, "tree height %u out of range [1, 11]", tree_height);
    return BLZ_OK;
}

}  // namespace

extern "C" {

int blz_poseidon_new(int device_id, int field, blz_poseidon** out) {
    if (!out) return fail(BLZ_ERR_INVALID_PARAM, "null out");
    *out = nullptr;
    const PoseidonFieldOps* ops = poseidon_ops_for(field);
    if (!ops) return fail(BLZ_ERR_INVALID_PARAM, "unknown field %d", field);
    BLZ_TRY(use_device(device_id));
    blz_poseidon* h = new blz_poseidon();
    h->device = device_id;
    h->field = field;
    h->ops = ops;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming);
    if (e != hipSuccess) {
        const int rc = fail_hip(BLZ_ERR_UNKNOWN, "stream/event creation failed: %s", hipGetErrorString(e));
        blz_poseidon_free(h);
        return rc;
    }
    *out = h;
    return BLZ_OK;
}

void blz_poseidon_free(blz_poseidon* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if ((h->stream && sync_stream_bounded(h->stream, "free: Poseidon stream") != BLZ_OK) ||
        (h->copy_stream && sync_stream_bounded(h->copy_stream, "free: Poseidon copy stream") != BLZ_OK)) {
        BLZ_LOG(0, "Poseidon handle freed while its device work is wedged: buffers and streams are leaked");
        delete h;
        return;
    }
    h->input.release(); h->layers.release(); h->records.release(); h->raw.release(); h->consts.release(); h->plan.release();
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    delete h;
}

int blz_poseidon_loaded_binary_parameters(blz_poseidon* h, uint32_t out[2]) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    // [0] image id 'MI35' (as the MSM handle); [1] decodes with PoseidonImageParametrs::parse_image_params (poseidon_api.rs:256-271:
    // to_be_bytes, packed_struct msb0 ranges, no bit reversal): is_stub (msb0 bits 28-31) 0, number_of_cores (20-27) = compute units
    // saturated at the field's 255, place holder 0
    out[0] = 0x4D493335u;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 0;
    const uint32_t cores = cus > 255 ? 255u : (uint32_t)cus;
    out[1] = cores << 4;
    return BLZ_OK;
}

int blz_poseidon_check_words(int field, int tree_mode, const uint8_t* words, size_t len, uint32_t out[4]) {
    if (tree_mode != BLZ_TREE_C && tree_mode != BLZ_TREE_D) return fail(BLZ_ERR_INVALID_PARAM, "unknown tree mode %d", tree_mode);
    PoseidonStream ps;
    BLZ_TRY(poseidon_parse(field, poseidon_need_mask(tree_mode), words, len, ps));
    if (out) {
        out[0] = (uint32_t)ps.blocks.size();
        out[1] = ps.width_mask;
        out[2] = 0;   // admission needs field arithmetic (is Mh invertible?): blz_poseidon_prepare_round_plan / blz_poseidon_info answer
        out[3] = (uint32_t)ps.consumed;
    }
    return BLZ_OK;
}

int blz_poseidon_initialize_words(blz_poseidon* h, uint32_t tree_height, int tree_mode, const uint8_t* words, size_t len) {
    BLZ_TRY(pos_check_init_args(h, tree_height, tree_mode));
    if (!words) return fail(BLZ_ERR_INVALID_PARAM, "null word stream");
    return pos_initialize_core(h, tree_height, tree_mode, words, len);
}

int blz_poseidon_initialize(blz_poseidon* h, uint32_t tree_height, int tree_mode, const char* instruction_path) {
    BLZ_TRY(pos_check_init_args(h, tree_height, tree_mode));
    std::vector<uint8_t> words;
    BLZ_TRY(read_instruction_csv(instruction_path, words));
    const int rc = pos_initialize_core(h, tree_height, tree_mode, words.data(), words.size());
    if (rc == BLZ_ERR_LOAD_FAILED) {   // LoadFailed { path } (poseidon_api.rs:100-103)
        const std::string why = blz_last_error_message();
        return fail(BLZ_ERR_LOAD_FAILED, "LoadFailed { path: \"%s\" }: %s", instruction_path, why.c_str());
    }
    return rc;
}

int blz_poseidon_set_data(blz_poseidon* h, const uint8_t* data, size_t len) { return pos_set_data_common(h, data, len, false); }
int blz_poseidon_set_data_device(blz_poseidon* h, const void* d_data, size_t len) { return pos_set_data_common(h, d_data, len, true); }

int blz_poseidon_wait_result(blz_poseidon* h) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_POS_LIVE(h);
    if (!h->initialized) return fail(BLZ_ERR_INVALID_PARAM, "wait_result before initialize");
    BLZ_TRY(use_device(h->device));
    BLZ_TRY(pos_advance(h, true));
    BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "wait_result: Poseidon"));
    return BLZ_OK;
}

int blz_poseidon_num_pending_results(blz_poseidon* h, uint32_t* out) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_POS_LIVE(h);
    *out = (uint32_t)h->pending_n;
    return BLZ_OK;
}

int blz_poseidon_raw_results(blz_poseidon* h, uint32_t n, uint8_t* out, size_t cap) {
    if (!h || (!out && n)) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_POS_LIVE(h);
    if (n > h->pending_n) return fail(BLZ_ERR_INVALID_PARAM, "%u records asked for, %llu pending", n, (unsigned long long)h->pending_n);
    if (cap < (size_t)n * 64u) return fail(BLZ_ERR_INVALID_PARAM, "output buffer too small for %u records", n);
    BLZ_TRY(use_device(h->device));
    return pos_pop(h, n, out);
}

int blz_poseidon_result(blz_poseidon* h, uint32_t expected, uint8_t* out, size_t cap, uint32_t* n) {
    if (!h || !n || (!out && expected)) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    *n = 0;
    BLZ_POS_LIVE(h);
    if (!h->initialized) return fail(BLZ_ERR_INVALID_PARAM, "result before initialize");
    BLZ_TRY(use_device(h->device));
    // the reference polls the pending count until `expected` records have come (poseidon_api.rs:128-145), for ever if they never do;
    // here every node whose inputs have arrived is hashed now, and what exists then is what there is
    BLZ_TRY(pos_advance(h, true));
    const uint64_t m = std::min<uint64_t>(expected, h->pending_n);
    if (cap < m * 64u) return fail(BLZ_ERR_INVALID_PARAM, "output buffer too small for %llu records", (unsigned long long)m);
    BLZ_TRY(pos_pop(h, m, out));
    *n = (uint32_t)m;
    return BLZ_OK;
}

int blz_poseidon_tree_device(blz_poseidon* h, void* d_out, size_t cap) {
    if (!h || !d_out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_POS_LIVE(h);
    if (!h->initialized || !h->tree_finished || pos_stashed(h) || h->popped_of_tree || h->pending_n != h->tree_records)
        return fail(BLZ_ERR_INVALID_PARAM, "tree_device needs a finished tree none of whose records has been read, and no older records pending");
    if (cap < h->tree_records * 64u) return fail(BLZ_ERR_INVALID_PARAM, "output buffer too small for %llu records", (unsigned long long)h->tree_records);
    BLZ_TRY(use_device(h->device));
    if (h->tree_records) {
        BLZ_HIP(hipMemcpyAsync(d_out, h->records.p, h->tree_records * 64u, hipMemcpyDeviceToDevice, h->stream), BLZ_ERR_READ);
        BLZ_POS_WAIT(h, sync_stream_bounded(h->stream, "tree_device: records"));
        h->last_hash_id = 0;
        h->last_layer = h->height - 1;
    }
    h->popped_of_tree += h->pending_n;
    h->pending.clear();
    h->pending_n = 0;
    return BLZ_OK;
}

int blz_poseidon_counters(blz_poseidon* h, uint32_t out[4]) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    out[0] = (uint32_t)h->total_elements;
    out[1] = h->last_hash_id;
    out[2] = h->last_layer;
    uint64_t waiting = 0;
    if (h->initialized && !h->tree_finished) waiting = h->received - (h->first_layer == 0 ? h->done[0] * 11u : (h->height > 1 ? h->done[1] * 8u : h->received));
    out[3] = (uint32_t)waiting;
    return BLZ_OK;
}

int blz_poseidon_info(blz_poseidon* h, uint64_t out[4]) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    out[0] = (uint64_t)(h->input.cap + h->layers.cap + h->records.cap + h->raw.cap + h->consts.cap + h->plan.cap);
    out[1] = pos_plan_in_force(h) ? 1u : 0u;
    out[2] = h->plan_state;
    out[3] = h->initialized ? h->width_mask : 0u;
    return BLZ_OK;
}

int blz_poseidon_set_round_plan(blz_poseidon* h, int enable) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    if (enable != 0 && enable != 1) return fail(BLZ_ERR_INVALID_PARAM, "round plan %d (0 dense, 1 optimised partial rounds where their self-check holds)", enable);
    // takes effect at the next layer launch (the bytes are the same either way); tables derived earlier are kept and reused
    h->plan_setting = enable;
    return BLZ_OK;
}

int blz_poseidon_prepare_round_plan(blz_poseidon* h, uint32_t out[2]) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_POS_LIVE(h);
    if (!h->initialized) return fail(BLZ_ERR_INVALID_PARAM, "prepare_round_plan before initialize");
    if (h->plan_setting == 1) {
        BLZ_TRY(use_device(h->device));
        BLZ_TRY(pos_prepare_plan(h));
    }
    if (out) {
        out[0] = pos_plan_in_force(h) ? 1u : 0u;
        out[1] = h->plan_state;
    }
    return BLZ_OK;
}

int blz_poseidon_last_kernel_ms(blz_poseidon* h, float* out) {
    if (!h || !out) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    BLZ_POS_LIVE(h);
    if (h->timing_valid) {
        BLZ_TRY(use_device(h->device));
        BLZ_POS_WAIT(h, sync_event_bounded(h->ev1, "last_kernel_ms: Poseidon"));
        (void)hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1);
    }
    *out = h->last_ms;
    return BLZ_OK;
}

int blz_poseidon_stream(blz_poseidon* h, void** hip_stream, int* device_id) {
    if (!h || !hip_stream) return fail(BLZ_ERR_INVALID_PARAM, "null argument");
    if (device_id) *device_id = h->device;
    *hip_stream = (void*)h->stream;
    return BLZ_OK;
}

int blz_poseidon_reset(blz_poseidon* h) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_TRY(use_device(h->device));
    BLZ_TRY(sync_stream_bounded(h->stream, "reset: Poseidon stream"));
    BLZ_TRY(sync_stream_bounded(h->copy_stream, "reset: Poseidon copy stream"));
    pos_drop_stream_state(h);
    h->in_busy = false;
    h->wedged = false;
    return BLZ_OK;
}

}  // extern "C"
