// set_data of the MSM primitive (src/ingo_msm/msm_api.rs:155-220): the bytes of the handle's task go to the device and the task to
// the engine - piece by piece while its data crosses the link, or whole once its data is complete.
//
// The reference's set_data walks its input in 2048-element chunks into FIFOs (msm_api.rs:155-202) and the card counts elements
// against the NUMBER_OF_MSM_ELEMENTS register that initialize() wrote (msm_hw_code.rs:18-19): whether a task's bytes come in one
// call or in many is invisible to it.  Here too: the task being fed is one record (blz_msm::Feed), and a set_data is a SLICE of it -
// in any of the three modes (1 scalars only over bases in the arena; 2 points + scalars; 3 points into the arena + scalars), any
// slice sizes (the reference's 2048-element cadence, ragged tails, one element).  A task in one call is a feed whose first slice
// carries all of it; data staged before start_process is a task of that call's size, launched by start_process.  One path:
//   check_slice    every check of the call, before anything is copied;
//   open_feed      the first slice: the task's size (fixed from then on), its staging set and buffers, and the piece-or-whole rule
//                  (open_pieces);
//   feed_slice     the slice's bytes - whole into the staging set, or part by part into the task's pieces, each piece handed to the
//                  engine as its data completes;
//   the last slice end() of a task in pieces, else the whole launch (launch_if_ready); task_enqueued / feed_abandon keep the books.
// The task is complete when received == n; more is refused, and so are initialize / start_process / a mode change while it is
// half-fed.  The reference's largest DMA-mode shape (tests/integration_msm.rs:386-467: 2^26 elements x 8 bases, a 48 GiB host
// vector) thus runs from host slices of any size.
#include "msm_handle.hpp"

namespace blz {

// the task is with the engine (slot): its staging set is free again behind set_free, its result goes to wait_result
static int task_enqueued(blz_msm* h, int slot) {
    if (h->feed.set >= 0) h->set_used[h->feed.set] = true;
    h->in_flight.push_back({slot, h->task_label});
    h->feed = blz_msm::Feed();
    return BLZ_OK;
}

void feed_abandon(blz_msm* h) {
    blz_msm::Feed& F = h->feed;
    if (F.slot >= 0) h->eng.abandon(F.slot);
    if (F.set >= 0) h->set_used[F.set] = true;   // (copies may have landed in it: the next user waits for set_free, recorded or long past)
    const bool armed = F.armed;
    F = blz_msm::Feed();
    F.armed = armed;
}

int launch_if_ready(blz_msm* h) {
    const blz_msm::Feed& F = h->feed;
    if (!(F.armed && F.ready)) return BLZ_OK;
    if (!h->eng.can_accept())
        return fail(BLZ_ERR_INVALID_PARAM, "task queue full (%d in flight); call wait_result first", MSM_QUEUE_DEPTH);
    uint32_t npts = F.n * h->pf;
    int sbits = h->pf == 1 ? 256 : 32;
    int slot = 0;
    int table_c = 0;
    const void* pts = h->points_mont.p;
    memset(h->table_info, 0, sizeof(h->table_info));
    memset(h->pc_info, 0, sizeof(h->pc_info));
    // (a task that has just loaded its own table - mode 3, msm_api.rs:203-216 - is a DMA-mode task as far as the plan is
    // concerned: a check per task would cost more than it saves)
    // A task that gathers from an auto-built window table pins it for the launch: an allocation of the launch that fails releases
    // the device's auto-built tables (arena.hip arena_release_auto_tables) - but not the rows this very task is about to read.  If
    // that was the memory the launch lacked, the table goes here, behind the failed launch, and the task is launched once more on
    // the plain path.
    for (int attempt = 0;; ++attempt) {
        if (F.mode != 2) BLZ_TRY(resolve_arena_task(h, F.arena_pos, F.n, true, F.mode == 1, &npts, &sbits, &table_c, &pts));
        h->eng.inputs_event = F.set >= 0 ? h->set_free[F.set] : nullptr;
        table_pin(table_c ? pts : nullptr);
        const int rc = h->eng.run(pts, F.d_scalars, npts, sbits, &slot, table_c, h->range_lo, h->range_hi);
        const bool skipped = table_pin_skipped();
        table_pin(nullptr);
        if (rc == BLZ_OK) break;
        if (!(attempt == 0 && skipped && !wait_timed_out() && release_auto_tables_on_oom() > 0)) return rc;
    }
    return task_enqueued(h, slot);
}

// How many pieces a task whose data arrives over the link is enqueued in (MsmEngine::begin): pieces of >= 2^19 points with
// their scalars (64 MiB of host bytes: 1.2 ms of link), at most 16.
// Measured (profiles/r04_dma_pieces.txt): 2^22 elements 22.6 ms in one piece, 16.2 / 15.35 / 17.1 in 4 / 8 / 16; 2^26
// 270.8, 191.8 / 178.3 / 171.5
static int pick_pieces(const blz_msm* h, uint32_t npts, bool with_points) {
    int pieces = env_int("BLAZE_MSM_PIECES", 0);   // (the same switch forces the piece count of device-resident tasks, msm.hip run())
    if (pieces <= 0) {
        if (with_points) {
            pieces = (int)(npts >> 19);
            if (npts >= (1u << 20) && npts <= (1u << 21)) pieces = (int)(npts >> 18);   // 2^20: 5.49 ms in 2 pieces, 5.23 in 4; 2^21: 8.47 in 4, 8.25 in 8
            if (pieces > 16) pieces = 16;
            // with another task in flight the link is the bound whatever the pieces do, and every piece costs it the
            // ~150 us of launches between two copies: fewer, larger pieces (2^22: 10.4 against 10.8 ms per MSM)
            if (busy(h) && pieces > 4) pieces = 4;
        } else {
            // scalars alone: the link is a quarter of the task, and every piece pays the sort stage's passes over the
            // bucket space again (not hidden here) - 2^26: 163.7 ms whole, 158.5 / 145.4 / 181.8 in 16 / 8 / 32 pieces
            // (2^22 .. 2^24 lone tasks: 14.25 / 25.6 / 46.2 ms whole, 13.3 / 23.6 / 42.5 in two pieces, 12.7 / 22.5 / 40.6 in four)
            pieces = (int)(npts >> 23);
            if (pieces > 8) pieces = 8;
            if (pieces < 4) pieces = 4;
        }
    }
    return pieces < 1 ? 1 : pieces;
}

// the ring's slots hold pieces of piece_pts points.  Transactional: a failed reserve leaves an empty ring (DevBuf::reserve has
// freed the old buffer), never a slot size over a buffer that is gone
static int ring_reserve(blz_msm* h, uint32_t piece_pts) {
    blz_msm::PieceRing& R = h->ring;
    if (piece_pts <= R.slot_pts) return BLZ_OK;
    // (a growing ring is reallocated behind a bounded drain of the device - DevBuf::reserve - so no piece in flight reads the old one)
    R.slot_pts = 0;
    for (bool& r : R.recorded) r = false;
    const size_t ps = point_size(h), mp = mont_point_bytes(h->curve);
    BLZ_TRY(R.raw.reserve((size_t)piece_pts * blz_msm::PieceRing::SLOTS * ps + 16, true));
    BLZ_TRY(R.mont.reserve((size_t)piece_pts * blz_msm::PieceRing::SLOTS * mp + 16, true));
    R.slot_pts = piece_pts;
    return BLZ_OK;
}

// piece `k` of the ring (a running number): where its raw points and their Montgomery copy go; the copy stream is ordered behind
// the to-Montgomery pass that last read the slot
static int ring_slot(blz_msm* h, uint64_t k, char** raw, char** mont) {
    blz_msm::PieceRing& R = h->ring;
    const int slot = (int)(k % blz_msm::PieceRing::SLOTS);
    *raw = (char*)R.raw.p + (size_t)slot * R.slot_pts * point_size(h);
    *mont = (char*)R.mont.p + (size_t)slot * R.slot_pts * mont_point_bytes(h->curve);
    return slot;
}
static int ring_wait_free(blz_msm* h, uint64_t k) {
    blz_msm::PieceRing& R = h->ring;
    const int slot = (int)(k % blz_msm::PieceRing::SLOTS);
    if (R.recorded[slot]) BLZ_HIP(hipStreamWaitEvent(h->copy_stream, R.raw_read[slot], 0), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}
// the piece's raw points -> Montgomery copy on the main stream; the slot's raw bytes are free behind it
static int ring_to_mont(blz_msm* h, uint64_t k, uint32_t np) {
    blz_msm::PieceRing& R = h->ring;
    char *raw = nullptr, *mont = nullptr;
    const int slot = ring_slot(h, k, &raw, &mont);
    BLZ_TRY(h->eng.points_to_mont(raw, mont, np));
    BLZ_HIP(hipEventRecord(R.raw_read[slot], h->eng.stream), BLZ_ERR_UNKNOWN);
    R.recorded[slot] = true;
    return BLZ_OK;
}

// Every check of a set_data call, before anything is copied.  *n_task: the elements of the task the slice belongs to - the open
// feed's, else the armed task's (initialize's nof_elements), else, before start_process, the call's own.
static int check_slice(blz_msm* h, int mode, bool on_device, const void* points, size_t points_len, const void* scalars, size_t scalars_len,
                       uint32_t m, uint64_t pos, uint32_t* n_task) {
    const blz_msm::Feed& F = h->feed;
    const size_t ps = point_size(h);
    const uint32_t n = F.open ? F.n : F.armed ? h->nof_elements : m;
    const uint32_t got = F.open ? F.received : 0;
    *n_task = n;
    if ((uint64_t)got + m > n)
        return fail(BLZ_ERR_INVALID_PARAM, "set_data carries %u elements, the queued task lacks only %u of its %u", m, n - got, n);
    if (!scalars && m) return fail(BLZ_ERR_INVALID_PARAM, "null scalars");
    if (scalars_len != (size_t)m * BLZ_SCALAR_SIZE)
        return fail(BLZ_ERR_INVALID_PARAM, "scalars length %zu != nof_elements %u * 32", scalars_len, m);
    if (points && points_len != (size_t)m * h->pf * ps)
        return fail(BLZ_ERR_INVALID_PARAM, "points length %zu != nof_elements %u * precompute_factor %u * %zu", points_len, m, h->pf, ps);
    if (F.open) {
        if (mode != F.mode || on_device != F.src_device)
            return fail(BLZ_ERR_INVALID_PARAM, "the queued task is being fed in another mode (points / hbm_point_addr / host or device pointers differ from its first slice)");
        if (mode == 1 && pos != F.arena_pos)
            return fail(BLZ_ERR_INVALID_PARAM, "hbm_point_addr differs from the first slice's (a streamed task names the address of its FIRST base in every slice)");
        // mode 3: the slices' tables back to back
        const uint64_t want = F.arena_pos + (uint64_t)F.received * h->pf * ps;
        if (mode == 3 && pos != want)
            return fail(BLZ_ERR_INVALID_PARAM, "slice of a streamed task: its points go to %llu, behind the %u elements already loaded at %llu (got %llu)",
                        (unsigned long long)want, F.received, (unsigned long long)F.arena_pos, (unsigned long long)pos);
        return BLZ_OK;
    }
    // ---- the first slice: the task as a whole
    if ((uint64_t)n * h->pf >= (1ull << 31)) return fail(BLZ_ERR_INVALID_PARAM, "too many points");
    // sizes the window planner cannot serve (u32 entry indexing: points x windows <= 2^32 - 2^26 (msm_engine.hpp MSM_MAX_ENTRIES) with
    // windows of at most 23 bits - 256-bit scalars need 12, so pf = 1 stops at 352 321 536 points (2^28.39; checked there:
    // tests/test_gpu_msm.py), the 32-bit chunks of pf = 8 at 2^31 - 2^25)
    if (n && h->eng.plan_for(n * h->pf, h->pf == 1 ? 256 : 32).c == 0)
        return fail(BLZ_ERR_INVALID_PARAM, "no window plan for %llu points of %d-bit scalars (u32 entry indexing: at most 352321536 points at pf = 1, 2113929216 at pf = 8)",
                    (unsigned long long)n * h->pf, h->pf == 1 ? 256 : 32);
    if (!h->eng.can_accept())
        return fail(BLZ_ERR_INVALID_PARAM, "task queue full (%d in flight); call wait_result first", MSM_QUEUE_DEPTH);
    if (on_device && m == n) {   // used in place (open_feed)
        if (((uintptr_t)scalars) % 16) return fail(BLZ_ERR_INVALID_PARAM, "device scalars must be 16-byte aligned");
        if (mode == 2 && ((uintptr_t)points) % 16) return fail(BLZ_ERR_INVALID_PARAM, "device points must be 16-byte aligned");
    }
    if (mode == 1) {
        // bases from the arena.  The reference's initialize() programs only hbm_point_addr.0 as the start address
        // (msm_api.rs:84-95) while load_data_to_hbm writes at addr+offset (msm_api.rs:312); both tests use offset 0.  Here the
        // task reads where the load wrote.
        Arena& A = arena_for(h->device);
        std::lock_guard<std::mutex> lk(A.mu);
        if (!arena_find(A, pos, (size_t)n * h->pf * ps))
            return fail(BLZ_ERR_INVALID_PARAM, "HBM bases: no loaded extent covers [%llu, +%zu) on device %d", (unsigned long long)pos,
                        (size_t)n * h->pf * ps, h->device);
    }
    return BLZ_OK;
}

// The piece-or-whole rule of the task being opened.  In pieces, the task goes to the engine while its data crosses the link, the
// way the reference streams interleaved chunks of scalars and points into the card's FIFOs while the card computes
// (msm_api.rs:175-202): per piece its scalars, then its sort stage; its points, then their to-Montgomery pass and the piece's
// accumulation (MsmEngine::begin / sort_slice / accumulate_slice / end: the pieces share one bucket space and the bucket sums are
// carried from piece to piece).  Link and multiplier work at the same time; what is left behind the last byte is the last piece's
// accumulation, the bucket reduce and the tail.  Taken by an armed task whose data lands in the staging set:
//  - points + scalars (mode 2, DMA mode, the reference's primary flow: tests/integration_msm.rs:149-207) always - in one call even
//    as a single piece (its points pass through the piece ring, not through buffers of the task's size);
//  - scalars over bases in the arena (the reference's HBM flow, tests/integration_msm_hbm.rs:57-100: mode 1, and mode 3 in one call)
//    when the handle is idle and the task large: a lone task's 2 GiB of scalars would otherwise cross the link with the chip doing
//    nothing (38 of 163 ms at 2^26); in a stream of tasks the whole upload already hides under the previous task's accumulation,
//    and the task keeps its one-piece form (hidden sort, no carried sums);
//  - a task fed by several calls only when the engine makes more than one piece of it; its table loaded slice by slice (mode 3),
//    never.
// Everything else is launched whole once its data is complete: data staged before start_process, a task from device pointers in
// one call (used in place), empty tasks, the overlap switched off.
static int open_pieces(blz_msm* h, bool one_call) {
    blz_msm::Feed& F = h->feed;
    if (!F.armed || F.n == 0 || F.set < 0 || (F.mode == 3 && !one_call) || exp_knob("BLAZE_DMA_OVERLAP", 1) == 0) return BLZ_OK;
    uint32_t npts = F.n * h->pf;
    int sbits = h->pf == 1 ? 256 : 32;
    const void* mont = nullptr;
    if (F.mode != 2) {
        if (!(npts >= (1u << 22) || env_int("BLAZE_MSM_PIECES", 0) > 1) || busy(h) || wants_table_for(h, F.arena_pos, npts)) return BLZ_OK;
        // (stale spans are converted on the main stream; a precompute handle on the checked-table plan: 4n even bases, 64-bit chunks)
        int tc = 0;
        BLZ_TRY(resolve_arena_task(h, F.arena_pos, F.n, false, F.mode == 1, &npts, &sbits, &tc, &mont));
    }
    const int want = pick_pieces(h, npts, F.mode == 2);
    if (!one_call && want < 2) return BLZ_OK;
    int slot = -1;
    h->eng.inputs_event = h->set_free[F.set];
    BLZ_TRY(h->eng.begin(npts, sbits, &slot, 0, h->range_lo, h->range_hi, want, true));
    const int pieces = h->eng.slots[slot].slices;
    if (!one_call && pieces < 2) {   // (the engine made one piece of it: the whole launch serves that)
        h->eng.abandon(slot);
        return BLZ_OK;
    }
    F.slot = slot;
    F.per = h->eng.slots[slot].pts_per_slice;
    F.npts = npts;
    F.sbits = sbits;
    F.ppe = npts / F.n;
    F.even = h->pc_info[0] != 0;
    F.mont = mont;
    if (F.mode == 2) {
        // the task's pieces take consecutive numbers of the handle's piece ring
        BLZ_TRY(ring_reserve(h, F.per));
        F.ring_first = h->ring.next;
        h->ring.next += (uint64_t)pieces;
    }
    return BLZ_OK;
}

// the first slice of a task (n elements, m of them in this call): its record, its staging set and buffers, how it is enqueued
static int open_feed(blz_msm* h, int mode, bool on_device, const void* scalars, uint32_t n, uint32_t m, uint64_t pos) {
    feed_abandon(h);   // (data staged before start_process and never launched is replaced)
    blz_msm::Feed& F = h->feed;
    F.open = true;
    F.mode = mode;
    F.src_device = on_device;
    F.n = n;
    F.arena_pos = mode == 2 ? 0 : pos;
    if (mode == 2) task_repr_bn254pc(h, false, 0);   // (DMA-mode task of a precompute handle: its arithmetic off the plan)
    if (on_device && m == n) {
        F.d_scalars = scalars;   // the whole task from device pointers: used in place, nothing is copied
    } else {
        // host buffers are staged on their own stream, so the transfer of this task overlaps the accumulation of the task in flight
        // (the reference's DMA writes overlap device compute the same way).  The staging set was last used two tasks
        // ago: its to-Montgomery pass and digit sort must have read it before the new copies land (an event on the main stream, not
        // a host wait; normally long past)
        F.set = h->stage_idx;
        if (h->set_used[F.set]) BLZ_HIP(hipStreamWaitEvent(h->copy_stream, h->set_free[F.set], 0), BLZ_ERR_UNKNOWN);
        h->stage_idx ^= 1;
        BLZ_TRY(h->scalars_buf[F.set].reserve(n ? (size_t)n * BLZ_SCALAR_SIZE : 16));
        F.d_scalars = h->scalars_buf[F.set].p;
    }
    if (F.armed) {
        memset(h->table_info, 0, sizeof(h->table_info));
        memset(h->pc_info, 0, sizeof(h->pc_info));
    }
    BLZ_TRY(open_pieces(h, m == n));
    if (F.slot < 0 && mode == 2) {   // launched whole: buffers of the task's size
        const size_t npts = (size_t)n * h->pf;
        if (F.set >= 0) BLZ_TRY(h->points_raw[F.set].reserve(npts ? npts * point_size(h) : 16));
        BLZ_TRY(h->points_mont.reserve(npts ? npts * mont_point_bytes(h->curve) : 16));
    }
    if (m != n) {
        BLZ_LOG(2, "streamed task: %u elements, mode %d (%s), %s", n, mode, mode == 1 ? "scalars over arena bases" : mode == 2 ? "points + scalars" : "points into the arena + scalars",
                F.slot >= 0 ? "enqueued in pieces as the slices arrive" : "launched whole behind its last slice");
        if (F.slot >= 0) BLZ_LOG(2, "streamed task: %d pieces of %u points%s", h->eng.slots[F.slot].slices, F.per, mode == 2 ? " through the piece ring" : "");
    }
    return BLZ_OK;
}

// The slice's m elements.  The caller may drop its buffers as soon as we return (set_data is synchronous: utils.rs:71): what was
// enqueued has landed before we do (bounded waits), also when a step failed.
//  - whole: behind the earlier slices in the staging set (used in place: nothing to copy);
//  - in pieces: part by part, a part lying inside one piece; the part that completes piece k lands its scalars and enqueues the
//    piece's sort before its points cross the link (a one-call task sorts piece k while its points are on the link), then the
//    piece's to-Montgomery pass (its points in a slot of the ring) and accumulation.  Any other part lands once, scalars and points
//    together.  So sort_slice(k) always follows accumulate_slice(k - 1), which the ping-pong sort buffers rely on (msm.hip).
static int feed_slice(blz_msm* h, const char* points, const char* scalars, uint32_t m) {
    blz_msm::Feed& F = h->feed;
    const size_t ps = point_size(h), pe = (size_t)h->pf * ps;   // pe: bytes of one element's points
    const hipMemcpyKind kind = F.src_device ? hipMemcpyDefault : hipMemcpyHostToDevice;
    bool pending = false;   // copies enqueued that have not landed
    auto copy = [&](void* dst, const void* src, size_t len, const char* what) -> int {
        if (!len) return BLZ_OK;
        if (hipMemcpyAsync(dst, src, len, kind, h->copy_stream) != hipSuccess) return fail_hip(BLZ_ERR_WRITE, "set_data: copy of the %s failed", what);
        pending = true;
        return BLZ_OK;
    };
    auto land = [&]() -> int {
        pending = false;
        wait_clear();
        const int r = sync_stream_bounded(h->copy_stream, "set_data: host -> device copy of a task's data");
        if (r != BLZ_OK && wait_timed_out()) h->wedged = true;
        return r;
    };
    int rc = BLZ_OK;
    if (F.slot < 0) {
        if (F.set >= 0) {
            rc = copy((char*)h->scalars_buf[F.set].p + (size_t)F.received * BLZ_SCALAR_SIZE, scalars, (size_t)m * BLZ_SCALAR_SIZE, "scalars");
            if (rc == BLZ_OK && F.mode == 2) rc = copy((char*)h->points_raw[F.set].p + (size_t)F.received * pe, points, (size_t)m * pe, "points");
            if (rc == BLZ_OK && pending) rc = land();
        }
        if (rc == BLZ_OK) F.received += m;
    }
    const size_t sb = (size_t)F.sbits / 8, mp = mont_point_bytes(h->curve);
    for (uint32_t off = 0; F.slot >= 0 && off < m && rc == BLZ_OK;) {
        const uint32_t at = F.received * F.ppe, k = at / F.per, fill = at % F.per, p0 = k * F.per;
        const uint32_t np = F.npts - p0 < F.per ? F.npts - p0 : F.per;   // points of piece k
        uint32_t take = (np - fill) / F.ppe;                               // elements that still fit into it (per holds whole elements)
        if (take > m - off) take = m - off;
        const bool completes = fill + take * F.ppe == np;
        char* d_sc = (char*)h->scalars_buf[F.set].p + (size_t)p0 * sb;
        char *d_raw = nullptr, *d_mont = nullptr;
        rc = copy(d_sc + (size_t)fill * sb, scalars + (size_t)off * BLZ_SCALAR_SIZE, (size_t)take * BLZ_SCALAR_SIZE, "scalars");
        if (rc == BLZ_OK && completes) rc = land();
        if (rc == BLZ_OK && completes) rc = h->eng.sort_slice(F.slot, (int)k, d_sc, np);
        if (rc == BLZ_OK && F.mode == 2) {
            (void)ring_slot(h, F.ring_first + k, &d_raw, &d_mont);
            if (fill == 0) rc = ring_wait_free(h, F.ring_first + k);
            if (rc == BLZ_OK) rc = copy(d_raw + (size_t)fill * ps, points + (size_t)off * pe, (size_t)take * pe, "points");
            if (rc == BLZ_OK) rc = land();
        }
        if (rc != BLZ_OK) break;
        F.received += take;
        off += take;
        if (!completes) continue;
        if (F.mode == 2) {
            rc = ring_to_mont(h, F.ring_first + k, np);
        } else if (!F.mont) {
            // the extent's copy as it stands NOW: a load between two slices may have moved the extent or rewritten bases (their
            // points are converted here, ahead of the piece); a checked table that a write re-opened cannot be served mid-task
            rc = arena_points_mont(h, F.arena_pos, F.n * h->pf, &F.mont, F.even);
            if (rc == BLZ_OK && !F.mont)
                rc = fail(BLZ_ERR_INVALID_PARAM, "the precompute table was rewritten while a task over it was being streamed on the checked-table "
                                                 "plan: reset the handle and send the task again");
        }
        if (rc == BLZ_OK) rc = h->eng.accumulate_slice(F.slot, (int)k, F.mode == 2 ? (const char*)d_mont : (const char*)F.mont + (size_t)p0 * mp);
    }
    if (pending) {
        const int lrc = land();
        if (rc == BLZ_OK) rc = lrc;
    }
    return rc;
}

// the task is complete: end() of a task in pieces, else its points to Montgomery form (mode 2) and the whole launch
static int finish_feed(blz_msm* h, const void* points) {
    blz_msm::Feed& F = h->feed;
    if (F.slot >= 0) {
        BLZ_TRY(h->eng.end(F.slot));
        return task_enqueued(h, F.slot);
    }
    if (F.mode == 2) BLZ_TRY(h->eng.points_to_mont(F.set >= 0 ? h->points_raw[F.set].p : points, h->points_mont.p, F.n * h->pf));
    F.open = false;
    F.ready = true;
    return launch_if_ready(h);
}

int stage(blz_msm* h, const void* points, size_t points_len, const void* scalars, size_t scalars_len, uint32_t m, int has_hbm,
          uint64_t hbm_addr, uint64_t hbm_off, bool on_device) {
    if (!h) return fail(BLZ_ERR_INVALID_PARAM, "null handle");
    BLZ_LIVE(h);
    BLZ_TRY(use_device(h->device));
    if (!points && !has_hbm) return BLZ_OK;  // reference: falls through every branch (msm_api.rs:163-216)
    if (has_hbm) BLZ_ARENA_ADDR(hbm_addr, hbm_off);
    blz_msm::Feed& F = h->feed;
    const int mode = points ? (has_hbm ? 3 : 2) : 1;
    const uint64_t pos = hbm_addr + hbm_off;
    uint32_t n = 0;
    BLZ_TRY(check_slice(h, mode, on_device, points, points_len, scalars, scalars_len, m, pos, &n));
    int rc = BLZ_OK;
    if (mode == 3) {
        // msm_api.rs:203-206: load_data_to_hbm(points, addr, offset) first
        wait_clear();
        rc = arena_write(h->device, pos, points, points_len, on_device, h->eng.stream);
        if (rc != BLZ_OK && wait_timed_out()) h->wedged = true;
        if (rc == BLZ_OK) {
            h->bases_from_hbm = true;
            h->hbm_addr = hbm_addr;
        }
    }
    if (rc == BLZ_OK && !F.open) rc = open_feed(h, mode, on_device, scalars, n, m, pos);
    else F.mont = nullptr;   // (resolved again for this slice's pieces)
    if (rc == BLZ_OK) rc = feed_slice(h, (const char*)points, (const char*)scalars, m);
    if (rc == BLZ_OK && F.received == F.n) rc = finish_feed(h, points);
    // a failure loses the task being fed (bytes of it may be missing): the task stays armed and may be sent again from its first
    // element.  (A whole launch refused at the end - bases gone from the arena, say - is not sent again without new data either.)
    if (rc != BLZ_OK && F.open) feed_abandon(h);
    return rc;
}

}  // namespace blz
