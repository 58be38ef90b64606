// The sort stage of an MSM task - everything in front of k_accumulate: signed window digits of every scalar sorted by bucket,
// the bucket / unit scans, the unit lists - chosen once and enqueued by one call.
//
//   plan_sort()       which of the three digit sorts a task gets and where it runs (msm_engine.hpp SortPlan): host arithmetic,
//                     called by MsmEngine::begin(), printed in the BLAZE_LOG=2 plan line, pinned by tests/test_msm_sort_plan.py
//   msm_sort_stage()  a piece's stage on C.sort_stream: what MsmEngine::sort_slice() enqueues between its waits and its events
// The three sorts cover different parts of the stage:
//   msm_sort_tiny.hip  all of it, in one block (small one-piece tasks)
//   msm_sort3.hip      count[] and entries[] in one go; the scans and the unit lists follow (built to run underneath an accumulation)
//   msm_sort.hip       count[], then - behind the scans, which it needs - entries[]; the unit lists follow
// and the kernels they share live here:
//   k_scan_*       exclusive scan: bucket offsets + accumulate-unit offsets (runs split at L)
//   k_fill_units   unit -> bucket map;  k_unit_* order the units by run length (descending)
#include "msm_sort.hpp"

namespace blz {

// ------------------------------------------------------------------------------------------------
// the choice (msm_engine.hpp SortPlan)
// ------------------------------------------------------------------------------------------------
// When the handle's other task is still in flight - its accumulation is running or about to - the stage of a one-piece task
// goes to sort_stream with the small-footprint three-level sort (msm_sort3.hip) and runs UNDERNEATH that accumulation; the
// accumulation of this task then starts with its sort already done.  The pieces of a task on an otherwise idle handle do the
// same among themselves: piece k + 1 sorts underneath the accumulation of piece k (ping-pong over the two slots' sort buffers).
// in.hide_env is BLAZE_SORT_HIDE: 0 never, 1 when there is something to hide under (default), 2 the three-level sort always (on
// the main stream when there is nothing to hide under: tests).
// Two guards, which hold at 1 and - for the ping-pong - at every value but 0:
//  - recent_hot.  The three-level sort gives one block a whole level-2 bin: fine for the near-uniform digits of real scalars, a
//    cliff for inputs that pile entries into a few buckets (the reference harness repeats a 256-point tile).  The handle's last
//    two COLLECTED tasks say which kind it is being fed (finish(): their largest bucket against their own mean - judged when
//    the host has waited for the task, never read from a copy that may still be in flight).
//  - fits (msm_sort_fits_beside).  The sort only hides if its waves fit BESIDE the accumulation's: two of those per SIMD (registers
//    are allocated in eights) plus one of the sort's.  Measured: the sort runs beside 2 x 194..199 (-> 2 x 200) + 72 = 472
//    registers, and waits for the accumulation to END behind 2 x 206 (-> 208) + 72 = 488 and 2 x 211 (-> 216) + 72 = 504 -
//    the SIMD does not hand out all 512.  A build whose k_accumulate grew past that still works, it just sorts in
//    the open (round 3 saw 211 VGPRs cost 4 ms per step before this check existed).
//    (the SIMD runs as many accumulation waves as their allocation admits: two of the reduced-radix kernels', three of
//    the 32-bit-limb kernel's, whose allocation is padded to 136 for exactly this purpose)
//    A table plan's largest kernel (k3t_l3<true>: 78 VGPRs, allocated as 80) fits with nothing to spare: 2 x 200 + 80 = 480.
//    The same goes for LDS: the BLS accumulation's four blocks per CU hold 4 x 16 KiB, the sort's largest block 83 KiB.
SortPlan plan_sort(const MsmPlan& P, uint32_t npts, int sbits, int pieces, const SortInputs& in) {
    const bool on = in.hide_env != 0, guarded = in.hide_env == 1;
    if (P.table)   // a table task has no other sort: where it cannot hide it sorts in the open
        return {SortPlan::S3, on && in.other_busy && (!guarded || in.fits) ? SortPlan::HIDDEN : SortPlan::OPEN};
    const bool s3_ok = on && msm_sort3_ok(P, sbits);
    if (pieces > 1) return s3_ok && !in.other_busy && !in.recent_hot && in.fits ? SortPlan{SortPlan::S3, SortPlan::PINGPONG} : SortPlan{SortPlan::LDS, SortPlan::OPEN};
    const bool s3 = s3_ok && (!guarded || (!in.recent_hot && in.fits));
    if (s3 && in.other_busy) return {SortPlan::S3, SortPlan::HIDDEN};
    if (s3 && in.hide_env == 2) return {SortPlan::S3, SortPlan::OPEN};
    // with nothing to hide under, the two-level sort is the faster one - and a small task's whole stage is one block's work
    return {msm_sort_tiny_ok(P, npts, sbits) ? SortPlan::TINY : SortPlan::LDS, SortPlan::OPEN};
}

std::string describe(const SortPlan& s) {
    static const char* const kind[] = {"lds", "s3", "tiny"};
    static const char* const where[] = {"open", "hidden", "pingpong"};
    return std::string(kind[s.kind]) + " " + where[s.where];
}

// do the hidden sort's waves (sv VGPRs) fit on a SIMD beside the accumulation's (av VGPRs each, as many as fit)?  Measured: the
// sort runs beside 2 x 200 + 72 = 472 registers and waits for the accumulation to END behind 2 x 208 + 72 = 488.
// LDS (reasoned from the allocation rules, not measured like the register bound): the accumulation's blocks are 128 lanes, so `waves` of its waves per SIMD are 2 x waves blocks per CU; one block of the
// sort has to fit in what they leave of the CU's 160 KiB (allocations taken in steps of 1 KiB).  A sort block that does not
// fit is not an error either: it waits until the accumulation's blocks drain from a CU, that is for its end.
bool msm_sort_fits_beside(int av, int sv, int al, int sl) {
    if (av <= 0 || sv <= 0) return true;
    const int a = (av + 7) & ~7, s = (sv + 7) & ~7;
    int waves = 512 / a;
    if (waves > 4) waves = 4;
    if (waves < 1) waves = 1;
    if (waves * a + s > 512 - 32) return false;
    if (al <= 0 || sl <= 0) return true;   // no LDS on one side (or not known): nothing to share
    const int ak = (al + 1023) >> 10, sk = (sl + 1023) >> 10;
    return 2 * waves * ak + sk <= 160;
}

// zero-fill (hipMemsetAsync's fill kernel took 0.7 ms for the 71 MB bucket-count array: ~100 GB/s)
__global__ __launch_bounds__(256) void k_zero(uint4* __restrict__ p, size_t n16) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = z;
}
void launch_zero(void* p, size_t n16, hipStream_t st) { hipLaunchKernelGGL(k_zero, dim3(2048), dim3(256), 0, st, (uint4*)p, n16); }

// scalar-range tasks: dst = words [w0, w0 + nw) of every 8-word scalar, zero-extended to 8 words
__global__ __launch_bounds__(256) void k_extract_range(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t n, uint32_t w0,
                                                       uint32_t nw) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel
    const uint64_t total = n * 8;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = (uint32_t)(i & 7u);
        dst[i] = j < nw ? src[(i & ~(uint64_t)7) + w0 + j] : 0u;
    }
}

// ------------------------------------------------------------------------------------------------
// exclusive scan of (count, units(count)) packed in one u64: low = entries, high = units
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 8;
static_assert(SCAN_TILE == 256 * SCAN_ITEMS, "a scan block of 256 lanes takes SCAN_ITEMS buckets per lane");

__device__ __forceinline__ uint64_t pack_cu(uint32_t cnt, uint32_t L) {
    return (uint64_t)cnt | ((uint64_t)((cnt + L - 1) / L) << 32);
}
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* sh) {
    // wave reduce then across 4 waves
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    uint64_t t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void k_scan_reduce(const uint32_t* __restrict__ count, uint64_t G, uint32_t L,
                                                     uint64_t* __restrict__ blocksums, uint32_t* __restrict__ stats) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    __shared__ uint64_t sh[4];
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t acc = 0;
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        if (i < G) {
            uint32_t cn = count[i];
            acc += pack_cu(cn, L);
            mx = cn > mx ? cn : mx;
        }
    }
    uint64_t tot = block_sum_u64(acc, sh);
    for (int o = 32; o > 0; o >>= 1) { uint32_t t = __shfl_down(mx, o, 64); mx = t > mx ? t : mx; }
    // (guarded: 5 x 10^4 unconditional atomics on one address cost 0.5 ms; the value only grows)
    if ((threadIdx.x & 63) == 0 && mx > *(volatile uint32_t*)&stats[1]) atomicMax(&stats[1], mx);
    if (threadIdx.x == 0) blocksums[blockIdx.x] = tot;
}

// single block: exclusive scan of blocksums in place; totals -> stats[0] (units), stats[2] (entries)
// (256 threads: the kernel belongs to the sort stage, which may have to fit beside another task's accumulation -
// a 1024-thread block needs four waves per SIMD at once and 4 x its registers of the ~100 VGPRs the accumulation leaves)
constexpr int SCAN_SUMS_THREADS = 256;
__global__ __launch_bounds__(SCAN_SUMS_THREADS) void k_scan_sums(uint64_t* __restrict__ blocksums, uint32_t nblocks,
                                                                 uint32_t* __restrict__ stats) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    __shared__ uint64_t sh[SCAN_SUMS_THREADS];
    __shared__ uint64_t carry_sh;
    if (threadIdx.x == 0) carry_sh = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += SCAN_SUMS_THREADS) {
        uint32_t i = base + threadIdx.x;
        uint64_t v = i < nblocks ? blocksums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < SCAN_SUMS_THREADS; o <<= 1) {
            uint64_t t = threadIdx.x >= (uint32_t)o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        uint64_t incl = sh[threadIdx.x];
        uint64_t carry = carry_sh;
        if (i < nblocks) blocksums[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == SCAN_SUMS_THREADS - 1) carry_sh = carry + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = (uint32_t)(carry_sh >> 32);
        stats[2] = (uint32_t)(carry_sh & 0xffffffffu);
    }
}

// per-block exclusive scan with the block's base; writes off[], unit_off[] and turns count[] into
// the scatter cursor (count[g] = off[g]).  Element G (one past the end) receives the totals.
__global__ __launch_bounds__(256) void k_scan_final(uint32_t* __restrict__ count, uint64_t G, uint32_t L,
                                                    const uint64_t* __restrict__ blocksums,
                                                    uint32_t* __restrict__ off, uint32_t* __restrict__ unit_off) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    __shared__ uint64_t sh[256];
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS];
    uint64_t tsum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        v[k] = i < G ? pack_cu(count[i], L) : 0;
        tsum += v[k];
    }
    sh[threadIdx.x] = tsum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        uint64_t t = threadIdx.x >= (uint32_t)o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    uint64_t run = blocksums[blockIdx.x] + sh[threadIdx.x] - tsum;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        if (i <= G) {
            off[i] = (uint32_t)(run & 0xffffffffu);
            unit_off[i] = (uint32_t)(run >> 32);
            if (i < G) count[i] = (uint32_t)(run & 0xffffffffu);
        }
        run += v[k];
    }
}

// ------------------------------------------------------------------------------------------------
// Units ordered by run length (descending), so the 64 lanes of a wave walk runs of equal length:
// with uniform scalars the runs are Poisson (mean n/2^(c-1)), and bucket order costs ~30% of the
// lanes to divergence.  Counting sort over <= 1025 length bins, LDS-privatised; both kernels walk the
// buckets in order (coalesced reads of off / unit_off), one lane per bucket.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t UNITS_INLINE = 8;   // buckets with more units than this are filled by the whole block

// unit -> bucket map + histogram of unit lengths.  Grid-stride over chunks of 256 buckets: the LDS
// histogram is flushed once per block (one block per chunk meant 10^5 blocks x 257 global atomics on
// the same 257 addresses: 1.3 ms at 2^26, all of it atomic serialisation).
constexpr uint32_t UNIT_GRID = 2048;

__global__ __launch_bounds__(256) void k_fill_units(const uint32_t* __restrict__ off, const uint32_t* __restrict__ unit_off,
                                                    uint64_t G, uint32_t L, uint32_t* __restrict__ unit_bucket,
                                                    uint32_t* __restrict__ hist) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    __shared__ uint32_t sh[MAX_L + 1];
    __shared__ uint32_t big[256], nbig;
    for (uint32_t i = threadIdx.x; i <= L; i += 256) sh[i] = 0;
    const uint64_t nchunks = (G + 255) / 256;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x == 0) nbig = 0;
        __syncthreads();
        // a bucket of cnt entries has cnt / L full units and one unit of cnt % L entries
        const uint64_t g0 = chunk * 256;
        uint64_t g = g0 + threadIdx.x;
        if (g < G) {
            uint32_t u0 = unit_off[g], u1 = unit_off[g + 1];
            uint32_t cnt = off[g + 1] - off[g];
            uint32_t nfull = cnt / L, rem = cnt - nfull * L;
            if (nfull) atomicAdd(&sh[L], nfull);
            if (rem) atomicAdd(&sh[rem], 1u);
            if (u1 - u0 > UNITS_INLINE) big[atomicAdd(&nbig, 1u)] = threadIdx.x;   // hot bucket: the block fills it together
            else for (uint32_t u = u0; u < u1; ++u) unit_bucket[u] = (uint32_t)g;
        }
        __syncthreads();
        for (uint32_t b = 0; b < nbig; ++b) {
            uint64_t gb = g0 + big[b];
            uint32_t u0 = unit_off[gb], u1 = unit_off[gb + 1];
            for (uint32_t u = u0 + threadIdx.x; u < u1; u += 256) unit_bucket[u] = (uint32_t)gb;
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i <= L; i += 256)
        if (sh[i]) atomicAdd(&hist[i], sh[i]);
}

// cursor[len] = number of units strictly longer than len (descending order); one block
__global__ __launch_bounds__(256) void k_unit_len_scan(const uint32_t* __restrict__ hist, uint32_t L,
                                                       uint32_t* __restrict__ cursor) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    if (threadIdx.x != 0) return;
    uint32_t run = 0;
    for (int len = (int)L; len >= 0; --len) {
        cursor[len] = run;
        run += hist[len];
    }
}

__global__ __launch_bounds__(256) void k_unit_order(const uint32_t* __restrict__ off, const uint32_t* __restrict__ unit_off,
                                                    uint64_t G, uint32_t L, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ unit_order) {
    __builtin_amdgcn_s_setprio(3);   // sort-stage kernel: may run underneath another task's accumulation (msm_sort3.hip)
    __shared__ uint32_t sh_cnt[MAX_L + 1];
    __shared__ uint32_t sh_base[MAX_L + 1];
    __shared__ uint32_t big[256], big_pos[256], nbig;
    for (uint32_t i = threadIdx.x; i <= L; i += 256) sh_cnt[i] = 0;
    __syncthreads();
    const uint64_t nchunks = (G + 255) / 256;
    // pass 1 over this block's chunks: how many units of each length
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint64_t g = chunk * 256 + threadIdx.x;
        if (g < G) {
            uint32_t cnt = off[g + 1] - off[g];
            uint32_t nfull = cnt / L, rem = cnt - nfull * L;
            if (nfull) atomicAdd(&sh_cnt[L], nfull);
            if (rem) atomicAdd(&sh_cnt[rem], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= L; i += 256) {
        uint32_t v = sh_cnt[i];
        sh_base[i] = v ? atomicAdd(&cursor[i], v) : 0u;
        sh_cnt[i] = 0;
    }
    // pass 2: place
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x == 0) nbig = 0;
        __syncthreads();
        const uint64_t g0 = chunk * 256;
        uint64_t g = g0 + threadIdx.x;
        if (g < G) {
            uint32_t u0 = unit_off[g];
            uint32_t cnt = off[g + 1] - off[g];
            uint32_t nfull = cnt / L, rem = cnt - nfull * L;
            if (nfull) {
                uint32_t pos = sh_base[L] + atomicAdd(&sh_cnt[L], nfull);
                if (nfull > UNITS_INLINE) {
                    uint32_t q = atomicAdd(&nbig, 1u);
                    big[q] = threadIdx.x;
                    big_pos[q] = pos;
                } else {
                    for (uint32_t k = 0; k < nfull; ++k) unit_order[pos + k] = u0 + k;
                }
            }
            if (rem) unit_order[sh_base[rem] + atomicAdd(&sh_cnt[rem], 1u)] = u0 + nfull;
        }
        __syncthreads();
        for (uint32_t b = 0; b < nbig; ++b) {
            uint64_t gb = g0 + big[b];
            uint32_t ub = unit_off[gb];
            uint32_t nf = (off[gb + 1] - off[gb]) / L, pos = big_pos[b];
            for (uint32_t k = threadIdx.x; k < nf; k += 256) unit_order[pos + k] = ub + k;
        }
        __syncthreads();
    }
}

int launch_fill_units(const MsmStep& C, uint32_t U /* upper bound of the unit count */) {
    const uint64_t G = C.P.G;
    const uint32_t L = C.P.L;
    hipStream_t st = C.sort_stream;
    MsmEngine::SortBufs& B = C.B;
    BLZ_TRY(B.unit_bucket.reserve(((size_t)U + 1) * 4));
    BLZ_TRY(B.unit_order.reserve(((size_t)U + 1) * 4));
    BLZ_TRY(B.lenhist.reserve(2 * (MAX_L + 1) * 4));
    uint32_t* hist = B.lenhist.as<uint32_t>();
    uint32_t* cursor = hist + (MAX_L + 1);
    BLZ_HIP(hipMemsetAsync(hist, 0, 2 * (MAX_L + 1) * 4, st), BLZ_ERR_UNKNOWN);
    uint64_t nchunks = (G + 255) / 256;
    dim3 gg((uint32_t)(nchunks < UNIT_GRID ? nchunks : UNIT_GRID)), b(256);
    hipLaunchKernelGGL(k_fill_units, gg, b, 0, st, B.off.as<uint32_t>(), B.unit_off.as<uint32_t>(), G, L, B.unit_bucket.as<uint32_t>(), hist);
    hipLaunchKernelGGL(k_unit_len_scan, dim3(1), b, 0, st, hist, L, cursor);
    hipLaunchKernelGGL(k_unit_order, gg, b, 0, st, B.off.as<uint32_t>(), B.unit_off.as<uint32_t>(), G, L, cursor, B.unit_order.as<uint32_t>());
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

// count[] -> off[], unit_off[] (+ the totals in `stats`); count[] becomes the scatter cursor
static void launch_scans(MsmEngine& E, const MsmStep& C) {
    const uint64_t G = C.P.G;
    const uint32_t nscan = (uint32_t)((G + 1 + SCAN_TILE - 1) / SCAN_TILE);
    MsmEngine::SortBufs& B = C.B;
    hipStream_t ss = C.sort_stream;
    dim3 b256(256);
    hipLaunchKernelGGL(k_scan_reduce, dim3(nscan), b256, 0, ss, B.count.as<uint32_t>(), G, C.P.L, E.blocksums.as<uint64_t>(),
                       B.stats.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_SUMS_THREADS), 0, ss, E.blocksums.as<uint64_t>(), nscan, B.stats.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_final, dim3(nscan), b256, 0, ss, B.count.as<uint32_t>(), G, C.P.L, E.blocksums.as<uint64_t>(),
                       B.off.as<uint32_t>(), B.unit_off.as<uint32_t>());
}

// the sort stage of a piece: np points whose scalars start at d_scalars (np x sbits / 8 bytes)
int msm_sort_stage(MsmEngine& E, const MsmStep& C, const void* d_scalars, uint32_t np) {
    MsmSlot& S = C.S;
    MsmEngine::SortBufs& B = C.B;
    hipStream_t ss = C.sort_stream;
    const char* sc_s = (const char*)d_scalars;
    if (S.ranged) {
        // the range of every scalar as a scalar of its own (zero-extended): everything downstream reads 32-byte scalars and
        // walks the plan's windows from bit 0; k_finish puts the 2^bit_lo back (FinishPlan offsets)
        BLZ_TRY(B.range_scalars.reserve((size_t)np * 32 + 16));
        hipLaunchKernelGGL(k_extract_range, dim3(2048), dim3(256), 0, ss, (const uint32_t*)sc_s, B.range_scalars.as<uint32_t>(),
                           (uint64_t)np, (uint32_t)(S.bit_lo >> 5), (uint32_t)((S.bit_hi - S.bit_lo) >> 5));
        sc_s = (const char*)B.range_scalars.p;
    }
    BLZ_HIP(hipMemsetAsync(B.stats.p, 0, 64, ss), BLZ_ERR_UNKNOWN);
    // No host round trip: the unit count stays on the device.  Buffers and grids are sized by the bound
    // (every bucket at most one short unit, plus entries / L full ones) and the kernels read the real count
    // from `stats`; the host copy is for the log line, the sanity check of finish() and the hot-bucket guard.
    auto stats_to_host = [&]() -> int {
        BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
        return copy_words_to_pinned(S.stats_h, B.stats.p, 4, ss);
    };
    switch (S.sort.kind) {
        case SortPlan::TINY:   // digits, bucket scan, entries, unit lists, stats: one block's work
            BLZ_TRY(msm_sort_tiny(E, C, sc_s, np, S.sbits, (uint32_t)S.max_units));
            BLZ_TRY(stats_to_host());
            break;
        case SortPlan::S3:     // count[] and entries[] in one go
            BLZ_TRY(msm_sort3(E, C, sc_s, np, S.sbits));
            launch_scans(E, C);
            BLZ_TRY(stats_to_host());
            BLZ_TRY(launch_fill_units(C, (uint32_t)S.max_units));
            break;
        case SortPlan::LDS: {  // count[]; entries[] behind the scan
            launch_zero(B.count.p, ((C.P.G + 1) * 4 + 15) / 16, ss);   // (the reserve of begin() rounds the allocation up)
            LdsSortPass pass;
            BLZ_TRY(msm_sort_lds(E, C, sc_s, np, S.sbits, pass));
            launch_scans(E, C);
            BLZ_TRY(msm_sort_lds_scatter(E, C, pass));
            BLZ_TRY(stats_to_host());
            BLZ_TRY(launch_fill_units(C, (uint32_t)S.max_units));
            break;
        }
    }
    return BLZ_OK;
}

}  // namespace blz
