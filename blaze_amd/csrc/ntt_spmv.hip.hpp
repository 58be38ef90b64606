// Sparse matrix-vector products on resident buffers (blz_ntt_vec_spmv): dst[p] = sum over the nonzeros k of row p of
// val[k] x[col[k] mod count], 0 for an empty row and for rows <= p < n.  The matrix is CSR (row_ptr, col, val) in the caller's
// device memory; without row_ptr row p holds nonzero p alone (the data-dependent gather), without val every coefficient is 1.
// Words are plain integers on the wire; any 256-bit word of x or val counts as its residue, every output word is canonical.
//
// k_spmv_index  index mode.  The shape of k_gather_strided: a grid-stride loop, one position per lane per step, destination
//               contiguous; the lane reads col[p] (coalesced), then the source word, then val[p].  With val the product is
//               vec_mul's two Montgomery products, without it vec_canon alone.  Positions >= rows store zeros and load nothing.
// k_spmv_tile   CSR mode, work split by NONZEROS: a block owns a tile of SPMV_TILE = 1024 consecutive nonzeros, lane t the four
//               consecutive ones 4t .. 4t + 3, so a row of any length is spread over lanes and tiles like every other.
//               Lane 0 finds the rows of the tile's first and last nonzero by binary search in row_ptr (the SPAN); where the
//               span has at most SPMV_SPAN entries it is copied into LDS, else it is read where it lies.  A lane finds the row
//               of its first nonzero by binary search in the span; where a row ends it searches again from the next row up,
//               so a run of empty rows costs log2 of the span, not its length.
//               The term of a nonzero is ONE product under DOT's rule (ntt_fold.hip.hpp): mont(x, canon(val)) = x val / R is below
//               2m for any 256-bit x; the stray 1 / R comes off once per finished sum (a product by R^2).  Without val: vec_canon
//               and additions.  The lane folds a run of nonzeros of one row in registers.  A row that begins and ends inside
//               the lane is stored at once.  The lane's LAST run (its only one, if all four nonzeros share a row) enters a
//               segmented inclusive scan over the 256 lanes in LDS, keyed by row - 8 Kogge-Stone steps, additions only; the
//               keys are nondecreasing, so "same key w lanes down" means the same row all the way.  The lane's FIRST run, if
//               a second follows it, ends a row: its sum plus the scanned value of the lane below (same row only) is that
//               row's.  A lane whose last run's row differs from the next lane's first closes that row with its scanned value.
//               Every row met in the tile is closed exactly once.  A row complete inside the tile is stored (canonical); one
//               that began before the tile (HEAD) or continues behind it (TAIL) leaves its sum - finished, canonical - and its
//               row id in the tile's 128 bytes of workspace.
// k_spmv_carry  one lane per tile whose TAIL is set: the row that begins there.  It adds the HEADs of the tiles behind for as
//               long as they carry on the same row, and stores.  Additions of canonical words only; a row of L nonzeros is at
//               most L / 1024 + 1 dependent additions in one lane, read SPMV_CARRY_BATCH tiles at a time: L / 8192 dependent
//               memory round trips.
// Rows without a nonzero are visited by no tile: the caller zeroes dst first (hipMemsetAsync on the same stream, ntt.hip).
// Sums are exact in the field, so no result depends on the order in which blocks run; no atomics, no flags, every dependency
// between blocks is a launch.
//
// The host never reads the arrays.  Every nonzero index is clamped to nnz, every row a search returns lies in [0, rows), every
// column is masked to the source: whatever bytes row_ptr and col hold, nothing outside the four arrays, dst and the workspace
// is touched.  row_ptr that is not nondecreasing with row_ptr[rows] <= nnz gives an unspecified dst.
//
// WORKSPACE (CSR mode with more than one tile): tiles x 32 dwords of the handle's `scratch` - HEAD word, TAIL word, then
// {head row, tail row, head carries on} with SPMV_NONE for "no such row".  nnz <= 256 n holds it within n x 32 bytes.
#pragma once
#include "ntt_vec.hip.hpp"

namespace blz {

constexpr uint32_t SPMV_PER_LANE = 4;
constexpr uint32_t SPMV_TILE = VEC_THREADS * SPMV_PER_LANE;
constexpr uint32_t SPMV_SPAN = 2048;         // row_ptr entries of a tile's span kept in LDS
constexpr uint32_t SPMV_WS_DWORDS = 32;      // per tile
constexpr uint32_t SPMV_CARRY_BATCH = 8;     // tiles k_spmv_carry reads per step
constexpr uint32_t SPMV_NONE = 0xffffffffu;  // no row: above every row id (rows <= 2^27)

template <class Fr, bool HAS_VAL>
__global__ __launch_bounds__(VEC_THREADS) void k_spmv_index(uint32_t* dst, NttVecArg x, const uint32_t* col, const uint32_t* val,
                                                            uint64_t rows, uint64_t n) {
    using E = Fp<Fr>;
    const uint64_t step = (uint64_t)gridDim.x * VEC_THREADS;
    for (uint64_t e = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; e < n; e += step) {
        E r;
        if (e < rows) {
            E xv;
            fp_load(xv, x.p + ((uint64_t)col[e] & x.mask) * 8);
            if constexpr (HAS_VAL) {
                E v;
                fp_load(v, val + e * 8);
                vec_mul(r, xv, v);
            } else {
                r = xv;
                vec_canon(r);
            }
            fp_reduce(r);
        } else {
            fp_zero(r);
        }
        fp_store(dst + e * 8, r);
    }
}

// what lane 0 of a tile works out for the block
struct SpmvSpan {
    uint32_t l0, l1;     // the tile's live nonzeros [l0, l1): inside the tile and inside [row_ptr[0], row_ptr[rows])
    uint32_t rlo, rhi;   // their first and last row
    uint32_t open0;      // row rlo began before the tile
    uint32_t open1;      // row rhi continues behind it
    uint32_t in_lds;     // row_ptr[rlo .. rhi + 1] sits in LDS
};

// the largest r in [lo, hi] with at(r) <= k, lo where there is none (or hi < lo): always inside [lo, max(lo, hi)]
template <class At>
BLZ_DEV uint32_t spmv_row_of(At&& at, uint32_t lo, uint32_t hi, uint32_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (at(mid) <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class Fr, bool HAS_VAL>
__global__ __launch_bounds__(VEC_THREADS) void k_spmv_tile(uint32_t* dst, uint32_t* ws, NttVecArg x, const uint32_t* row_ptr,
                                                           const uint32_t* col, const uint32_t* val, uint32_t rows, uint32_t nnz) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t sum[VEC_THREADS * 8];
    __shared__ uint32_t key_first[VEC_THREADS], key_last[VEC_THREADS];
    __shared__ uint32_t span[SPMV_SPAN];
    __shared__ SpmvSpan sp_lds;
    const uint32_t t = threadIdx.x;
    const bool tiled = gridDim.x > 1;   // a single tile has no neighbour and no workspace
    uint32_t* const wt = ws + (size_t)blockIdx.x * SPMV_WS_DWORDS;
    if (t == 0) {
        SpmvSpan s{};
        const uint32_t k0 = blockIdx.x * SPMV_TILE;
        const uint32_t k1 = nnz - k0 < SPMV_TILE ? nnz : k0 + SPMV_TILE;
        const uint32_t a0 = row_ptr[0] < nnz ? row_ptr[0] : nnz;
        const uint32_t a1 = row_ptr[rows] < nnz ? row_ptr[rows] : nnz;
        s.l0 = k0 > a0 ? k0 : a0;
        s.l1 = k1 < a1 ? k1 : a1;
        if (s.l0 < s.l1) {
            auto at = [&](uint32_t i) { return row_ptr[i]; };
            s.rlo = spmv_row_of(at, 0u, rows - 1, s.l0);
            s.rhi = spmv_row_of(at, s.rlo, rows - 1, s.l1 - 1);
            s.open0 = tiled && row_ptr[s.rlo] < s.l0;
            s.open1 = tiled && row_ptr[s.rhi + 1] > s.l1;
            s.in_lds = s.rhi - s.rlo + 2 <= SPMV_SPAN;
        }
        if (tiled) {
            const bool one_row = s.rlo == s.rhi;
            wt[16] = s.open0 ? s.rlo : SPMV_NONE;
            wt[17] = s.open1 && !(s.open0 && one_row) ? s.rhi : SPMV_NONE;
            wt[18] = s.open0 && s.open1 && one_row;
        }
        sp_lds = s;
    }
    __syncthreads();
    const SpmvSpan sp = sp_lds;
    if (sp.l0 >= sp.l1) return;   // (the whole block)
    if (sp.in_lds) {
        for (uint32_t i = t; i < sp.rhi - sp.rlo + 2; i += VEC_THREADS) span[i] = row_ptr[sp.rlo + i];
        __syncthreads();
    }
    auto at = [&](uint32_t i) { return sp.in_lds ? span[i - sp.rlo] : row_ptr[i]; };   // sp.rlo <= i <= sp.rhi + 1

    // a finished sum of row r (sp.rlo <= r <= sp.rhi): into dst, or into the tile's HEAD / TAIL word
    auto emit = [&](uint32_t r, E v) {
        if constexpr (HAS_VAL) fp_to_mont(v, v);   // (sum x val / R) R^2 / R
        fp_reduce(v);
        const bool head = sp.open0 && r == sp.rlo, tail = sp.open1 && r == sp.rhi;
        fp_store(head ? wt : tail ? wt + 8 : dst + (size_t)r * 8, v);
    };

    E acc, first;   // the current run; the lane's first run once a second has begun
    fp_zero(acc);
    fp_zero(first);
    uint32_t cur = SPMV_NONE, row_first = SPMV_NONE, end = 0;
    bool several = false;
    const uint32_t kb = blockIdx.x * SPMV_TILE + t * SPMV_PER_LANE;
#pragma unroll 1
    for (uint32_t j = 0; j < SPMV_PER_LANE; ++j) {
        const uint32_t k = kb + j;
        if (k < sp.l0 || k >= sp.l1) continue;
        if (cur == SPMV_NONE || k >= end) {
            uint32_t from = sp.rlo;
            if (cur != SPMV_NONE) {   // a run has ended, and with it its row
                if (!several) {
                    first = acc;
                    several = true;
                } else {
                    emit(cur, acc);   // began and ended inside the lane
                }
                fp_zero(acc);
                from = cur < sp.rhi ? cur + 1 : sp.rhi;
            }
            cur = spmv_row_of(at, from, sp.rhi, k);
            end = at(cur + 1);
            if (row_first == SPMV_NONE) row_first = cur;
        }
        E term;
        fp_load(term, x.p + ((uint64_t)col[k] & x.mask) * 8);
        if constexpr (HAS_VAL) {
            E v;
            fp_load(v, val + (size_t)k * 8);
            vec_canon(v);
            fp_mul(term, term, v);
        } else {
            vec_canon(term);
        }
        fp_add(acc, acc, term);
    }

    // segmented inclusive scan of the lanes' last runs, keyed by row
    key_first[t] = row_first;
    key_last[t] = cur;
    fp_store(sum + t * 8, acc);
    __syncthreads();
#pragma unroll 1
    for (uint32_t w = 1; w < VEC_THREADS; w <<= 1) {
        const bool take = t >= w && cur != SPMV_NONE && key_last[t - w] == cur;
        E below;
        if (take) fp_load(below, sum + (t - w) * 8);
        __syncthreads();
        if (take) {
            fp_add(acc, acc, below);
            fp_store(sum + t * 8, acc);
        }
        __syncthreads();
    }
    if (several) {   // the first run ended its row inside this lane
        if (t > 0 && key_last[t - 1] == row_first) {
            E below;
            fp_load(below, sum + (t - 1) * 8);
            fp_add(first, first, below);
        }
        emit(row_first, first);
    }
    if (cur != SPMV_NONE && (t == VEC_THREADS - 1 || key_first[t + 1] != cur)) emit(cur, acc);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_spmv_carry(uint32_t* dst, const uint32_t* ws, uint32_t tiles) {
    using E = Fp<Fr>;
    const uint32_t b = blockIdx.x * VEC_THREADS + threadIdx.x;   // (at most 2^21 tiles: the grid covers them, no loop)
    if (b < tiles) {
        const uint32_t* wt = ws + (size_t)b * SPMV_WS_DWORDS;
        const uint32_t r = wt[17];
        if (r == SPMV_NONE) return;
        E acc;
        fp_load(acc, wt + 8);
        // SPMV_CARRY_BATCH tiles per memory round trip: their loads do not depend on one another, only the decision to go on does.
        // A slot past the last tile reads tile `tiles - 1` again, and a tile without a HEAD never wrote that word: both are
        // loaded and neither is used - the row[u] == r gate is closed for them
        bool more = true;
#pragma unroll 1
        for (uint32_t j = b + 1; more && j < tiles; j += SPMV_CARRY_BATCH) {
            uint32_t row[SPMV_CARRY_BATCH], on[SPMV_CARRY_BATCH];
            E head[SPMV_CARRY_BATCH];
#pragma unroll
            for (uint32_t u = 0; u < SPMV_CARRY_BATCH; ++u) {
                const bool inside = j + u < tiles;
                const uint32_t* wj = ws + (size_t)(inside ? j + u : tiles - 1) * SPMV_WS_DWORDS;
                row[u] = inside ? wj[16] : SPMV_NONE;
                on[u] = wj[18];
                fp_load(head[u], wj);
            }
#pragma unroll
            for (uint32_t u = 0; u < SPMV_CARRY_BATCH; ++u) {
                more = more && row[u] == r;
                if (more) fp_add(acc, acc, head[u]);
                more = more && on[u] != 0;
            }
        }
        fp_reduce(acc);
        fp_store(dst + (size_t)r * 8, acc);
    }
}

// dst: n words that x's do not overlap.  row_ptr == nullptr: index mode, rows == nnz <= n, every position of dst is written.
// Otherwise dst must hold zeros already (rows without a nonzero are not visited); rows >= 1, nnz >= 1, and with more than one
// tile ws holds tiles x SPMV_WS_DWORDS dwords
template <class Fr>
int ntt_vec_spmv_t(hipStream_t st, uint32_t* dst, NttVecArg x, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* val,
                   uint64_t rows, uint64_t nnz, uint64_t n, uint32_t* ws) {
    const dim3 thr(VEC_THREADS);
    if (!row_ptr) {
        const uint64_t blocks = (n + VEC_THREADS - 1) / VEC_THREADS;
        const dim3 grid((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS));
        if (val) hipLaunchKernelGGL((k_spmv_index<Fr, true>), grid, thr, 0, st, dst, x, col, val, rows, n);
        else hipLaunchKernelGGL((k_spmv_index<Fr, false>), grid, thr, 0, st, dst, x, col, val, rows, n);
    } else {
        const uint32_t tiles = (uint32_t)((nnz + SPMV_TILE - 1) / SPMV_TILE);
        if (val) hipLaunchKernelGGL((k_spmv_tile<Fr, true>), dim3(tiles), thr, 0, st, dst, ws, x, row_ptr, col, val, (uint32_t)rows, (uint32_t)nnz);
        else hipLaunchKernelGGL((k_spmv_tile<Fr, false>), dim3(tiles), thr, 0, st, dst, ws, x, row_ptr, col, val, (uint32_t)rows, (uint32_t)nnz);
        if (tiles > 1) {
            hipLaunchKernelGGL(k_spmv_carry<Fr>, dim3((tiles + VEC_THREADS - 1) / VEC_THREADS), thr, 0, st, dst, (const uint32_t*)ws, tiles);
        }
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
