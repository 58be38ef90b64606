// Scatter-add on resident buffers (blz_ntt_vec_scatter): dst[t] = sum over the nonzeros k < nnz with (idx[k] mod n) == t of
// val[k] x[src(k) mod count], src(k) = src ? src[k] : k; 0 for a position no nonzero names.  Without val every coefficient is 1,
// without x every x word is 1, without both dst[t] is the number of nonzeros that name t (the histogram).  Words are plain
// integers on the wire; any 256-bit word of x or val counts as its residue, every output word is canonical.
//
// A field word cannot be added atomically; its limbs can.  A term is eight 32-bit limbs - a product below 3m, or the raw word
// of the one operand present: any value below 2^256 is a term, the residue is taken once per position at the end - and limb i
// of every term of position t is added into a 64-bit accumulator of its own.  nnz <= 2^31 terms of limbs below 2^32: no
// accumulator reaches 2^63.  Integer addition is associative, so the eight sums, and with them the result, do not depend on the
// order in which lanes, waves and blocks arrive: two runs give the same bytes.
//
// ACCUMULATORS of position t: limbs 0 .. 3 are the four uint64 at dst + 32 t bytes - the position's own word - and limbs 4 .. 7
// the four at ws + 32 t bytes.  Both are zeroed on the stream ahead of the kernels (ntt_vec_scatter_t).
//
// k_scatter_add      a grid-stride loop over the nonzeros, a step of the block is SCATTER_THREADS of them.  Lane l computes the
//                    term of nonzero base + l - every lane of the wave multiplies, none idles - and leaves its limbs and its
//                    position in LDS.  Then eight rounds: in round i the eight lanes 8g .. 8g + 7 add nonzero base + 8g + i, lane
//                    j its limb j: one return-less 64-bit atomic instruction of the wave covers eight nonzeros x (32 contiguous
//                    bytes of dst + 32 of ws) - two 64-byte requests at the memory side per nonzero where one lane issuing its
//                    eight adds alone would make eight.
// k_scatter_fin      one lane per position: the eight accumulators, carries propagated into nine limbs (the value is below
//                    2^287), the ninth folded in as top 2^256 mod m (one Montgomery product by R^2), the canonical word stored
//                    over the position's own four accumulators - read and written by the same lane.
// k_scatter_count    the histogram: one lane per nonzero, one 32-bit atomic add of 1 into ws[t] (4 n bytes).  No field
//                    arithmetic; a template only so that each field's translation unit owns its copy.
// k_scatter_count_fin  dst[t] = the count: below 2^32, below m, canonical as it stands.
// SMALL DESTINATIONS (n <= SCATTER_LDS_ADD / SCATTER_LDS_COUNT - the path depends on n and the mode, never on the data): all
// accumulators of the destination fit a block's LDS, n x 64 or n x 4 bytes.  k_scatter_add_lds / k_scatter_count_lds: a block
// accumulates its share of the nonzeros there with LDS atomics - one lane per nonzero, its eight limbs in turn; LDS has no
// 64-byte requests to save - and after a barrier adds its NONZERO accumulators to the global ones above, eight consecutive
// lanes the eight of a position.  The finish kernels are the same.  At most SCATTER_LDS_BLOCKS blocks, and no more than one
// per 4 n nonzeros: the flush is n x 8 (or n) atomics per block and stays below a quarter of the adds it saves.
// No flags, no spinning, no compare-and-swap: every dependency between kernels is a launch.
//
// The host never reads the arrays.  idx is masked to n, src to x's count, k < nnz: whatever bytes the arrays hold, nothing
// outside them, dst and the workspace is touched.
//
// WORKSPACE: n x 32 bytes of the handle's `scratch` in add mode (limbs 4 .. 7), n x 4 in count mode.
#pragma once
#include "ntt_vec.hip.hpp"

namespace blz {

constexpr uint32_t SCATTER_THREADS = VEC_THREADS;
constexpr uint32_t SCATTER_MAX_BLOCKS = 1024;   // 256 CUs x 4 blocks: sixteen waves a CU keep the memory side's atomic units fed
constexpr uint32_t SCATTER_TURN = SCATTER_MAX_BLOCKS * SCATTER_THREADS;   // nonzeros per turn of the grid-stride loops
constexpr uint64_t SCATTER_LDS_ADD = 1024;      // n up to which add mode accumulates in LDS: n x 64 bytes, 64 KiB
constexpr uint64_t SCATTER_LDS_COUNT = 16384;   // ... and count mode: n x 4 bytes, 64 KiB
constexpr uint32_t SCATTER_LDS_BLOCKS = 512;    // two blocks of 64 KiB a CU

BLZ_DEV void scatter_add64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// accumulator j (0 .. 7) of position t
BLZ_DEV unsigned long long* scatter_slot(unsigned long long* lo, unsigned long long* hi, uint32_t t, uint32_t j) {
    return (j < 4 ? lo : hi) + (size_t)t * 4 + (j & 3u);
}

// the term of nonzero k: a product below 3m, or the one operand's word as it stands
template <class Fr, bool HAS_X, bool HAS_VAL>
BLZ_DEV void scatter_term(Fp<Fr>& term, NttVecArg x, const uint32_t* src, const uint32_t* val, uint32_t k) {
    static_assert(HAS_X || HAS_VAL, "without both it is the histogram");
    Fp<Fr> v;
    if constexpr (HAS_VAL) fp_load(v, val + (size_t)k * 8);
    if constexpr (HAS_X) {
        const uint64_t s = src ? src[k] : k;
        fp_load(term, x.p + (s & x.mask) * 8);
        if constexpr (HAS_VAL) vec_mul(term, term, v);
    } else {
        term = v;
    }
}

template <class Fr, bool HAS_X, bool HAS_VAL>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_add(unsigned long long* lo, unsigned long long* hi, NttVecArg x,
                                                                 const uint32_t* idx, const uint32_t* src, const uint32_t* val,
                                                                 uint32_t nnz, uint32_t mask) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t limbs[SCATTER_THREADS * 8];
    __shared__ uint32_t pos[SCATTER_THREADS];
    const uint32_t l = threadIdx.x, j = l & 7u, g = l & ~7u;
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    // (base is the block's: every lane takes every turn and meets every barrier; base < nnz <= 2^31 and step <= 2^18: no wrap)
    for (uint32_t base = blockIdx.x * SCATTER_THREADS; base < nnz; base += step) {
        const uint32_t k = base + l;
        if (k < nnz) {
            E term;
            scatter_term<Fr, HAS_X, HAS_VAL>(term, x, src, val, k);
            fp_store(limbs + l * 8, term);
            pos[l] = idx[k] & mask;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t s = g + i;   // the group's nonzero of this round
            if (base + s < nnz) scatter_add64(scatter_slot(lo, hi, pos[s], j), limbs[s * 8 + j]);
        }
        __syncthreads();
    }
}

template <class Fr, bool HAS_X, bool HAS_VAL>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_add_lds(unsigned long long* lo, unsigned long long* hi, NttVecArg x,
                                                                     const uint32_t* idx, const uint32_t* src, const uint32_t* val,
                                                                     uint32_t nnz, uint32_t mask) {
    using E = Fp<Fr>;
    __shared__ unsigned long long acc[SCATTER_LDS_ADD * 8];
    const uint32_t l = threadIdx.x, slots = (mask + 1u) * 8u;   // mask < SCATTER_LDS_ADD
    for (uint32_t i = l; i < slots; i += SCATTER_THREADS) acc[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    for (uint32_t k = blockIdx.x * SCATTER_THREADS + l; k < nnz; k += step) {
        E term;
        scatter_term<Fr, HAS_X, HAS_VAL>(term, x, src, val, k);
        unsigned long long* const a = acc + (idx[k] & mask) * 8u;
#pragma unroll
        for (int i = 0; i < 8; ++i) (void)__hip_atomic_fetch_add(a + i, (unsigned long long)term.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (uint32_t i = l; i < slots; i += SCATTER_THREADS) {
        const unsigned long long v = acc[i];
        if (v != 0) scatter_add64(scatter_slot(lo, hi, i >> 3, i & 7u), v);
    }
}

template <class Fr>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_fin(uint32_t* dst, const unsigned long long* hi, uint32_t n) {
    using E = Fp<Fr>;
    static_assert(Fr::N == 8, "eight limbs, eight accumulators");
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    for (uint32_t t = blockIdx.x * SCATTER_THREADS + threadIdx.x; t < n; t += step) {
        E a, b;   // the accumulators as they lie: (a, b).v[2 i], v[2 i + 1] = accumulator i's halves
        fp_load(a, dst + (size_t)t * 8);
        fp_load(b, hi + (size_t)t * 4);
        E low, top;
        fp_zero(top);
        unsigned long long c = 0;   // below 2^32: an accumulator is below 2^63
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const E& h = i < 4 ? a : b;
            c += (unsigned long long)h.v[2 * (i & 3)] | (unsigned long long)h.v[2 * (i & 3) + 1] << 32;
            low.v[i] = (uint32_t)c;
            c >>= 32;
        }
        top.v[0] = (uint32_t)c;
        fp_to_mont(top, top);   // top R = top 2^256
        fp_reduce(top);
        vec_canon(low);
        fp_add(low, low, top);
        fp_reduce(low);
        fp_store(dst + (size_t)t * 8, low);
    }
}

template <class Fr>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_count(uint32_t* counts, const uint32_t* idx, uint32_t nnz, uint32_t mask) {
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    for (uint32_t k = blockIdx.x * SCATTER_THREADS + threadIdx.x; k < nnz; k += step)
        (void)__hip_atomic_fetch_add(counts + (idx[k] & mask), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class Fr>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_count_lds(uint32_t* counts, const uint32_t* idx, uint32_t nnz, uint32_t mask) {
    __shared__ uint32_t acc[SCATTER_LDS_COUNT];
    const uint32_t l = threadIdx.x, slots = mask + 1u;   // mask < SCATTER_LDS_COUNT
    for (uint32_t i = l; i < slots; i += SCATTER_THREADS) acc[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    for (uint32_t k = blockIdx.x * SCATTER_THREADS + l; k < nnz; k += step)
        (void)__hip_atomic_fetch_add(acc + (idx[k] & mask), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    for (uint32_t i = l; i < slots; i += SCATTER_THREADS) {
        const uint32_t v = acc[i];
        if (v != 0) (void)__hip_atomic_fetch_add(counts + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <class Fr>
__global__ __launch_bounds__(SCATTER_THREADS) void k_scatter_count_fin(uint32_t* dst, const uint32_t* counts, uint32_t n) {
    using E = Fp<Fr>;
    const uint32_t step = gridDim.x * SCATTER_THREADS;
    for (uint32_t t = blockIdx.x * SCATTER_THREADS + threadIdx.x; t < n; t += step) {
        E r;
        fp_zero(r);
        r.v[0] = counts[t];
        fp_store(dst + (size_t)t * 8, r);
    }
}

template <class Fr, bool HAS_X, bool HAS_VAL>
void scatter_launch_add(hipStream_t st, bool lds, unsigned blocks, uint32_t* dst, uint32_t* ws, NttVecArg x, const uint32_t* idx,
                        const uint32_t* src, const uint32_t* val, uint32_t nnz, uint32_t mask) {
    auto* const lo = reinterpret_cast<unsigned long long*>(dst);
    auto* const hi = reinterpret_cast<unsigned long long*>(ws);
    if (lds) hipLaunchKernelGGL((k_scatter_add_lds<Fr, HAS_X, HAS_VAL>), dim3(blocks), dim3(SCATTER_THREADS), 0, st, lo, hi, x, idx, src, val, nnz, mask);
    else hipLaunchKernelGGL((k_scatter_add<Fr, HAS_X, HAS_VAL>), dim3(blocks), dim3(SCATTER_THREADS), 0, st, lo, hi, x, idx, src, val, nnz, mask);
}

// dst: n words that x's do not overlap; 1 <= nnz <= 2^31.  x.p == nullptr: every x word is 1 (src is nullptr then); val ==
// nullptr: every coefficient is 1; both: the histogram.  ws: n x 32 bytes
template <class Fr>
int ntt_vec_scatter_t(hipStream_t st, uint32_t* dst, NttVecArg x, const uint32_t* idx, const uint32_t* src, const uint32_t* val,
                      uint64_t nnz, uint64_t n, uint32_t* ws) {
    const bool count = !x.p && !val;
    const bool lds = n <= (count ? SCATTER_LDS_COUNT : SCATTER_LDS_ADD);
    const uint64_t want = (nnz + SCATTER_THREADS - 1) / SCATTER_THREADS;
    const uint64_t cap = lds ? std::min<uint64_t>(SCATTER_LDS_BLOCKS, std::max<uint64_t>(1, nnz / (4 * n))) : SCATTER_MAX_BLOCKS;
    const unsigned blocks = (unsigned)std::min(want, cap);
    const unsigned fin_blocks = (unsigned)std::min<uint64_t>((n + SCATTER_THREADS - 1) / SCATTER_THREADS, VEC_MAX_BLOCKS);
    const uint32_t z = (uint32_t)nnz, mask = (uint32_t)(n - 1);
    const dim3 thr(SCATTER_THREADS);
    if (count) {
        BLZ_HIP(hipMemsetAsync(ws, 0, n * 4, st), BLZ_ERR_UNKNOWN);
        if (lds) hipLaunchKernelGGL(k_scatter_count_lds<Fr>, dim3(blocks), thr, 0, st, ws, idx, z, mask);
        else hipLaunchKernelGGL(k_scatter_count<Fr>, dim3(blocks), thr, 0, st, ws, idx, z, mask);
        hipLaunchKernelGGL(k_scatter_count_fin<Fr>, dim3(fin_blocks), thr, 0, st, dst, (const uint32_t*)ws, (uint32_t)n);
    } else {
        BLZ_HIP(hipMemsetAsync(dst, 0, n * 32, st), BLZ_ERR_UNKNOWN);
        BLZ_HIP(hipMemsetAsync(ws, 0, n * 32, st), BLZ_ERR_UNKNOWN);
        if (x.p && val) scatter_launch_add<Fr, true, true>(st, lds, blocks, dst, ws, x, idx, src, val, z, mask);
        else if (x.p) scatter_launch_add<Fr, true, false>(st, lds, blocks, dst, ws, x, idx, src, val, z, mask);
        else scatter_launch_add<Fr, false, true>(st, lds, blocks, dst, ws, x, idx, src, val, z, mask);
        hipLaunchKernelGGL(k_scatter_fin<Fr>, dim3(fin_blocks), thr, 0, st, dst, (const unsigned long long*)ws, (uint32_t)n);
    }
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
