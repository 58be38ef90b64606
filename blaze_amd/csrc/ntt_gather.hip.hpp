// Gathers on resident buffers (blz_ntt_vec_gather): dst[p] = a[(offset + stride p) mod count] for p < len, 0 for len <= p < n.
// The one op of the family that moves an element to another position, or between vectors of different length: a rotation
// (Z(wX) next to Z(X)), a low-degree extension (count < n, zero above), a slice of a longer vector (count > n), a decimation
// (every 4th value of a 4n domain), a reversal, a broadcast.  A canonicalising copy: any 256-bit source word counts as its
// residue (vec_canon, then the final reduction of the element-wise ops); no Montgomery product, no LDS, no workspace.
//
// The shape is k_vec_ew's: 256 lanes, at most VEC_MAX_BLOCKS blocks, a grid-stride loop, one 32-byte word per lane per step as
// two 16-byte accesses.  The DESTINATION is always contiguous (a wave stores 2 KiB); only the source address differs:
//   k_gather_contig   stride = 1 (mod count): the source word of position e is (offset + e) & mask - one 64-bit add and one
//                     AND off the loop counter, contiguous apart from the wrap (once for a rotation, every `count` positions
//                     where len > count tiles the source).
//   k_gather_strided  any other stride: the lane multiplies ONCE (stride x its first position) and then carries the index,
//                     adding the wave-uniform stride x grid step per turn; the wrap at 2^64 is harmless, count divides it.
//                     stride = 0 (a broadcast), an even stride (words read more than once) and stride = count - 1 (backwards)
//                     all come out of the one formula.  A wave reads 64 words `stride` apart: what that costs is the memory
//                     system's to say (stride 4 fetches four times the bytes it uses).
// The variant is chosen from the reduced stride alone (ntt_vec_gather_t).  Positions p >= len store zeros and load nothing.
// dst must NOT overlap a's words: a lane writes positions other lanes still read.  The handle gathers into its scratch and
// copies back when a names the destination buffer (ntt.hip).
#pragma once
#include "ntt_vec.hip.hpp"

namespace blz {

// word `idx` of a -> position e of dst, canonical; zero where e >= len
template <class Fr>
BLZ_DEV void gather_word(uint32_t* dst, NttVecArg a, uint64_t idx, uint64_t e, uint64_t len) {
    Fp<Fr> x;
    if (e < len) {
        fp_load(x, a.p + (idx & a.mask) * 8);
        vec_canon(x);
        fp_reduce(x);
    } else {
        fp_zero(x);
    }
    fp_store(dst + e * 8, x);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_gather_contig(uint32_t* dst, NttVecArg a, uint64_t offset, uint64_t len, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * VEC_THREADS;
    for (uint64_t e = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x; e < n; e += step) gather_word<Fr>(dst, a, offset + e, e, len);
}

template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_gather_strided(uint32_t* dst, NttVecArg a, uint64_t offset, uint64_t stride,
                                                                 uint64_t len, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * VEC_THREADS;
    const uint64_t istep = stride * step;   // wave-uniform
    uint64_t e = (uint64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    for (uint64_t idx = offset + stride * e; e < n; e += step, idx += istep) gather_word<Fr>(dst, a, idx, e, len);
}

// offset < count = a.mask + 1, stride already reduced modulo count, len <= n; dst: n words that a's do not overlap
template <class Fr>
int ntt_vec_gather_t(hipStream_t st, uint32_t* dst, NttVecArg a, uint64_t offset, uint64_t stride, uint64_t len, uint64_t n) {
    const uint64_t blocks = (n + VEC_THREADS - 1) / VEC_THREADS;
    const dim3 grid((unsigned)(blocks < VEC_MAX_BLOCKS ? blocks : VEC_MAX_BLOCKS)), thr(VEC_THREADS);
    // count = 1: every stride is 0 = 1 (mod 1), and (offset + e) & 0 reads the one word
    if (((stride - 1) & a.mask) == 0)
        hipLaunchKernelGGL(k_gather_contig<Fr>, grid, thr, 0, st, dst, a, offset, len, n);
    else
        hipLaunchKernelGGL(k_gather_strided<Fr>, grid, thr, 0, st, dst, a, offset, stride, len, n);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
