// The Fiat-Shamir transcript step (blz_ntt_fs_challenge, and between the rounds of blz_ntt_sumcheck_prove): SHA3-256 (FIPS 202)
// of state || w_0 || .. || w_{count-1}, the digest stored as the new state and, with its top bits cleared, as the challenge.
// Field-independent - the bytes are hashed as stored and the mask width is an argument - so there is ONE kernel in the code
// object, k_fs_absorb, compiled with ntt.hip and not with the per-field sources.
//
// The kernel sits between two rounds of a sumcheck, alone on the device: it is written for latency.  ONE wave; GPU lane
// i = x + 5 y < 25 holds the 64-bit Keccak lane A[x, y] in a register pair, and a round of Keccak-f[1600] is nine cross-lane
// reads of 64 bits (__shfl: two ds_bpermute_b32 each, no LDS allocation, no barrier) in four dependent stages:
//   theta  C[x] = xor of the column: the lanes i + 5, i + 10, i + 15, i + 20 (mod 25) are the other four rows of column x, so four
//          independent reads leave C[x] in all five lanes of the column; D[x] = C[x - 1] ^ rotl(C[x + 1], 1): two reads inside the row;
//   rho    a rotation by the lane's own offset (a per-lane constant, one table load before the first round);
//   pi     B[y, 2 x + 3 y] = A[x, y] as a gather: lane (x', y') reads lane ((x' + 3 y') mod 5, x'): one read;
//   chi    A[x] = B[x] ^ (~B[x + 1] & B[x + 2]): two reads inside the row;
//   iota   lane 0 xors the round constant (wave-uniform table, indexed by the round).
// The source lanes are per-lane constants computed once.  Lanes 25 .. 63 mirror lane 0 and store nothing.
//
// ABSORB  The message is (1 + count) x 32 bytes: L = 4 (1 + count) lanes of 64 bits, so the padding never splits a lane: 0x06 is
//   the low byte of lane L and 0x80 the top byte of the last lane of the last block.  blocks = L / 17 + 1 blocks of 17 lanes
//   (136 bytes, the rate); L a multiple of 17 (count == 16) makes the padding a block of its own.  GPU lane i < 17 loads message
//   lane 17 b + i of block b - 8 aligned bytes of the state or of a word - and the next block's load is issued ahead of the
//   permutation that absorbs this one.  Every load of the state comes before the stores: one wave, program order.
// OUTPUT  lanes 0 .. 3 hold the digest: they store it to the state and, the top lane masked to keep_bits - 192 bits, to r.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace blz {

constexpr uint32_t FS_MAX_WORDS = 32;   // words absorbed behind the state by one call
constexpr int FS_RATE_LANES = 17;       // SHA3-256: 1088 bits

__device__ const uint64_t FS_ROUND_CONSTANTS[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
// rho's offsets at x + 5 y
__device__ const uint32_t FS_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// state: 4 x 64 bits, read, then written; words: count x 32 bytes (not looked at when count == 0); r: 4 x 64 bits or nullptr;
// keep_bits in (192, 256]: the challenge keeps bits [0, keep_bits) of the digest.  One block of one wave.
__global__ __launch_bounds__(64) void k_fs_absorb(uint64_t* state, const uint64_t* words, uint32_t count, uint64_t* r, uint32_t keep_bits) {
    const int lane = threadIdx.x < 25 ? (int)threadIdx.x : 0;
    const int x = lane % 5, y = lane / 5;
    const int col1 = (lane + 5) % 25, col2 = (lane + 10) % 25, col3 = (lane + 15) % 25, col4 = (lane + 20) % 25;
    const int left = (x + 4) % 5 + 5 * y, right = (x + 1) % 5 + 5 * y, right2 = (x + 2) % 5 + 5 * y;
    const int pi_src = (x + 3 * y) % 5 + 5 * x;
    const uint32_t rot = FS_RHO[lane];
    const uint32_t msg_lanes = 4u * (1u + count);
    const uint32_t blocks = msg_lanes / FS_RATE_LANES + 1;
    // message lane g of the padded message, for the GPU lanes below the rate
    auto message = [&](uint32_t block) -> uint64_t {
        if (lane >= FS_RATE_LANES) return 0;
        const uint32_t g = block * FS_RATE_LANES + (uint32_t)lane;
        uint64_t v = 0;
        if (g < 4) v = state[g];
        else if (g < msg_lanes) v = words[g - 4];
        if (g == msg_lanes) v = 0x06;
        if (block == blocks - 1 && lane == FS_RATE_LANES - 1) v ^= 0x8000000000000000ull;
        return v;
    };
    uint64_t a = 0, next = message(0);
#pragma unroll 1
    for (uint32_t b = 0; b < blocks; ++b) {
        a ^= next;
        if (b + 1 < blocks) next = message(b + 1);
#pragma unroll 1
        for (int round = 0; round < 24; ++round) {
            const uint64_t c = a ^ __shfl(a, col1) ^ __shfl(a, col2) ^ __shfl(a, col3) ^ __shfl(a, col4);
            const uint64_t cr = __shfl(c, right);
            a ^= __shfl(c, left) ^ (cr << 1 | cr >> 63);
            a = a << rot | a >> ((64 - rot) & 63);
            a = __shfl(a, pi_src);
            a ^= ~__shfl(a, right) & __shfl(a, right2);
            if (lane == 0) a ^= FS_ROUND_CONSTANTS[round];
        }
    }
    if (threadIdx.x < 4) {
        state[threadIdx.x] = a;
        if (r) r[threadIdx.x] = threadIdx.x == 3 ? a & (~0ull >> (256 - keep_bits)) : a;
    }
}

// enqueue one transcript step; the caller has checked every pointer
inline int ntt_fs_absorb(hipStream_t st, void* d_state, const void* d_words, uint32_t count, void* d_r, uint32_t keep_bits) {
    hipLaunchKernelGGL(k_fs_absorb, dim3(1), dim3(64), 0, st, (uint64_t*)d_state, (const uint64_t*)d_words, count, (uint64_t*)d_r, keep_bits);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
