// The small rounds of a GKR grand product (blz_ntt_gkr_prove) in ONE block: k_gkr_tail keeps a layer's two tables and its weight
// in LDS and runs fold, round, Keccak and the next fold without leaving the CU.  A product tree over 2^m leaves is proven by m
// layers and m (m - 1) / 2 sumcheck rounds, and all but a handful of them run over tables of a few hundred words: as a chain of
// launches such a round costs its launches and the one-wave transcript kernel, not its arithmetic.  Templated on the scalar field
// like the other ops whose wire format and 8 x 32-bit arithmetic (field.hip.hpp, vec_canon) it shares.
//
// LAYERS  Layer j, 0 <= j < m, has the tables lo and hi, the halves of layer m - 1 - j of the tree (of the leaves for j = m - 1),
//   2^j words each; its weight is W = eq(tau_0 .. tau_{j-2}) over row j - 1 of the points, 2^(j-1) words; its sumcheck is
//   blz_ntt_zerocheck_gate's chain over the gate lo hi at 3 points (include/blaze_hip.h, THE ONE-CALL GKR PROVER).
//
// ONE BODY, TWO JOBS
//   the tail of a large layer (tail != 0, 2^j > GKR_TAIL_LEN)  The chain of step launches has brought the live length down to
//     GKR_TAIL_LEN = 512 and has written, but not absorbed, the current round's row.  The block loads the 512 live words of lo and
//     hi and the 256 of W, and loops: absorb the row -> the challenge into its word of the points; fold both tables, sum the
//     weight and - while a pair is left - make the next row.  Then the claims lo[0], hi[0] and the transcript step over them.
//   whole small layers (2^j <= GKR_TAIL_LEN)  W is built in LDS from the point row by doubling (k_mle_eq's top level: seeded with
//     the integer 1, one product per pair), lo and hi are loaded AS STORED, round 0 is made, then the same loop.  The launch goes
//     on to the next layer while it fits: a tree with m <= 10 is one launch.
//   Nothing is written to the tree, the leaves or the weight: the folded words live in LDS and only lo[0] and hi[0] leave, into
//   the claims.
//
// LANES  256, and a round is cut into two stages so that no lane runs more than two field products one behind the other - in a
//   block that is alone on its CU a product's latency, about a microsecond, is what a round costs:
//   bind    an item is one folded word: word p of lo or of hi, p < live / 2, x[p] <- x[p] + r (x[p + live / 2] - x[p]) as k_mle_fold
//           makes it, `live` items over the lanes (two each at 512); no item reads what another writes, so the fold is in place.
//           The lanes from the top sum the weight, W[q] <- W[q] + W[q + live / 4]: additions only.
//   round   wave t < 3 evaluates point t: lane l takes the pairs l, l + 64, ... and adds W (lo + t dlo)(hi + t dhi), two products a
//           pair; the wave's sum is reduced by __shfl_down (six steps of eight words, no LDS) and its lane 0 holds u(t) whole: it
//           reduces it, stores it to d_rounds and hands it to wave 0 through LDS.  No sum crosses a wave.
//   Three barriers a round: behind the challenge, behind the bind, behind the row.
//
// TRANSCRIPT  The same function as blz_ntt_fs_challenge: SHA3-256 of state || words, the challenge masked at keep_bits.  Wave 0
//   runs Keccak-f[1600] in that kernel's lane layout (GPU lane x + 5 y holds A[x, y]; nine cross-lane reads a round) while the
//   other waves wait at the barrier.  The message never touches memory: lanes 0 .. 3 keep the state - it is the digest they
//   hold - in registers across the launch, lane i < 3 holds word i of the row (or claim i) in registers too, and message lane
//   g >= 4 takes its 64 bits from lane g / 4 - 1 by four cross-lane reads.  A row is 1 + 3 words = 16 message lanes and the claims
//   1 + 2 = 12: below the rate of 17, always one permutation.  d_state is read once at the start and stored once at the end.
//
// WHAT IS STORED IS CANONICAL  A row word, a folded word and a summed weight go through fp_reduce, and a field element has one
//   canonical word: the rows feed SHA3 as stored, so this is what makes this kernel and the chain of launches agree byte for
//   byte.  The claims of layer 0 are the root's own pair, copied as stored.
//
// MONTGOMERY POWERS  The tables are plain words, so mont(lo_t, hi_t) carries 1 / R and a plain weight would add another: the step
//   kernels close their sums with two products by R^2.  Here the weight is KEPT as W R^2 - the doubling is seeded with R^2 instead
//   of 1, a tail converts the 256 words it loads once - and mont(mont(lo_t, hi_t), W R^2) = lo_t hi_t W is plain as it stands:
//   the form survives the weight's sums, and no product stands between the wave's sum and the transcript.
//
// WHY EVERY INTERMEDIATE FITS  (lazy fields keep [0, 2m], the strict field [0, m); field.hip.hpp)
//   a table word goes through vec_canon before the first subtraction: [0, m).  bind: hi - lo in [0, 2m], times r R (< 2m) is
//   below 2m, plus lo: fp_add's range; fp_reduce -> [0, m).  points: lo + t d by fp_add, in range for any t.  A term is
//   mont(mont(lo_t, hi_t), W R^2) with the weight in [0, m): every product has both operands <= 2m.  A sum of n <= 4 + 6 terms in
//   a lane and across a wave by fp_add stays in fp_add's range whatever n; fp_reduce makes the row word canonical.
//   The weight by doubling: up = mont(old, tau R) < 2m, old - up by fp_sub: [0, 2m]; reduced once at the end, and at every sum.
//
// HOUSE RULES  No atomics, no allocation, no scratch memory, no spinning on memory.  The block synchronises with __syncthreads
//   alone; every loop bound around a barrier is block-uniform (the arguments, the layer, the live length) and nothing returns, so
//   every lane reaches every barrier.  LDS: 2 x 16 KiB of tables, 8 KiB of weight, under 2 KiB for the row, the challenge, the
//   point row and its Montgomery forms: 42 KiB, static, below the 64 KiB a static allocation may have - which is why the largest
//   live length is 512 and not 1024 (80 KiB).
#pragma once
#include "ntt_zerocheck.hip.hpp"

namespace blz {

// (GKR_TAIL_LEN = 512, the largest live length the block takes, stands in ntt_engine.hpp: the entry point plans by it)
constexpr int GKR_POINTS = 3;                           // the gate lo hi has degree 2
static_assert(GKR_TAIL_LEN / 2 == (uint32_t)VEC_THREADS, "a tail loads one weight word per lane");
static_assert(VEC_THREADS / 64 >= GKR_POINTS, "one wave per point");
static_assert(NTT_MAX_LOG <= 32, "the point row in LDS holds 32 words");

// Keccak-f[1600]: the round constants and rho's offsets at x + 5 y (FIPS 202)
__device__ const uint64_t GKR_KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
__device__ const uint32_t GKR_KECCAK_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// a GPU lane's constants of the permutation: lane x + 5 y < 25 holds A[x, y]; lanes 25 .. 63 mirror lane 0
struct GkrKeccakLane {
    int lane, col1, col2, col3, col4, left, right, right2, pi_src, msg_src;
    uint32_t rot;
};
BLZ_DEV GkrKeccakLane gkr_keccak_lane() {
    GkrKeccakLane k;
    k.lane = (threadIdx.x & 63u) < 25u ? (int)(threadIdx.x & 63u) : 0;
    const int x = k.lane % 5, y = k.lane / 5;
    k.col1 = (k.lane + 5) % 25, k.col2 = (k.lane + 10) % 25, k.col3 = (k.lane + 15) % 25, k.col4 = (k.lane + 20) % 25;
    k.left = (x + 4) % 5 + 5 * y, k.right = (x + 1) % 5 + 5 * y, k.right2 = (x + 2) % 5 + 5 * y;
    k.pi_src = (x + 3 * y) % 5 + 5 * x;
    k.msg_src = k.lane >= 4 ? k.lane / 4 - 1 : 0;   // the lane that holds the word of message lane k.lane
    k.rot = GKR_KECCAK_RHO[k.lane];
    return k;
}

// One transcript step by ONE whole wave.  st: lanes 0 .. 3 hold the state; w: lane i < count holds word i as 4 x 64 bits;
// count <= 3, so the padded message is one block.  Returns the lane's 64 bits of the permuted state: lanes 0 .. 3 the digest
BLZ_DEV uint64_t gkr_absorb(const GkrKeccakLane& k, uint64_t st, const uint64_t (&w)[4], uint32_t count) {
    const int msg_lanes = 4 * (1 + (int)count);
    const uint64_t x0 = __shfl(w[0], k.msg_src), x1 = __shfl(w[1], k.msg_src), x2 = __shfl(w[2], k.msg_src), x3 = __shfl(w[3], k.msg_src);
    const int q = k.lane & 3;
    uint64_t a = q == 0 ? x0 : q == 1 ? x1 : q == 2 ? x2 : x3;
    if (k.lane < 4) a = st;
    else if (k.lane >= msg_lanes) a = 0;
    if (k.lane == msg_lanes) a = 0x06;
    if (k.lane == 16) a ^= 0x8000000000000000ull;   // the last lane of the rate
#pragma unroll 1
    for (int round = 0; round < 24; ++round) {
        const uint64_t c = a ^ __shfl(a, k.col1) ^ __shfl(a, k.col2) ^ __shfl(a, k.col3) ^ __shfl(a, k.col4);
        const uint64_t cr = __shfl(c, k.right);
        a ^= __shfl(c, k.left) ^ (cr << 1 | cr >> 63);
        a = a << k.rot | a >> ((64 - k.rot) & 63);
        a = __shfl(a, k.pi_src);
        a ^= ~__shfl(a, k.right) & __shfl(a, k.right2);
        if (k.lane == 0) a ^= GKR_KECCAK_RC[round];
    }
    return a;
}

// the challenge's 64 bits of digest lane `i` < 4
BLZ_DEV uint64_t gkr_challenge(uint64_t digest, uint32_t i, uint32_t keep_bits) { return i == 3 ? digest & (~0ull >> (256 - keep_bits)) : digest; }

template <class Fr>
BLZ_DEV void gkr_pack(uint64_t (&w)[4], const Fp<Fr>& x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint64_t)x.v[2 * i] | (uint64_t)x.v[2 * i + 1] << 32;
}

// where layer j's tables start: the halves of layer m - 1 - j of the tree, of the leaves for j = m - 1; hi = lo + 2^j words
BLZ_DEV const uint32_t* gkr_layer(const NttGkrTail& g, uint32_t j) {
    return j + 1 == g.m ? g.a : g.tree + ((1ull << g.m) - (4ull << j)) * 8;
}

// Bind the top variable of both tables in LDS, in place, and sum the weight: `live` words in each table, live / 2 come out
template <class Fr>
BLZ_DEV void gkr_bind(uint32_t* lo, uint32_t* hi, uint32_t* wt, uint32_t live, const Fp<Fr>& rm) {
    const uint32_t half = live >> 1, quarter = live >> 2;
#pragma unroll 1
    for (uint32_t item = threadIdx.x; item < live; item += VEC_THREADS) {
        uint32_t* const tb = item < half ? lo : hi;
        const uint32_t p = item < half ? item : item - half;
        Fp<Fr> x, y;
        fp_load(x, tb + p * 8);
        fp_load(y, tb + (p + half) * 8);
        vec_canon(x);
        vec_canon(y);
        fp_sub(y, y, x);
        fp_mul(y, y, rm);
        fp_add(x, x, y);
        fp_reduce(x);
        fp_store(tb + p * 8, x);
    }
    const uint32_t q = VEC_THREADS - 1 - threadIdx.x;   // from the top: the lanes the fold leaves idle below 512
    if (q < quarter) {
        Fp<Fr> w, w2;
        fp_load(w, wt + q * 8);
        fp_load(w2, wt + (q + quarter) * 8);
        fp_add(w, w, w2);
        fp_reduce(w);
        fp_store(wt + q * 8, w);
    }
}

// The round polynomial over `pairs` pairs of both tables: wave t < 3 makes u(t) = sum_p W[p] (lo + t dlo)(hi + t dhi), canonical,
// into word t of `out` (d_rounds) and of `row` (LDS).  wt holds W R^2.  Every lane calls it
template <class Fr>
BLZ_DEV void gkr_round(const uint32_t* lo, const uint32_t* hi, const uint32_t* wt, uint32_t pairs, uint32_t* row, uint32_t* out) {
    using E = Fp<Fr>;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (wave < (uint32_t)GKR_POINTS) {
        E acc;
        fp_zero(acc);
#pragma unroll 1
        for (uint32_t p = lane; p < pairs; p += 64) {
            E a, b, d, w;
            fp_load(a, lo + p * 8);
            fp_load(d, lo + (p + pairs) * 8);
            vec_canon(a);
            vec_canon(d);
            fp_sub(d, d, a);
            if (wave >= 1) fp_add(a, a, d);
            if (wave >= 2) fp_add(a, a, d);
            fp_load(b, hi + p * 8);
            fp_load(d, hi + (p + pairs) * 8);
            vec_canon(b);
            vec_canon(d);
            fp_sub(d, d, b);
            if (wave >= 1) fp_add(b, b, d);
            if (wave >= 2) fp_add(b, b, d);
            fp_mul(a, a, b);
            fp_load(w, wt + p * 8);
            fp_mul(a, a, w);
            fp_add(acc, acc, a);
        }
#pragma unroll 1
        for (int off = 32; off >= 1; off >>= 1) {
            E o;
#pragma unroll
            for (int k = 0; k < Fr::N; ++k) o.v[k] = __shfl_down(acc.v[k], (unsigned)off);
            fp_add(acc, acc, o);
        }
        if (lane == 0) {
            fp_reduce(acc);
            fp_store(row + wave * 8, acc);
            fp_store(out + wave * 8, acc);
        }
    }
}

// g: NttGkrTail (ntt_engine.hpp).  One block of VEC_THREADS lanes
template <class Fr>
__global__ __launch_bounds__(VEC_THREADS) void k_gkr_tail(NttGkrTail g) {
    using E = Fp<Fr>;
    __shared__ __attribute__((aligned(16))) uint32_t lo[GKR_TAIL_LEN * 8];
    __shared__ __attribute__((aligned(16))) uint32_t hi[GKR_TAIL_LEN * 8];
    __shared__ __attribute__((aligned(16))) uint32_t wt[GKR_TAIL_LEN / 2 * 8];
    __shared__ __attribute__((aligned(16))) uint32_t row[GKR_POINTS * 8];      // the round polynomial, from the waves that made it to wave 0
    __shared__ __attribute__((aligned(16))) uint32_t chal[8];                 // the round's challenge, for every lane
    __shared__ __attribute__((aligned(16))) uint32_t pt[32 * 8];               // the point row: read for W, then rewritten by the layer
    __shared__ __attribute__((aligned(16))) uint32_t tm[GKR_TAIL_LOG * 8];     // tau R of the weight's variables
    const uint32_t t = threadIdx.x;
    const bool wave0 = t < 64;
    const GkrKeccakLane kl = gkr_keccak_lane();
    uint64_t st = 0;
    if (t < 4) st = reinterpret_cast<const uint64_t*>(g.state)[t];
    // a launch that starts with a whole layer below the root takes that layer's point from memory; later layers find it in pt
    if (!g.tail && t < g.first) {
        const uint32_t* const row = g.points + ((size_t)(g.first - 1) * g.first / 2 + t) * 8;
        reinterpret_cast<uint4*>(pt + t * 8)[0] = reinterpret_cast<const uint4*>(row)[0];
        reinterpret_cast<uint4*>(pt + t * 8)[1] = reinterpret_cast<const uint4*>(row)[1];
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = g.first; j < g.last; ++j) {
        const uint32_t* const gl = gkr_layer(g, j);
        const uint32_t* const gh = gl + ((size_t)8 << j);
        uint32_t* const rows = g.rounds + (size_t)GKR_POINTS * (j * (j - 1u) / 2) * 8;             // layer j's rounds
        uint64_t* const prow = reinterpret_cast<uint64_t*>(g.points) + (size_t)(j * (j + 1u) / 2) * 4;   // row j of the points
        uint64_t* const pt64 = reinterpret_cast<uint64_t*>(pt);
        uint32_t live, i;
        bool made_here;   // the current row is in `row`; else the chain's last step left it in d_rounds
        if (g.tail) {
            live = GKR_TAIL_LEN, i = j - GKR_TAIL_LOG, made_here = false;
#pragma unroll
            for (uint32_t p = t; p < GKR_TAIL_LEN; p += VEC_THREADS) {
                E x, y;
                fp_load(x, gl + (size_t)p * 8);
                fp_load(y, gh + (size_t)p * 8);
                fp_store(lo + p * 8, x);
                fp_store(hi + p * 8, y);
            }
            E w;   // the weight as the steps left it, plain: W R^2 from here on
            fp_load(w, g.weight + (size_t)t * 8);
            fp_to_mont(w, w);
            fp_to_mont(w, w);
            fp_reduce(w);
            fp_store(wt + t * 8, w);
            __syncthreads();
        } else {
            live = 1u << j, i = 0, made_here = true;
#pragma unroll 1
            for (uint32_t p = t; p < live; p += VEC_THREADS) {
                E x, y;
                fp_load(x, gl + (size_t)p * 8);
                fp_load(y, gh + (size_t)p * 8);
                fp_store(lo + p * 8, x);
                fp_store(hi + p * 8, y);
            }
            if (j >= 1) {
                // W R^2 = eq(tau_0 .. tau_{j-2}) R^2 by doubling: k_mle_eq's top level, seeded with R^2 where that seeds with 1
                const uint32_t nv = j - 1;
                if (t < nv) {
                    E w;
                    fp_load(w, pt + t * 8);
                    fp_to_mont(w, w);
                    fp_store(tm + t * 8, w);
                }
                if (t == 0) {
                    E seed;
#pragma unroll
                    for (int k = 0; k < Fr::N; ++k) seed.v[k] = Fr::R2[k];
                    fp_store(wt, seed);
                }
                __syncthreads();
#pragma unroll 1
                for (uint32_t s = 0; s < nv; ++s) {
                    const uint32_t size = 1u << s;
                    if (t < size) {
                        E w, old, up;
                        fp_load(w, tm + s * 8);
                        fp_load(old, wt + t * 8);
                        fp_mul(up, old, w);
                        fp_sub(old, old, up);
                        fp_store(wt + t * 8, old);
                        fp_store(wt + (t + size) * 8, up);
                    }
                    __syncthreads();
                }
                if (t < (1u << nv)) {
                    E w;
                    fp_load(w, wt + t * 8);
                    fp_reduce(w);
                    fp_store(wt + t * 8, w);
                }
                __syncthreads();
                // round 0 over the pairs of the tables as stored
                gkr_round<Fr>(lo, hi, wt, live >> 1, row, rows);
            }
            __syncthreads();
        }
        // one pass per variable: absorb the row, bind the top variable, make the next row while a pair is left
#pragma unroll 1
        while (j >= 1 && live >= 2) {
            if (wave0) {
                E u;
                fp_zero(u);
                if (t < (uint32_t)GKR_POINTS) fp_load(u, made_here ? row + t * 8 : rows + ((size_t)i * GKR_POINTS + t) * 8);
                uint64_t w4[4];
                gkr_pack<Fr>(w4, u);
                st = gkr_absorb(kl, st, w4, GKR_POINTS);
                if (t < 4) {
                    const uint64_t c = gkr_challenge(st, t, g.keep_bits);
                    prow[(size_t)(j - 1 - i) * 4 + t] = c;   // backwards: the row ends up in bit order
                    pt64[(j - 1 - i) * 4 + t] = c;
                    reinterpret_cast<uint64_t*>(chal)[t] = c;
                }
            }
            __syncthreads();
            E rm;
            fp_load(rm, chal);
            fp_to_mont(rm, rm);
            gkr_bind<Fr>(lo, hi, wt, live, rm);
            live >>= 1, ++i, made_here = true;
            __syncthreads();
            if (live >= 2) {
                gkr_round<Fr>(lo, hi, wt, live >> 1, row, rows + (size_t)i * GKR_POINTS * 8);
                __syncthreads();
            }
        }
        // the claims lo[0], hi[0] - the tables at the challenges; layer 0: the root's own pair as stored - and their transcript step
        if (wave0) {
            E cw;
            fp_zero(cw);
            if (t < 2) {
                fp_load(cw, t == 0 ? lo : hi);
                fp_store(g.claims + ((size_t)2 * j + t) * 8, cw);
            }
            uint64_t w4[4];
            gkr_pack<Fr>(w4, cw);
            st = gkr_absorb(kl, st, w4, 2);
            if (t < 4) {
                const uint64_t c = gkr_challenge(st, t, g.keep_bits);
                prow[(size_t)j * 4 + t] = c;
                pt64[j * 4 + t] = c;
            }
        }
        __syncthreads();
    }
    if (t < 4) reinterpret_cast<uint64_t*>(g.state)[t] = st;
}

// The claims of layer g.first alone, for the chain of launches: word 0 of lo and of hi into row g.first of the claims
template <class Fr>
__global__ __launch_bounds__(64) void k_gkr_claims(NttGkrTail g) {
    const uint32_t* const gl = gkr_layer(g, g.first);
    const uint32_t* const src = threadIdx.x < 2 ? gl : gl + ((size_t)8 << g.first);
    if (threadIdx.x < 4)
        reinterpret_cast<uint4*>(g.claims + (size_t)2 * g.first * 8)[threadIdx.x] = reinterpret_cast<const uint4*>(src)[threadIdx.x & 1u];
}

// g.claims_only: k_gkr_claims for layer g.first; else k_gkr_tail over the layers [g.first, g.last).  The caller has checked every
// pointer and that the layers fit: tail != 0 takes ONE layer with 2^first > GKR_TAIL_LEN, else 2^(last - 1) <= GKR_TAIL_LEN
template <class Fr>
int ntt_gkr_tail_t(hipStream_t st, const NttGkrTail& g) {
    if (g.claims_only) hipLaunchKernelGGL(k_gkr_claims<Fr>, dim3(1), dim3(64), 0, st, g);
    else hipLaunchKernelGGL(k_gkr_tail<Fr>, dim3(1), dim3(VEC_THREADS), 0, st, g);
    BLZ_HIP(hipGetLastError(), BLZ_ERR_UNKNOWN);
    return BLZ_OK;
}

}  // namespace blz
