// What batched-affine bucket accumulation would have to move, measured: Montgomery's trick
// trades ~3.5 field products per addition for memory traffic - every addition reads its two operands twice
// (forward pass: denominators and running products; backward pass: slopes and sums) and parks a running product and a
// result in memory in between.  This tool times the bare memory side on the 2^26 working set:
//   A  805 M random 128-byte line gathers out of an 8 GiB table (what k_accumulate does once per MSM)
//   B  the same gathers done twice (operands of a level re-read on the way back), plus the 56-byte running product
//      written and read back and the 112-byte affine result written, per addition
// No arithmetic at all: these are floors for the memory side, to be set against the multiply-adds saved.
//   C  pattern A's gathers fetched as whole lines: eight consecutive lanes fetch one point's 128-byte line, 16 B each,
//      straight into LDS (global_load_lds_dwordx4, eight per wave-gather), and every lane reads its own 112 bytes back
//      with ds_read_b128.  64 line and page look-ups per wave-gather instead of A's 448.  C' is C with the pieces of a
//      line rotated by the instruction number, so that the eight lanes of a group read eight different LDS banks.
//      `gather_bw 26 1 lines` times A, C and C' alone and beside a streaming copy (min / median / max of 5 runs),
//      each as compiled and with 200 VGPRs claimed, which is the accumulation kernel's two waves per SIMD.
// Build: hipcc --offload-arch=gfx950 -O3 tools/gather_bw.hip -o build/gather_bw
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

__global__ __launch_bounds__(256) void k_fill_idx(uint32_t* idx, uint64_t n, uint32_t mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint64_t z = (i + 0x9e3779b97f4a7c15ull) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        idx[i] = (uint32_t)(z ^ (z >> 31)) & mask;
    }
}

// one lane per run of `len` entries (a bucket's run), 2 gathers in flight per lane (the next point prefetched),
// exactly the access pattern of the accumulation kernel; MODE 1 adds the batched-affine side traffic
// NV = 200 claims 200 VGPRs, which gives the accumulation kernel's two waves per SIMD
template <int MODE, int NV = 0>
__global__ __launch_bounds__(128) void k_gather(const uint4* __restrict__ pts, const uint32_t* __restrict__ idx, uint64_t nruns,
                                                uint32_t len, uint4* __restrict__ side, uint4* __restrict__ sink) {
    if (NV == 200) asm volatile("v_mov_b32 v199, 0" ::: "v199");
    uint64_t t = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    if (t >= nruns) return;
    const uint32_t* e = idx + t * len;
    uint4 acc = make_uint4(0, 0, 0, 0);
    const int passes = MODE ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        uint4 nx[7];
        {
            const uint4* p = pts + (uint64_t)e[0] * 8;
#pragma unroll
            for (int k = 0; k < 7; ++k) nx[k] = p[k];
        }
        for (uint32_t j = 0; j < len; ++j) {
            uint4 cur[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) cur[k] = nx[k];
            if (j + 1 < len) {
                const uint4* p = pts + (uint64_t)e[j + 1] * 8;
#pragma unroll
                for (int k = 0; k < 7; ++k) nx[k] = p[k];
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) { acc.x ^= cur[k].x; acc.y += cur[k].y; acc.z ^= cur[k].z; acc.w += cur[k].w; }
            if (MODE) {
                // per addition (= per pair of points, so every other entry): 56 B running product out (pass 0) and
                // back in (pass 1), 112 B result out (pass 1)
                if (j & 1) {
                    uint4* s = side + (t * (len / 2) + j / 2) * 11;   // 3.5 + 7 sixteen-byte pieces, rounded to 11
                    if (pass == 0) { s[0] = acc; s[1] = acc; s[2] = acc; s[3] = acc; }
                    else {
                        acc.x ^= s[0].x ^ s[1].y ^ s[2].z ^ s[3].w;
#pragma unroll
                        for (int k = 4; k < 11; ++k) s[k] = acc;
                    }
                }
            }
        }
    }
    if (acc.x == 0x12345678u && acc.y == 0x9abcdef0u) sink[0] = acc;
}

// pattern C: the same runs, the same two gathers in flight per lane, but the prefetched point lands in LDS as whole
// lines.  Instruction k of a wave-gather fetches the lines owned by lanes 8g + k (g = 0..7): lane (g, r) fetches piece
// r (SWZ: piece (r + k) & 7).  The hardware writes lane l's 16 bytes at base + 16 l, so the image of instruction k is
// [g][r] and lane 8g + k finds its point at piece k * 64 + g * 8.  Every lane takes part in every load: lanes past
// the last run fetch line 0.
template <int SWZ, int NV>
__global__ __launch_bounds__(128) void k_gather_lines(const uint4* __restrict__ pts, const uint32_t* __restrict__ idx, uint64_t nruns,
                                                      uint32_t len, uint4* __restrict__ sink) {
    if (NV == 200) asm volatile("v_mov_b32 v199, 0" ::: "v199");
    __shared__ uint4 img[2][512];   // 8 KiB per wave
    const uint32_t lane = threadIdx.x & 63, r = lane & 7, g0 = lane & ~7u;
    uint4* my = img[threadIdx.x >> 6];
    const uint64_t t = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    const bool live = t < nruns;
    const uint32_t* e = idx + (live ? t : 0) * len;
    auto issue = [&](uint32_t own) {
        uint32_t o[8];   // the owners' entry indices, passed around the group
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = __shfl(own, g0 + k);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4* src = pts + (uint64_t)o[k] * 8 + (SWZ ? ((r + k) & 7) : r);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(my + k * 64), 16, 0, 0);
        }
    };
    const uint32_t home = r * 64 + (lane >> 3) * 8;   // this lane's own line in the image
    uint4 acc = make_uint4(0, 0, 0, 0);
    issue(live ? e[0] : 0);
    uint32_t nidx = live && len > 1 ? e[1] : 0;
    for (uint32_t j = 0; j < len; ++j) {
        uint4 cur[7];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's own loads have landed: nothing else orders the reads
#pragma unroll
        for (int k = 0; k < 7; ++k) cur[k] = my[home + (SWZ ? ((k - r) & 7) : k)];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are read out before the next gather overwrites them
        if (j + 1 < len) {
            issue(nidx);
            nidx = live && j + 2 < len ? e[j + 2] : 0;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) { acc.x ^= cur[k].x; acc.y += cur[k].y; acc.z ^= cur[k].z; acc.w += cur[k].w; }
    }
    if (acc.x == 0x12345678u && acc.y == 0x9abcdef0u) sink[0] = acc;
}

// (the streaming copy of tools/coresident.hip)
__global__ __launch_bounds__(256) void k_copy(const uint4* __restrict__ in, uint4* __restrict__ out, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) out[i] = in[i];
}

// A, C and C' alone and beside a streaming copy on a second stream that lasts at least as long as the gather
static int run_lines(const uint4* pts, const uint32_t* idx, uint64_t nruns, uint32_t len, uint4* sink) {
    const size_t cbytes = (size_t)1 << 30;
    uint4 *cin, *cout;
    if (hipMalloc(&cin, cbytes) != hipSuccess || hipMalloc(&cout, cbytes) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    hipStream_t sa, sb;
    hipEvent_t e0, e1, f0, f1;
    if (hipMemset(cin, 1, cbytes) != hipSuccess || hipStreamCreateWithFlags(&sa, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&sb, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess || hipEventCreate(&f0) != hipSuccess || hipEventCreate(&f1) != hipSuccess) {
        printf("stream / event setup failed\n");
        return 1;
    }
    const dim3 grid((unsigned)((nruns + 127) / 128));
    auto launch = [&](int pat, int occ) {
        if (pat == 0) {
            if (occ) hipLaunchKernelGGL((k_gather<0, 200>), grid, dim3(128), 0, sa, pts, idx, nruns, len, (uint4*)nullptr, sink);
            else hipLaunchKernelGGL((k_gather<0, 0>), grid, dim3(128), 0, sa, pts, idx, nruns, len, (uint4*)nullptr, sink);
        } else if (pat == 1) {
            if (occ) hipLaunchKernelGGL((k_gather_lines<0, 200>), grid, dim3(128), 0, sa, pts, idx, nruns, len, sink);
            else hipLaunchKernelGGL((k_gather_lines<0, 0>), grid, dim3(128), 0, sa, pts, idx, nruns, len, sink);
        } else {
            if (occ) hipLaunchKernelGGL((k_gather_lines<1, 200>), grid, dim3(128), 0, sa, pts, idx, nruns, len, sink);
            else hipLaunchKernelGGL((k_gather_lines<1, 0>), grid, dim3(128), 0, sa, pts, idx, nruns, len, sink);
        }
    };
    float tc = 0;
    for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(f0, sb);
        hipLaunchKernelGGL(k_copy, dim3(4096), dim3(256), 0, sb, cin, cout, cbytes / 16);
        hipEventRecord(f1, sb); hipStreamSynchronize(sb); hipEventElapsedTime(&tc, f0, f1);
    }
    printf("copy alone: %.3f ms per GiB -> %.0f GB/s (r+w)\n", tc, 2.0 * cbytes / tc / 1e6);
    const char* name[3] = {"A  per-lane, 7 x global_load_dwordx4", "C  whole lines through LDS", "C' whole lines through LDS, pieces rotated"};
    const int reps = 5;
    for (int occ = 0; occ < 2; ++occ)
    for (int beside = 0; beside < 2; ++beside)
        for (int pat = 0; pat < 3; ++pat) {
            float ms[reps], alone = 0, cms = 0;
            for (int rep = 0; rep < reps; ++rep) {
                int ncopy = 0;
                if (beside) {
                    if (rep == 0) { hipEventRecord(e0, sa); launch(pat, occ); hipEventRecord(e1, sa); hipStreamSynchronize(sa); hipEventElapsedTime(&alone, e0, e1); }
                    ncopy = (int)(1.5f * alone / tc) + 2;
                    hipEventRecord(f0, sb);
                    for (int i = 0; i < ncopy; ++i) hipLaunchKernelGGL(k_copy, dim3(4096), dim3(256), 0, sb, cin, cout, cbytes / 16);
                    hipEventRecord(f1, sb);
                }
                hipEventRecord(e0, sa); launch(pat, occ); hipEventRecord(e1, sa);
                if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { printf("launch or kernel failed\n"); return 1; }
                hipEventElapsedTime(&ms[rep], e0, e1);
                if (beside) { hipEventElapsedTime(&cms, f0, f1); cms /= ncopy; }
            }
            std::sort(ms, ms + reps);
            printf("%s %-46s %s: min %.2f  median %.2f  max %.2f ms", occ ? "200 VGPRs (2 waves/SIMD)" : "VGPRs as compiled       ", name[pat], beside ? "beside the copy" : "alone          ", ms[0], ms[reps / 2], ms[reps - 1]);
            if (beside) printf("   (copy: %.3f ms per GiB)", cms);
            printf("\n");
        }
    return 0;
}

int main(int argc, char** argv) {
    // optional argument: log2 of the table size in points (26 = the 8 GiB table of the 2^26 MSM); the entry count stays
    const int logp = argc > 1 ? atoi(argv[1]) : 26;
    const int nmodes = argc > 2 ? atoi(argv[2]) : 2;   // 1: pattern A only (big tables: B's side buffer is 97 GB)
    const uint64_t npts = 1ull << logp, entries = 12ull << 26;
    printf("table: 2^%d points x 128 B = %.2f GiB\n", logp, (double)npts * 128 / (1ull << 30));
    const uint32_t len = 44;   // mean run length of the 2^26 plan (805 M entries over ~18 M buckets)
    const uint64_t nruns = entries / len;
    uint4 *pts, *side, *sink;
    uint32_t* idx;
    hipMalloc(&pts, npts * 128);
    hipMalloc(&idx, entries * 4);
    hipMalloc(&side, nmodes > 1 ? nruns * (len / 2) * 11 * 16 : 64);
    hipMalloc(&sink, 64);
    hipMemset(pts, 1, npts * 128);
    hipLaunchKernelGGL(k_fill_idx, dim3(4096), dim3(256), 0, 0, idx, entries, (uint32_t)(npts - 1));
    hipDeviceSynchronize();
    if (argc > 3 && !strcmp(argv[3], "lines")) return run_lines(pts, idx, nruns, len, sink);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int mode = 0; mode < nmodes; ++mode) {
        float best = 1e9f;
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0);
            if (mode == 0) hipLaunchKernelGGL(k_gather<0>, dim3((unsigned)((nruns + 127) / 128)), dim3(128), 0, 0, pts, idx, nruns, len, side, sink);
            else hipLaunchKernelGGL(k_gather<1>, dim3((unsigned)((nruns + 127) / 128)), dim3(128), 0, 0, pts, idx, nruns, len, side, sink);
            hipEventRecord(e1);
            hipDeviceSynchronize();
            float ms; hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        const double gathered = (double)nruns * len * 112 * (mode ? 2 : 1);
        const double sidebytes = mode ? (double)nruns * (len / 2) * (64.0 * 2 + 112.0) : 0.0;
        printf("%s: %.2f ms for %.1f GB gathered (128-B lines, 112 B used) + %.1f GB side traffic -> %.2f TB/s of useful bytes\n",
               mode ? "B batched-affine traffic pattern (no arithmetic)" : "A one gather per entry (k_accumulate's pattern, no arithmetic)",
               best, gathered / 1e9, sidebytes / 1e9, (gathered + sidebytes) / best / 1e9);
    }
    return 0;
}
