// Microbenchmark 16 (not product code): the gate for streaming long frames
// through nt LDS-DMA. mb9 put the hash beside a DMA stream on cfg3's layout
// and lost; mb10 did it on a contiguous buffer and lost. Two causes looked
// removable: mb10 made room for its ring by cutting table replicas (bank
// conflicts) and mb9 copied dword-aligned spans, so the 128-B line two
// consecutive rounds share was fetched twice (nt lines are not kept). Here
// the real slice-by-4 CRC runs beside the DMA with both removed:
//   * compact tables that stay conflict-free by rotating the lookup order by
//     lane (XOR commutes): 16 replicas, 256-B rows T3|T2|T1|T0, lanes with
//     bit 4 set look up slots 1,0,3,2 (64 KiB); or 8 replicas, 128-B rows,
//     four quarter-rotations (32 KiB, one shift more per lookup);
//   * a unit grid anchored at floor128(frame end), so every round after
//     round 0 is four whole lines of its frame, requested by exactly one DMA
//     instruction (one instruction = two frames' 512-B rounds). Round 0 (the
//     frame's front, unit 0 from inside the frame's first line) and the
//     <= 124 bytes past the grid are read by ordinary loads; the tail is fed
//     after the merge by word steps of lane G - 1.
// cfg3's layout: 1,048,576 frames of 16,400 B at a 16,404-B stride (17.2 GB),
// G = 8, 16 waves per CU, one workgroup per CU. Arms:
//   plain     the product's k_frames<8, 1> (128 KiB tables, dwordx4 unit
//             loads, one round prefetched), static deal
//   ring-64K  4 KiB nt-DMA batch per wave (8 frames x 4 lines), read back by
//             ds_read_b128, the next batch re-issued into the same slots,
//             then hashed with the two-way-rotated 64 KiB tables
//   ring-32K  the same with the four-way-rotated 32 KiB tables
//   ring-xor  the same stream, XOR instead of table work (its stream roof)
// Every hashing arm writes one CRC per frame; the ring arms' must equal the
// plain arm's word for word, and three frames are checked against a bitwise
// host CRC. Arms alternate kReps times; the gate compares the best ring arm's
// median with plain's and with the spread of plain's own repeats.
//   mb16        timing
//   mb16 pmc    two launches of plain, ring-64K and ring-32K only (counter passes)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crc_kernels.hpp"

using namespace vcrc;

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__);           \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define LDSP(x) ((__attribute__((address_space(3))) void *)(x))

constexpr int kG = 8;
constexpr uint32_t kRing = 65536;        // ring: 16 waves x 4 KiB above the compact tables
constexpr uint32_t kRound = kG * kUnit;  // 512 B of a frame per round

__global__ void k_fill(u32x4 *p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t z = i * 0x9E3779B97F4A7C15ull;
        z ^= z >> 29;
        p[i] = u32x4{(uint32_t)z, (uint32_t)(z >> 32), (uint32_t)(z * 3), (uint32_t)i};
    }
}

// LDS reads of the ring arms go through asm: hipcc cannot tell the tables from
// the ring (one array) and would wait vmcnt(0) for the batch in flight before
// every table lookup. Each statement holds its reads and their wait.
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ uint32_t lds_xor4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3)
{
    uint32_t r0, r1, r2, r3;
    asm("ds_read_b32 %0, %4 offset:%8\n\tds_read_b32 %1, %5 offset:%9\n\t"
        "ds_read_b32 %2, %6 offset:%10\n\tds_read_b32 %3, %7 offset:%11\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "i"(O0), "i"(O1), "i"(O2), "i"(O3));
    return r0 ^ r1 ^ r2 ^ r3;
}
__device__ __forceinline__ uint32_t map_apply_asm(uint32_t a, uint32_t map)
{
    uint32_t ad[8], r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) ad[k] = map + ((a >> (4 * k)) & 15u) * 4u;
    asm("ds_read_b32 %0, %8\n\tds_read_b32 %1, %9 offset:64\n\tds_read_b32 %2, %10 offset:128\n\t"
        "ds_read_b32 %3, %11 offset:192\n\tds_read_b32 %4, %12 offset:256\n\tds_read_b32 %5, %13 offset:320\n\t"
        "ds_read_b32 %6, %14 offset:384\n\tds_read_b32 %7, %15 offset:448\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7])
        : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7]));
    return r[0] ^ r[1] ^ r[2] ^ r[3] ^ r[4] ^ r[5] ^ r[6] ^ r[7];
}

// TAB 64: 256-B row per byte value, slot s (64 B, 16 replicas) = T_{3-s}, which
// consumes byte s of the word. Lanes with bit 4 clear read slots 0,1,2,3, the
// others 1,0,3,2: in every ds_read_b32 one half of a half-wave is in banks
// 0-15 and the other in banks 16-31. Slots 2 and 3 through the offset field.
// TAB 32: 128-B rows, slot = 32 B (8 replicas); lane class c = (lane >> 3) & 3
// reads slot (i + c) & 3 in instruction i: four classes, four bank octets.
// TAB 0: XOR only.
template <int TAB>
struct Tab {
    uint32_t base[4], sel[4];
    __device__ Tab(int lane)
    {
        if (TAB == 64) {
            const uint32_t lo = (uint32_t)(lane & 15) << 2, c = (uint32_t)(lane >> 4) & 1u;
            const uint32_t k[4] = {c, 1u - c, 2u + c, 3u - c};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                base[i] = (k[i] & 1u) * 64u + lo;
                sel[i] = 0x0C020400u + (k[i] << 8);
            }
        } else {
            const uint32_t rep = (uint32_t)(lane & 7), c = (uint32_t)(lane >> 3) & 3u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t s = ((uint32_t)i + c) & 3u;
                base[i] = s * 64u + rep * 8u;  // twice the byte offset in the row: the address is shifted right once
                sel[i] = 0x0C020400u + (s << 8);
            }
        }
    }
    __device__ __forceinline__ uint32_t step(uint32_t c, uint32_t w) const
    {
        const uint32_t y = c ^ w;
        if (TAB == 0) return y;
        uint32_t a[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            a[i] = __builtin_amdgcn_perm(y, base[i], sel[i]);
            if (TAB == 32) a[i] >>= 1;
        }
        return TAB == 64 ? lds_xor4<0, 0, 128, 128>(a[0], a[1], a[2], a[3]) : lds_xor4<0, 0, 0, 0>(a[0], a[1], a[2], a[3]);
    }
    __device__ __forceinline__ uint32_t advance(uint32_t a, uint32_t map) const { return TAB == 0 ? a : map_apply_asm(a, map); }
};

template <int TAB>
__device__ void build_compact(const uint32_t *consts)
{
    const uint32_t t = threadIdx.x;
    if (TAB == 64) {
        for (uint32_t wi = t; wi < 16384u; wi += kBlock) s_lds[wi] = consts[kConstSlice + (3u - ((wi >> 4) & 3u)) * 256u + (wi >> 6)];
    } else if (TAB == 32) {
        for (uint32_t wi = t; wi < 8192u; wi += kBlock) s_lds[wi] = consts[kConstSlice + (3u - ((wi >> 3) & 3u)) * 256u + (wi >> 5)];
    }
    for (uint32_t i = t; i < kNumMaps * 128u; i += kBlock) s_lds[kLdsMaps / 4u + i] = consts[kConstGap + i];
    __syncthreads();
}

// One frame group (8 frames) of a wave. Hash lane = (frame lane / 8, unit g).
// Batch image in the wave's 4 KiB slot: unit m = hash lane m at 64 m, its 16-B
// piece k at position (k + (m >> 2)) & 3, so each ds_read_b128 of the read-back
// has its 16 lanes of a pass in 16 different bank quads. DMA instruction q,
// lane l writes slot + 1024 q + 16 l: unit m = 16 q + (l >> 2), i.e. frame
// 2 q + (l >> 5), unit (l >> 2) & 7, piece ((l & 3) - (l >> 4)) & 3.
template <int TAB>
__device__ __forceinline__ void ring_group(const FrameParams &p, uint64_t fb, int lane, uint32_t slot, const uint32_t (&rd)[4],
                                           const Tab<TAB> &tb)
{
    const int g = lane & (kG - 1);
    const uint64_t f = fb + (uint64_t)(lane >> 3);
    const bool active = f < p.n;
    uint64_t off = 0;
    uint32_t L = 0;
    if (active) frame_desc(p, f, off, L);
    gu8 *const fp = gptr(p.base) + off;
    // grid: ends at floor128(frame end); T bytes (whole words here) lie past it
    const uint32_t T = min((uint32_t)((uintptr_t)(fp + L) & 127u), L);
    const uint32_t Lg = L - T;
    const uint32_t U = Lg ? (Lg + kUnit - 1) / kUnit : 1u;
    const uint32_t R = active ? (U + kG - 1) / kG : 0u;
    const uint32_t pad = U * kUnit - Lg;
    const int u0 = (int)U - kG * (int)R + g;
    // ordinary loads: round 0 and the tail line (lane g its 16-B piece g)
    uint32_t w0[kWords];
    load_unit0<false, false>(w0, u0, fp, Lg, pad, gptr(reinterpret_cast<const uint8_t *>(p.consts)));
    u32x4 tl = {0, 0, 0, 0};
    if (active && 16u * (uint32_t)g < T) tl = *reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(fp + Lg + 16 * g);
    // DMA sources, relative to the group's first frame
    const uint64_t gb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)off);
    const uint8_t *const gbase = p.base + gb;
    const uint32_t relE = (uint32_t)(off - gb) + Lg;
    uint32_t src[4], lim[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int fl = 8 * (2 * q + (lane >> 5));  // first hash lane of this DMA lane's frame
        const uint32_t Eq = __shfl(relE, fl), Rq = __shfl(R, fl);
        lim[q] = Rq > 1u ? Eq : 0u;
        src[q] = Rq > 1u ? Eq - (Rq - 1u) * kRound + (uint32_t)((lane >> 2) & 7) * 64u + 16u * (uint32_t)(((lane & 3) - (lane >> 4)) & 3)
                         : 0u;
    }
    uint32_t Rmax = R;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) Rmax = max(Rmax, (uint32_t)__shfl_xor(Rmax, o));
    Rmax = __builtin_amdgcn_readfirstlane(Rmax);
    auto issue = [&] {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (src[q] < lim[q])
                __builtin_amdgcn_global_load_lds((const void *)(gbase + src[q]), LDSP((char *)s_lds + slot + q * 1024), 16, 0, 2);
            src[q] += kRound;
        }
    };
    if (Rmax > 1u) issue();
    // round 0 (as hash_frame; the seed cannot spill: pad <= 60 for whole-word frames)
    const uint32_t seed = (f == 0) ? p.seed0 : p.seed_rest;
    uint32_t acc = 0;
    if (R > 0) {
        if (u0 == 0 && Lg >= 4) unit0_line_shift(w0, fp, pad);
        unit0_finish(w0, u0, Lg, pad, seed);
#pragma unroll
        for (int i = 0; i < kWords; i++) acc = tb.step(acc, w0[i]);
    }
    for (uint32_t k = 1; k < Rmax; k++) {
        u32x4 cur[4];
        asm volatile("s_waitcnt vmcnt(0)\n\t"
                     "ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(cur[0]), "=&v"(cur[1]), "=&v"(cur[2]), "=&v"(cur[3])
                     : "v"(rd[0]), "v"(rd[1]), "v"(rd[2]), "v"(rd[3])
                     : "memory");
        if (k + 1u < Rmax) issue();
        uint32_t a = tb.advance(acc, gap_map(3));
#pragma unroll
        for (int q = 0; q < 4; q++) {
            a = tb.step(a, cur[q].x);
            a = tb.step(a, cur[q].y);
            a = tb.step(a, cur[q].z);
            a = tb.step(a, cur[q].w);
        }
        acc = k < R ? a : acc;
    }
    if (TAB != 0) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t other = __shfl_xor(acc, 1 << j);
            const bool right = (g >> j) & 1;
            acc = tb.advance(right ? other : acc, tree_map(j)) ^ (right ? acc : other);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) acc ^= __shfl_xor(acc, 1 << j);
    }
    // the tail: lane G - 1 feeds piece after piece, word by word
    uint32_t Tmax = T;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) Tmax = max(Tmax, (uint32_t)__shfl_xor(Tmax, o));
    Tmax = __builtin_amdgcn_readfirstlane(Tmax);
    for (uint32_t pc = 0; 16u * pc < Tmax; pc++) {
        const int from = (lane & ~(kG - 1)) | (int)pc;
        const uint32_t w[4] = {(uint32_t)__shfl(tl.x, from), (uint32_t)__shfl(tl.y, from), (uint32_t)__shfl(tl.z, from),
                               (uint32_t)__shfl(tl.w, from)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t a = tb.step(acc, w[j]);
            acc = (16u * pc + 4u * (uint32_t)j < T) ? a : acc;
        }
    }
    if (active && g == kG - 1) p.out_crc[f] = acc ^ p.xorout;
}

template <int TAB>
__global__ __launch_bounds__(kBlock) void k_ring(const FrameParams p)
{
    build_compact<TAB>(p.consts);
    const int lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t slot = kRing + wid * 4096u;
    const Tab<TAB> tb(lane);
    uint32_t rd[4];
#pragma unroll
    for (int k = 0; k < 4; k++) rd[k] = slot + (uint32_t)lane * 64u + 16u * (uint32_t)((k + (lane >> 2)) & 3);
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + wid, nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t fb = wave * 8; fb < p.n; fb += nwaves * 8) ring_group<TAB>(p, fb, lane, slot, rd, tb);
}

template <typename F>
float timeit(F f, int reps = 5)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    f();
    CHECK(hipDeviceSynchronize());
    std::vector<float> t;
    for (int r = 0; r < reps; r++) {
        CHECK(hipEventRecord(a));
        f();
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    CHECK(hipGetLastError());
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return t[t.size() / 2];
}

static uint32_t host_crc(const uint8_t *b, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= b[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

typedef void (*Kern)(const FrameParams);
struct Arm {
    const char *name;
    Kern k;
    bool hashed;
    std::vector<float> ms;
};

int main(int argc, char **argv)
{
    const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
    constexpr uint32_t kN = 1u << 20, kLen = 16400, kStride = 16404;
    static_assert(kLen % 4 == 0 && kStride % 4 == 0, "whole-word frames: the micro's tail is fed by word steps");
    constexpr int kReps = 4;
    hipDeviceProp_t pr;
    CHECK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount;
    const size_t bytes = (size_t)kN * kStride;
    uint8_t *d;
    uint32_t *consts, *out_ref, *out_arm;
    CHECK(hipMalloc(&d, bytes + 256));
    CHECK(hipMalloc(&out_ref, (size_t)kN * 4));
    CHECK(hipMalloc(&out_arm, (size_t)kN * 4));
    std::vector<uint32_t> blob(kConstWords);
    fill_const_blob(blob.data());
    CHECK(hipMalloc(&consts, blob.size() * 4));
    CHECK(hipMemcpy(consts, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, (u32x4 *)d, (bytes + 256) / 16);
    CHECK(hipDeviceSynchronize());
    FrameParams p{};
    p.base = d;
    p.stride = kStride;
    p.flen = p.last_len = kLen;
    p.n = kN;
    p.seed0 = p.seed_rest = 0xFFFFFFFFu;
    p.xorout = 0xFFFFFFFFu;
    p.consts = consts;
    Arm arms[] = {{"plain", k_frames<8, 1, false, false>, true, {}},
                  {"ring-64K", k_ring<64>, true, {}},
                  {"ring-32K", k_ring<32>, true, {}},
                  {"ring-xor", k_ring<0>, false, {}}};
    auto launch = [&](const Arm &a, uint32_t *out) {
        FrameParams q = p;
        q.out_crc = out;
        hipLaunchKernelGGL(a.k, dim3(cus), dim3(kBlock), 0, 0, q);
    };
    printf("mb16: %u frames of %u B at stride %u (%.2f GiB), %d CUs x 16 waves, G = %d\n", kN, kLen, kStride,
           (double)bytes / (1 << 30), cus, kG);
    // resources and agreement
    std::vector<uint32_t> ref(kN), got(kN);
    bool all_ok = true;
    for (Arm &a : arms) {
        if (pmc && !strcmp(a.name, "ring-xor")) continue;
        hipFuncAttributes fa;
        CHECK(hipFuncGetAttributes(&fa, (const void *)a.k));
        const bool first = &a == &arms[0];
        CHECK(hipMemset(first ? out_ref : out_arm, 0, (size_t)kN * 4));
        launch(a, first ? out_ref : out_arm);
        CHECK(hipDeviceSynchronize());
        CHECK(hipGetLastError());
        const char *verdict = "not compared";
        if (first) {
            CHECK(hipMemcpy(ref.data(), out_ref, (size_t)kN * 4, hipMemcpyDeviceToHost));
            bool ok = true;
            std::vector<uint8_t> fr(kLen);
            for (uint32_t f : {0u, 12345u, kN - 1}) {
                CHECK(hipMemcpy(fr.data(), d + (size_t)f * kStride, kLen, hipMemcpyDeviceToHost));
                ok = ok && host_crc(fr.data(), kLen) == ref[f];
            }
            verdict = ok ? "3 frames equal the host CRC" : "MISMATCH with the host CRC";
            all_ok = all_ok && ok;
        } else if (a.hashed) {
            CHECK(hipMemcpy(got.data(), out_arm, (size_t)kN * 4, hipMemcpyDeviceToHost));
            size_t bad = 0;
            for (uint32_t f = 0; f < kN; f++) bad += got[f] != ref[f];
            verdict = bad ? "MISMATCH with plain" : "all CRCs equal plain's";
            if (bad) printf("  %zu of %u frames differ\n", bad, kN);
            all_ok = all_ok && !bad;
        }
        printf("%-9s LDS %6zu B  VGPRs %3d  scratch %zu B  %s\n", a.name, fa.sharedSizeBytes, fa.numRegs, fa.localSizeBytes, verdict);
        fflush(stdout);
        if (pmc) {
            launch(a, first ? out_ref : out_arm);
            CHECK(hipDeviceSynchronize());
        }
    }
    if (pmc || !all_ok) {
        printf(all_ok ? "done\n" : "FAILED\n");
        return all_ok ? 0 : 1;
    }
    const double in_bytes = (double)kN * kLen;
    for (int rep = 0; rep < kReps; rep++)
        for (Arm &a : arms) {
            const float ms = timeit([&] { launch(a, &a == &arms[0] ? out_ref : out_arm); });
            a.ms.push_back(ms);
            printf("rep %d %-9s %.4f ms %7.1f GB/s of CRC input\n", rep, a.name, ms, in_bytes / ms / 1e6);
            fflush(stdout);
        }
    auto med = [](std::vector<float> v) {
        std::sort(v.begin(), v.end());
        return 0.5f * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
    };
    for (Arm &a : arms) {
        const float lo = *std::min_element(a.ms.begin(), a.ms.end()), hi = *std::max_element(a.ms.begin(), a.ms.end());
        printf("%-9s median %.4f ms %7.1f GB/s  spread %.4f ms\n", a.name, med(a.ms), in_bytes / med(a.ms) / 1e6, hi - lo);
    }
    const float pm = med(arms[0].ms);
    const float spread = *std::max_element(arms[0].ms.begin(), arms[0].ms.end()) - *std::min_element(arms[0].ms.begin(), arms[0].ms.end());
    const float best = std::min(med(arms[1].ms), med(arms[2].ms));
    printf("gate (timing half): best hashed ring arm %.4f ms against plain %.4f ms, margin %+.4f ms, twice plain's spread %.4f ms: %s\n",
           best, pm, pm - best, 2 * spread, pm - best > 2 * spread ? "PASS" : "FAIL");
    printf("done\n");
    return 0;
}
