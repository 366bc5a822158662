// unpack_kernel.hpp -- the receive-side counterpart of k_pack (gfx950): the
// kernels behind val_frame_unpack_batch_dev. Included by val_crc32_hip.hip.
//
// A window of received frames in HBM is delivered into a GPU-resident file in
// a short pipeline on one stream: the verify launches
// of val_crc32_verify_frames_ex_dev give ok[i] and the payload states pay[i];
// then
//   k_unpack_parse  grid-wide, one frame per thread: the header facts of
//                   val_frame_data_offsets / val_frame_payload_lens
//                   (csrc/val_wire.c) into the workspace;
//   k_unpack_order  one workgroup: the receiver's ordering rule (reference
//                   src/val_receiver.c:871-895) over the whole batch, the
//                   destinations dst[i], `written`, the counters and the
//                   rolling file CRC state;
//   k_unpack<G>     the hot path: every accepted payload copied to
//                   file + dst[i]. k_pack with the hashing removed.
// val_frame_unpack_files_dev delivers a window that holds frames of many
// files through the same stages: one verify, one parse (which also marks
// every frame as not accepted), k_unpack_order_files (a grid of workgroups,
// each applying the rule to whole files, one after the other, and storing
// absolute addresses in dst[i]) and one k_unpack<G> with file = NULL.
// A payload may be written only when its own CRC matched (known after its last
// byte was hashed) and its offset equals `written` (which depends on the
// verdicts of every earlier frame), so the write cannot be fused into the
// hash pass: a corrupt frame, or a stale duplicate with a valid CRC, would
// land on bytes already accepted.
//
// None of these kernels touches the LDS table image of crc_device.hpp.
#pragma once

#include "crc_device.hpp"
#include "val_wire.h"

namespace vcrc {

constexpr int kUnpackBlock = 256;  // threads per k_unpack workgroup (4 waves)
// Resident k_unpack workgroups per CU the persistent grid is sized for: the
// kernel holds no LDS, so VGPRs decide. Every instantiation stays within 64
// VGPRs (from -Rpass-analysis=kernel-resource-usage):
// 8 waves per SIMD, 32 per CU.
constexpr int kUnpackBlocksPerCU = 8;
constexpr int kOrderBlock = 1024;  // k_unpack_order: one frame per thread and chunk

struct UnpackParams {
    const uint8_t *base;
    const uint64_t *off;   // NULL: strided mode
    const uint32_t *len;
    uint64_t stride;
    uint32_t flen;
    uint32_t n;
    const uint8_t *ok;     // verify's verdicts
    uint8_t *file;
    uint64_t file_cap;
    // workspace
    uint64_t *foff;        // parsed offset: explicit, IMPLIED, or NOT_DATA (also when ok[i] == 0)
    uint32_t *plen;        // payload bytes
    const uint32_t *pay;   // payload states from the verify stage
    uint64_t *dst;         // destination in the file, or VAL_FRAME_NOT_ACCEPTED
    // in/out and results
    uint64_t *written;
    uint32_t *file_state;  // nullable
    uint8_t *accept;       // nullable
    uint32_t *naccepted;   // nullable, incremented
    uint32_t *noverflow;   // nullable, incremented
    const uint32_t *consts;
    // val_frame_unpack_files_dev only: written, file_state, naccepted and
    // noverflow are then arrays over the files, and file / file_cap are unused
    uint32_t n_files;
    const uint32_t *first;      // n_files + 1 frame indices
    const uint64_t *file_ptr;   // the files' device addresses
    const uint64_t *file_caps;
    uint32_t *file_nbad;        // nullable, incremented
};

typedef uint32_t __attribute__((address_space(1))) uw32;
typedef u32x4u __attribute__((address_space(1))) uw32x4u;
typedef uint8_t __attribute__((address_space(1))) uw8;

// ---- header facts ----------------------------------------------------------
// Exactly val_frame_data_offsets and val_frame_payload_lens for frame i, with
// a frame that failed its CRC folded into NOT_DATA (it is never accepted).
// FILES (val_frame_unpack_files_dev): a frame that no file owns is visited by
// no order workgroup, so every frame starts as not accepted here.
template <bool FILES>
__global__ __launch_bounds__(256) void k_unpack_parse(const UnpackParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t L = p.len ? p.len[i] : p.flen;
    uint64_t fo = VAL_FRAME_OFFSET_NOT_DATA;
    uint32_t pre = VAL_WIRE_HEADER_SIZE;
    if (L >= VAL_WIRE_HEADER_SIZE) {
        gu8 *f = gptr(p.base) + (p.off ? p.off[i] : i * p.stride);
        const uint32_t type = f[0], flags = f[1];
        const bool expl = (flags & VAL_DATA_OFFSET_PRESENT) != 0;
        if (expl) pre += 8u;
        if (type == (uint32_t)VAL_PKT_DATA && p.ok[i]) {
            if (!expl) fo = VAL_FRAME_OFFSET_IMPLIED;
            else if (L >= VAL_WIRE_HEADER_SIZE + 8u)
                fo = (uint64_t)ld32(f + 8) | ((uint64_t)ld32(f + 12) << 32);
        }
    }
    p.foff[i] = fo;
    p.plen[i] = L >= pre ? L - pre : 0u;
    if (FILES) {
        p.dst[i] = VAL_FRAME_NOT_ACCEPTED;
        if (p.accept) p.accept[i] = 0u;
    }
}

// ---- ordering --------------------------------------------------------------
// Index of the first thread of the workgroup whose `pred` holds (kOrderBlock:
// none), and through *below the number of threads before it whose `other`
// holds. One barrier: the wave masks go through `slot`, which the caller
// alternates between two buffers so that the next call's writes cannot overtake
// this call's reads. After the barrier lane l holds the masks of wave l % 16
// and two ballots say which waves have a hit; the count walks the masks only
// when some `other` holds at all (a capacity skip: rare).
__device__ __forceinline__ uint32_t order_first(bool pred, bool other, uint64_t (*slot)[kOrderBlock / 64],
                                                uint32_t *below)
{
    constexpr uint32_t kWaves = kOrderBlock / 64;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t mp = __ballot(pred), mo = __ballot(other);
    if (lane == 0) {
        slot[0][wave] = mp;
        slot[1][wave] = mo;
    }
    __syncthreads();
    const uint64_t a = slot[0][lane % kWaves], b = slot[1][lane % kWaves];
    const uint32_t hit = (uint32_t)__ballot(a != 0) & ((1u << kWaves) - 1u);
    const uint32_t any_other = (uint32_t)__ballot(b != 0) & ((1u << kWaves) - 1u);
    uint32_t first = kOrderBlock, fw = kWaves, bit = 0;
    if (hit) {
        fw = (uint32_t)__builtin_ctz(hit);
        bit = (uint32_t)__builtin_ctzll(__shfl(a, (int)fw));
        first = fw * 64u + bit;
    }
    uint32_t cnt = 0;
    if (any_other) {
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint64_t bw = slot[1][w];
            if (w < fw) cnt += (uint32_t)__builtin_popcountll(bw);
            else if (w == fw) cnt += (uint32_t)__builtin_popcountll(bw & ((1ull << bit) - 1ull));
        }
    }
    *below = cnt;
    return first;
}

// Advance raw register v over n < 2^48 zero bytes through the nibble maps
// "advance 2^k bytes" in `pow` (the blob's kConstPow maps, copied to LDS): 8
// lookups per set bit of n.
__device__ __forceinline__ uint32_t order_map(uint32_t v, const uint32_t *m)
{
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) r ^= m[k * 16 + ((v >> (4 * k)) & 15u)];
    return r;
}

__device__ __forceinline__ uint32_t order_shift(uint32_t v, uint64_t n, const uint32_t *pow)
{
    while (n) {
        v = order_map(v, pow + (uint32_t)__builtin_ctzll(n) * 128u);
        n &= n - 1;
    }
    return v;
}

// shift(v1, n1) ^ shift(v2, n2) with the two chains of lookups side by side:
// thread 0's wave advances the incoming state next to its frame's
// contribution in the time of one shift.
__device__ __forceinline__ uint32_t order_shift2(uint32_t v1, uint64_t n1, uint32_t v2, uint64_t n2, const uint32_t *pow)
{
    while (n1 | n2) {
        const uint32_t r1 = order_map(v1, pow + (n1 ? (uint32_t)__builtin_ctzll(n1) : 0u) * 128u);
        const uint32_t r2 = order_map(v2, pow + (n2 ? (uint32_t)__builtin_ctzll(n2) : 0u) * 128u);
        v1 = n1 ? r1 : v1;
        v2 = n2 ? r2 : v2;
        n1 &= n1 - 1;  // 0 stays 0
        n2 &= n2 - 1;
    }
    return v1 ^ v2;
}

// The receiver's rule over frames first..last-1 with state W = *written, in
// chunks of one frame per thread. Within a chunk the frames are not walked one
// by one: an exclusive scan of the candidates' payload lengths proposes every
// frame's position; a find-first gives the next frame that can be accepted at
// the known W (everything before it is skipped in that step), a second one the
// first later candidate that disagrees with its proposed position (everything
// before it is accepted in that step). The cost is two barriers per accepted
// run, whatever the number of skipped frames.
// The file CRC state folds chunk by chunk: an accepted frame contributes its
// payload state advanced over the bytes accepted after it in the chunk, the
// incoming state advances over the chunk's bytes (thread 0, beside its own frame),
// and the XOR of all of them is the new state. A chunk accepts fewer than
// 2^42 bytes, so every distance fits order_shift.
struct OrderShared {
    uint64_t pos[kOrderBlock + 1];  // exclusive scan of candidate payload bytes; [kOrderBlock] = total
    uint64_t wsum[kOrderBlock / 64];
    uint64_t mask[2][2][kOrderBlock / 64];
    uint32_t pow[kBlobPowMaps * 128];
    uint32_t x, nacc;
};
static_assert(kBlobPowMaps * 128 % kOrderBlock == 0, "whole rounds of the workgroup copy the maps");

// The blob's pow maps into LDS, once per workgroup. Published by the first
// barrier of the first chunk (the scan's): the fold is the only reader.
__device__ __forceinline__ void order_copy_pow(const UnpackParams &p, OrderShared &sh)
{
#pragma unroll
    for (uint32_t r = 0; r < kBlobPowMaps * 128 / kOrderBlock; r++)
        sh.pow[r * kOrderBlock + threadIdx.x] = p.consts[kConstPow + r * kOrderBlock + threadIdx.x];
}

// A value every lane holds alike, moved to scalar registers: what a workgroup
// loads per file after its first stores comes per lane otherwise, and with
// those in VGPRs k_unpack_order_files spilled.
__device__ __forceinline__ uint64_t order_uniform(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// One file's frames, by the whole workgroup. dst[i] = base + the frame's
// offset in the file: base is 0 for k_unpack_order (the scatter adds p.file)
// and the file's address for k_unpack_order_files. Everything a file's pass
// keeps between chunks (W, the state, the counters, the ballot slot in turn,
// the chunk loaded ahead, sh.x and sh.nacc) starts afresh here, and the
// barrier in front of the results is also the one between this range's last
// use of `sh` and the next range's first. FILES adds the per-file count of
// failed trailers from ok[]; k_unpack_order does not load ok[] at all.
template <bool FILES>
__device__ __forceinline__ void order_range(const UnpackParams &p, OrderShared &sh, const uint64_t first,
                                            const uint64_t last, const uint64_t cap, const uint64_t base,
                                            uint64_t *written, uint32_t *file_state, uint32_t *naccepted,
                                            uint32_t *noverflow, uint32_t *file_nbad)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint64_t W = *written;
    uint32_t state = file_state ? *file_state : 0u;  // thread 0's copy is the live one
    uint32_t novf = 0, flip = 0, nbad = 0;
    if (t == 0) sh.x = 0u, sh.nacc = 0u;
    // the next chunk's header facts and payload state are loaded while this one is ordered
    uint64_t fo_n = VAL_FRAME_OFFSET_NOT_DATA;
    uint32_t pl_n = 0, py_n = 0;
    uint32_t ok_n = 1;  // kept as loaded: a comparison here would wait for the load where it is issued
    if (first + t < last) {
        fo_n = p.foff[first + t];
        pl_n = p.plen[first + t];
        if (file_state) py_n = p.pay[first + t];
        if (FILES) ok_n = p.ok[first + t];
    }
    for (uint64_t c0 = first; c0 < last; c0 += kOrderBlock) {
        const uint64_t i = c0 + t;
        const bool valid = i < last;
        const uint64_t fo = fo_n;
        const uint32_t pl = pl_n, py = py_n;
        if (FILES) nbad += (uint32_t)__builtin_popcountll(__ballot(ok_n == 0));
        fo_n = VAL_FRAME_OFFSET_NOT_DATA, pl_n = 0, py_n = 0, ok_n = 1;
        if (i + kOrderBlock < last) {
            fo_n = p.foff[i + kOrderBlock];
            pl_n = p.plen[i + kOrderBlock];
            if (file_state) py_n = p.pay[i + kOrderBlock];
            if (FILES) ok_n = p.ok[i + kOrderBlock];
        }
        const bool cand = fo != VAL_FRAME_OFFSET_NOT_DATA;
        const bool impl = fo == VAL_FRAME_OFFSET_IMPLIED;
        // exclusive scan of the candidates' payload bytes
        const uint64_t mine = cand ? (uint64_t)pl : 0u;
        uint64_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(incl, d);
            if ((int)lane >= d) incl += o;
        }
        if (lane == 63u) sh.wsum[wave] = incl;
        __syncthreads();
        uint64_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kOrderBlock / 64; w++) {
            const uint64_t v = sh.wsum[w];
            if (w < wave) wbase += v;
            total += v;
        }
        const uint64_t pos = wbase + incl - mine;
        sh.pos[t] = pos;
        if (t == 0) sh.pos[kOrderBlock] = total;
        // (published by the barrier of the first order_first below)
        const uint64_t W0 = W;
        bool acc = false;
        uint64_t my_dst = 0;
        uint32_t s = 0;
        while (s < kOrderBlock) {
            // the next frame that can be accepted at W; candidates before it that match W
            // but do not fit the file are the capacity skips
            const bool match = cand && t >= s && (impl || fo == W);
            const bool fits = W <= cap && (uint64_t)pl <= cap - W;
            uint32_t below = 0;
            const uint32_t j = order_first(match && fits, match && !fits, sh.mask[flip], &below);
            flip ^= 1u;
            novf += below;
            if (j == kOrderBlock) break;
            // every candidate from j on, placed as if all candidates before it were accepted
            const uint64_t prop = W + (pos - sh.pos[j]);
            const bool agree = (impl || fo == prop) && prop <= cap && (uint64_t)pl <= cap - prop;
            uint32_t unused = 0;
            const uint32_t b = order_first(cand && t > j && !agree, false, sh.mask[flip], &unused);
            flip ^= 1u;
            if (cand && t >= j && t < b) {
                acc = true;
                my_dst = prop;
            }
            W += sh.pos[b] - sh.pos[j];  // b == kOrderBlock: the chunk's total
            s = b;                       // frame b is judged against the new W in the next step
        }
        if (valid) {
            p.dst[i] = acc ? base + my_dst : VAL_FRAME_NOT_ACCEPTED;
            if (p.accept) p.accept[i] = acc ? 1u : 0u;
        }
        const uint64_t am = __ballot(acc);
        if (lane == 0 && am) atomicAdd(&sh.nacc, (uint32_t)__builtin_popcountll(am));
        if (file_state && W != W0) {  // uniform: every thread tracks the same W
            uint32_t x = 0;
            const uint64_t after = W - (my_dst + pl);  // bytes accepted after this frame in the chunk
            if (wave == 0) x = order_shift2(acc ? py : 0u, acc ? after : 0u, t == 0 ? state : 0u, t == 0 ? W - W0 : 0u, sh.pow);
            else if (acc && pl) x = order_shift(py, after, sh.pow);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) x ^= __shfl_xor(x, d);
            if (lane == 0 && x) atomicXor(&sh.x, x);
            __syncthreads();
            if (t == 0) {
                state = sh.x;
                sh.x = 0u;
            }
        }
        // the next chunk's first barrier (the scan's) orders these shared writes before its own
    }
    __syncthreads();
    if (t == 0) {
        *written = W;
        if (file_state) *file_state = state;
        if (naccepted && sh.nacc) atomicAdd(naccepted, sh.nacc);
        if (noverflow && novf) atomicAdd(noverflow, novf);
    }
    if (FILES && file_nbad && lane == 0 && nbad) atomicAdd(file_nbad, nbad);  // every wave saw its own 64 frames per chunk
}

// One file: the whole batch is its range.
__global__ __launch_bounds__(kOrderBlock) void k_unpack_order(const UnpackParams p)
{
    __shared__ OrderShared sh;
    if (p.file_state) order_copy_pow(p, sh);
    order_range<false>(p, sh, 0, p.n, p.file_cap, 0, p.written, p.file_state, p.naccepted, p.noverflow, nullptr);
}

// Many files (val_frame_unpack_files_dev): workgroup b takes files b,
// b + gridDim.x, ... one after the other; file s owns the frames
// [first[s], first[s + 1]) clamped to [0, n] (a decreasing pair: none), and
// written, file_state and the counters are arrays over the files. The maps
// are copied once per workgroup. An empty file costs its two index reads.
__global__ __launch_bounds__(kOrderBlock) void k_unpack_order_files(const UnpackParams p)
{
    __shared__ OrderShared sh;
    if (p.file_state) order_copy_pow(p, sh);
    for (uint64_t s = blockIdx.x; s < p.n_files; s += gridDim.x) {
        const uint32_t a = p.first[s], b = p.first[s + 1];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(a, p.n));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(max(a, b), p.n));
        if (lo >= hi) continue;
        order_range<true>(p, sh, lo, hi, order_uniform(p.file_caps[s]), order_uniform(p.file_ptr[s]), p.written + s,
                          p.file_state ? p.file_state + s : nullptr, p.naccepted ? p.naccepted + s : nullptr,
                          p.noverflow ? p.noverflow + s : nullptr, p.file_nbad ? p.file_nbad + s : nullptr);
    }
}

// ---- scatter ---------------------------------------------------------------
// One accepted payload as a lane sees it, after the <= 3 head bytes that bring
// the destination to a dword boundary. Addresses are integers.
struct UnpackFrame {
    uint64_t dst;   // dword-aligned destination of body byte 0
    uint64_t src;   // source address of body byte 0
    uint64_t send;  // end of the payload in the source
    uint64_t nb;    // body bytes
};

// The 17 aligned source dwords covering the 64-B unit at body byte q (a[16]
// only when the source is misaligned against the destination grid): every one
// of them holds a payload byte.
__device__ __forceinline__ void unpack_load(uint32_t (&a)[kWords + 1], const UnpackFrame &d, uint64_t q)
{
    const uint64_t sb = d.src + q;
    const uint64_t s0 = sb & ~(uint64_t)3;
#pragma unroll
    for (int k = 0; k < kWords / 4; k++) {
        const u32x4u v = *reinterpret_cast<gu32x4u *>(s0 + 16u * k);
        a[4 * k + 0] = v.x;
        a[4 * k + 1] = v.y;
        a[4 * k + 2] = v.z;
        a[4 * k + 3] = v.w;
    }
    a[kWords] = 0;
    if (sb & 3u) a[kWords] = *reinterpret_cast<gu32 *>(s0 + 64u);
}

__device__ __forceinline__ void unpack_store(const uint32_t (&a)[kWords + 1], const UnpackFrame &d, uint64_t q)
{
    const uint32_t m = (uint32_t)((d.src + q) & 3u);
    const uint64_t up = d.dst + q;
#pragma unroll
    for (int k = 0; k < kWords / 4; k++) {
        u32x4u v;
        v.x = __builtin_amdgcn_alignbyte(a[4 * k + 1], a[4 * k + 0], m);
        v.y = __builtin_amdgcn_alignbyte(a[4 * k + 2], a[4 * k + 1], m);
        v.z = __builtin_amdgcn_alignbyte(a[4 * k + 3], a[4 * k + 2], m);
        v.w = __builtin_amdgcn_alignbyte(a[4 * k + 4], a[4 * k + 3], m);
        *reinterpret_cast<uw32x4u *>(up + 16u * k) = v;
    }
}

// The last, partial unit (r = 1..63 bytes at body byte q): dword by dword, only
// source dwords that overlap the payload, whole dwords as dword stores and the
// <= 3 bytes after them as byte stores.
__device__ __forceinline__ void unpack_partial(const UnpackFrame &d, uint64_t q, uint32_t r)
{
    const uint64_t sb = d.src + q;
    const uint64_t s0 = sb & ~(uint64_t)3;
    const uint32_t m = (uint32_t)(sb & 3u);
    uint32_t a[kWords + 1];
#pragma unroll
    for (int j = 0; j <= kWords; j++) {
        const uint64_t A = s0 + 4u * j;
        a[j] = 0;
        if (A < d.send && (j < kWords || m)) a[j] = *reinterpret_cast<gu32 *>(A);
    }
    const uint64_t up = d.dst + q;
    const uint32_t nd = r >> 2, tb = r & 3u;
#pragma unroll
    for (int i = 0; i < kWords; i++) {
        const uint32_t w = __builtin_amdgcn_alignbyte(a[i + 1], a[i], m);
        if ((uint32_t)i < nd) {
            *reinterpret_cast<uw32 *>(up + 4u * i) = w;
        } else if ((uint32_t)i == nd) {
#pragma unroll
            for (uint32_t b = 0; b < 3; b++)
                if (b < tb) *reinterpret_cast<uw8 *>(up + 4u * i + b) = (uint8_t)(w >> (8 * b));
        }
    }
}

// Copy frame f's payload with the G lanes of this lane's group (lane g of G).
// A frame that was not accepted costs the read of dst[f] and nothing else.
template <int G>
__device__ __forceinline__ void unpack_frame(const UnpackParams &p, uint64_t f, int g)
{
    const uint64_t at = p.dst[f];
    if (at == VAL_FRAME_NOT_ACCEPTED) return;
    const uint32_t n = p.plen[f];
    if (!n) return;
    const uint32_t L = p.len ? p.len[f] : p.flen;
    const uint64_t pstart = (uint64_t)(uintptr_t)p.base + (p.off ? p.off[f] : f * p.stride) + (L - n);
    const uint64_t D = (uint64_t)(uintptr_t)p.file + at;
    // the first partial dword of the destination: byte stores, never a read-modify-write
    const uint32_t h = min((uint32_t)(-D & 3u), n);
    if (g == 0) {
#pragma unroll
        for (uint32_t b = 0; b < 3; b++)
            if (b < h) *reinterpret_cast<uw8 *>(D + b) = *reinterpret_cast<gu8 *>(pstart + b);
    }
    UnpackFrame d;
    d.dst = D + h;
    d.src = pstart + h;
    d.send = pstart + n;
    d.nb = (uint64_t)n - h;
    const uint32_t U = (uint32_t)(d.nb >> 6);  // whole units
    const uint32_t r = (uint32_t)(d.nb & 63u);
    // whole units, lane g takes g, g + G, ...; one round of source dwords in flight ahead
    uint32_t u = (uint32_t)g;
    uint32_t nxt[kWords + 1];
    if (u < U) unpack_load(nxt, d, (uint64_t)u * kUnit);
    for (; u < U; u += G) {
        uint32_t a[kWords + 1];
#pragma unroll
        for (int i = 0; i <= kWords; i++) a[i] = nxt[i];
        if (u + G < U) unpack_load(nxt, d, (uint64_t)(u + G) * kUnit);
        unpack_store(a, d, (uint64_t)u * kUnit);
    }
    if (r && (U & (uint32_t)(G - 1)) == (uint32_t)g) unpack_partial(d, (uint64_t)U * kUnit, r);
}

template <int G>
__global__ __launch_bounds__(kUnpackBlock) void k_unpack(const UnpackParams p)
{
    constexpr int kGroups = 64 / G;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kUnpackBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kUnpackBlock) >> 6;
    for (uint64_t fb = wave * kGroups; fb < p.n; fb += nwaves * kGroups) {
        const uint64_t f = fb + (uint64_t)(lane / G);
        if (f < p.n) unpack_frame<G>(p, f, lane % G);
    }
}

}  // namespace vcrc
