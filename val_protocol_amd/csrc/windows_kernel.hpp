// windows_kernel.hpp -- the kernels behind val_crc32_file_windows_dev and the
// three resume calls (gfx950): the CRC-32 of one byte window per file, for many
// files whose addresses, sizes and windows live in HBM, in one short pipeline
// with no host round trip. Included by
// val_crc32_hip.hip.
//
//   k_win_count   one thread per file: the call's rule (the generic window, or
//                 one of resume_rules.h) gives the window; it is validated
//                 (inside the file, judged without wrap-around, and at most
//                 max_len), its chunk count written, its accumulator and
//                 arrival count zeroed. A file without chunks (an empty or
//                 refused window, a file the rule does not hash) is finished
//                 here.
//   k_scan_first  (scan_kernel.hpp) first = exclusive scan of the chunk counts.
//   k_win_hash    persistent grid over the flat space of all chunks. The chunk
//                 size W = 2^k0 is one for the call (the host picks it from
//                 max_len and n_files, never from a length), so one set of LDS
//                 maps "advance W * 2^i bytes" serves every file. A wave takes
//                 a chunk, finds its file by binary search in `first`, and
//                 hashes it with hash_frame at 64 lanes as k_region does. A
//                 window is cut into C = ceil(len / W) chunks anchored at its
//                 END: only chunk 0 can be short, and it carries the seed.
//                 Chunk c's register, advanced over the (C - 1 - c) * W bytes
//                 behind it (one map per set bit: C <= 2^16), is XORed into the
//                 file's accumulator with a device-scope atomic: the advance is
//                 linear and XOR commutes, so the sum is bit-exact in any
//                 arrival order. A workgroup's 16 waves take 16 consecutive
//                 chunks per step; when those are one file's, wave 0 folds the
//                 16 registers first (k_region's shuffle tree) and the file
//                 gets one atomic for them: with an atomic per chunk, thousands
//                 of waves on one file's word cost more than the hashing
//                 (DESIGN.md section 5). The XOR has returned before the count-
//                 in (k_region's ordering); the arrival that completes the
//                 count takes the sum, finalizes it and finishes the file (the
//                 CRC, and in the resume calls what follows from it). No
//                 workgroup waits for another; inside one, a barrier per step.
// Reads: hash_frame's branch-free path (crc_kernels.hpp load_unit0 BF): whole
// 64-B units inside the window by dwordx4, the short first unit by dword loads
// clamped to the window's first dword, up to three tail bytes; a window of
// fewer than 4 bytes on the unit grid by byte loads. So only aligned dwords
// that overlap the window are read from a file, and no byte of a refused
// window. Lanes without a unit read the constant blob.
#pragma once

#include "crc_kernels.hpp"
#include "resume_rules.h"

namespace vcrc {

constexpr int kWinCountBlock = 256;     // threads per workgroup of k_win_count
constexpr uint32_t kWinK0Min = 12, kWinK0Max = 16;  // W = 4 .. 64 KiB
constexpr uint64_t kWinMaxLen = (uint64_t)1 << (kWinK0Max + kNumPowMaps);  // 2^32: C <= 2^16 at W = 64 KiB

enum : uint32_t { kWinGeneric = 0, kWinTail = 1, kWinRequest = 2, kWinCheck = 3 };

struct WinParams {
    uint32_t mode;               // kWin*
    uint32_t n_files;
    uint32_t k0;                 // log2 of the chunk bytes
    uint64_t max_len;
    const uint64_t *file_ptr;    // device address of byte 0 of each file
    // the file's size: file_size (generic, request) or existing (tail, check)
    const uint64_t *file_size;
    const uint64_t *win_off;     // generic: the window; check: req_off
    const uint64_t *win_len;     // generic
    const uint32_t *req_len;     // check: the window's length
    const uint32_t *req_crc;     // check: the sender's CRC
    const uint64_t *incoming;    // tail, check
    const int32_t *action;       // request; check (nullable: every file)
    const uint64_t *resume_off;  // request: the receiver's proposal; check: rec_resume_off
    const uint64_t *verify_len;  // request
    uint64_t tail_cap, min_verify;  // tail
    int mismatch_skip;              // tail, check
    // outputs
    uint32_t *out_crc;           // generic crc, tail verify_crc, request req_crc, check local_crc (nullable there)
    int32_t *out_status;         // generic, request: nullable; check: result
    int32_t *out_action;         // tail
    uint64_t *out_off;           // tail resume_off, request req_off, check written
    uint64_t *out_len64;         // tail verify_len
    uint32_t *out_len32;         // request req_len
    // workspace (val_file_windows_work_bytes)
    uint64_t *wbase;             // absolute address of the window's first byte
    uint64_t *wlen;
    uint32_t *first;             // n_files + 1, written by k_scan_first
    uint32_t *wcnt;              // chunks per file
    uint32_t *acc;               // XOR of the advanced chunk registers
    uint32_t *arrived;           // chunks counted in
    const uint32_t *consts;
};

// What a finished window leaves behind: crc is the finalized CRC-32 of an
// accepted window (ok), and ignored for a refused one.
__device__ __forceinline__ void win_finish(const WinParams &p, uint32_t s, uint32_t crc, bool ok)
{
    const uint32_t c = ok ? crc : 0u;
    switch (p.mode) {
    case kWinTail:
        p.out_crc[s] = c;
        break;
    case kWinCheck: {
        uint64_t off = 0;
        const val_status_t st =
            val_rule_verdict(ok, c, p.req_crc[s], p.mismatch_skip, p.resume_off[s], p.incoming[s], &off);
        if (p.out_crc) p.out_crc[s] = c;
        p.out_status[s] = (int32_t)st;
        p.out_off[s] = off;
        break;
    }
    default:  // generic, request
        p.out_crc[s] = c;
        if (p.out_status) p.out_status[s] = ok ? (int32_t)VAL_OK : (int32_t)VAL_ERR_INVALID_ARG;
        break;
    }
}

__global__ __launch_bounds__(kWinCountBlock) void k_win_count(const WinParams p)
{
    const uint64_t s64 = (uint64_t)blockIdx.x * kWinCountBlock + threadIdx.x;
    if (s64 >= p.n_files) return;
    const uint32_t s = (uint32_t)s64;
    bool take = true;  // the file has a window to hash
    uint64_t off = 0, len = 0;
    switch (p.mode) {
    case kWinTail: {
        uint64_t roff = 0, vlen = 0;
        const uint64_t existing = p.file_size[s];
        const int action =
            val_rule_tail_window(existing, p.incoming[s], p.tail_cap, p.min_verify, p.mismatch_skip, &roff, &vlen);
        p.out_action[s] = action;
        p.out_off[s] = roff;
        p.out_len64[s] = vlen;
        take = action == VAL_RESUME_VERIFY_FIRST;
        if (take) {
            off = existing - vlen;
            len = vlen;
        } else {
            p.out_crc[s] = 0u;
        }
        break;
    }
    case kWinRequest: {
        const uint64_t roff = p.resume_off[s];
        uint64_t start = roff;
        uint32_t v32 = 0;
        take = p.action[s] == VAL_RESUME_VERIFY_FIRST && val_rule_request_window(roff, p.verify_len[s], &start, &v32);
        if (take) {
            off = start;
            len = v32;
        }
        p.out_off[s] = take ? start : roff;
        p.out_len32[s] = take ? v32 : 0u;
        if (!take) {
            p.out_crc[s] = 0u;
            if (p.out_status) p.out_status[s] = (int32_t)VAL_OK;
        }
        break;
    }
    case kWinCheck:
        take = !p.action || p.action[s] == VAL_RESUME_VERIFY_FIRST;
        if (take) {
            off = p.win_off[s];
            len = p.req_len[s];
        }
        break;
    default:
        off = p.win_off[s];
        len = p.win_len[s];
        break;
    }
    bool ok = false;
    uint32_t C = 0;
    if (take) {
        const uint64_t size = p.file_size[s];
        ok = len <= p.max_len && off <= size && len <= size - off;
        if (ok) C = (uint32_t)((len + (((uint64_t)1 << p.k0) - 1u)) >> p.k0);  // <= 2^16: len <= max_len <= 2^(k0+16)
    }
    p.wcnt[s] = C;
    p.wbase[s] = p.file_ptr[s] + off;  // wraps by definition; used only when C > 0
    p.wlen[s] = len;
    p.acc[s] = 0u;
    p.arrived[s] = 0u;
    if (take && C == 0u) win_finish(p, s, 0u, ok);  // the empty window's CRC is 0
}

// One chunk's (n = 1) or one workgroup's (n = 16) register v, which ends
// `behind` chunks in front of its window's end, goes into file s's sum: advanced
// over behind * W bytes (one map per set bit: behind < 2^16), XORed in, counted
// in. The XOR has been performed (its value returned) before the count-in, so
// the arrival that completes the count finds every term in the sum.
__device__ __forceinline__ void win_fold(const WinParams &p, uint32_t s, uint32_t C, uint32_t v, uint32_t behind,
                                         uint32_t n)
{
#pragma unroll
    for (int i = 0; i < (int)kNumPowMaps; i++)
        if ((behind >> i) & 1u) v = map_apply(v, pow_map(i));
    const uint32_t old = atomicXor(&p.acc[s], v);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(old) : "memory");
    const uint32_t arrived = atomicAdd(&p.arrived[s], n);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(arrived) : "memory");
    if (arrived + n == C) win_finish(p, s, atomicExch(&p.acc[s], 0u) ^ 0xFFFFFFFFu, true);
}

__global__ __launch_bounds__(kBlock) void k_win_hash(const WinParams p)
{
    // what the waves of a workgroup leave each other per step: the chunk's register and its file
    // (two slots in turn, so one barrier per step)
    __shared__ uint32_t s_state[2][kWavesPerBlock];
    __shared__ uint32_t s_file[2][kWavesPerBlock];
    constexpr uint32_t kNoFile = 0xFFFFFFFFu;
    LdsImage im;
    lds_tables_issue(p.consts, im);
    PowImage pim;
    lds_pow_issue(p.consts, p.k0, pim);
    lds_tables_write(im);
    lds_pow_write(pim);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const SliceBases sb = slice_bases((uint32_t)(lane & 31) << 2);
    const uint32_t n = p.n_files;
    const uint64_t total = p.first[n];
    const uint64_t W = (uint64_t)1 << p.k0;
    FrameParams q{};
    q.seed0 = 0xFFFFFFFFu;  // chunk 0 carries the seed; the others start from zero
    q.consts = p.consts;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint32_t slot = 0;
    // A step of the workgroup is 16 consecutive chunks, one per wave. The trip count depends on
    // blockIdx and total alone, and every wave meets the one barrier of every step.
    for (uint64_t u0 = (uint64_t)blockIdx.x * kWavesPerBlock; u0 < total; u0 += stride, slot ^= 1u) {
        const uint64_t u = u0 + wi;
        const bool real = u < total;
        uint32_t s = 0, C = 0, c = 0, st = 0;
        if (real) {
            // the file of chunk u: first[s] <= u < first[s + 1] (first[0] = 0 <= u < total = first[n])
            uint32_t hi_s = n;
            while (hi_s - s > 1u) {
                const uint32_t mid = s + (hi_s - s) / 2u;
                if ((uint64_t)p.first[mid] <= u) s = mid;
                else hi_s = mid;
            }
            C = p.wcnt[s];
            c = (uint32_t)(u - p.first[s]);  // < C
            const uint64_t L = p.wlen[s];
            const uint64_t hi = L - (uint64_t)(C - 1u - c) * W;
            const uint64_t lo = hi > W ? hi - W : 0u;
            q.n = C;
            st = hash_frame<64, 1, false, true>(q, c, true, p.wbase[s] + lo, (uint32_t)(hi - lo), lane, sb, 64, [] {});
        }
        if (lane == 63) {
            s_state[slot][wi] = st;
            s_file[slot][wi] = real ? s : kNoFile;
        }
        __syncthreads();
        // The files of the step's first and last chunk are equal iff all 16 chunks are one file's
        // (first[] is monotone): consecutive chunks c .. c + 15 of it. Wave 0 then folds the 16
        // registers as k_region does (level j advances the left half over W * 2^j bytes) and the
        // file's sum takes one term for them; a step that spans files, or the last, partial one,
        // leaves a term per chunk.
        const uint32_t f_last = s_file[slot][kWavesPerBlock - 1];
        const bool whole = f_last != kNoFile && s_file[slot][0] == f_last;
        if (whole) {
            if (wi == 0) {
                uint32_t v = lane < kWavesPerBlock ? s_state[slot][lane] : 0u;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t other = __shfl_xor(v, 1 << j);
                    const bool right = (lane >> j) & 1;
                    const uint32_t left = right ? other : v;
                    v = map_apply(left, pow_map(j)) ^ (right ? v : other);
                }
                if (lane == kWavesPerBlock - 1) win_fold(p, s, C, v, C - (uint32_t)kWavesPerBlock - c, kWavesPerBlock);
            }
        } else if (real && lane == 63) {
            win_fold(p, s, C, st, C - 1u - c, 1u);
        }
    }
}

}  // namespace vcrc
