// fill_kernel.hpp -- the planning kernels behind val_frame_fill_files_dev
// (gfx950): the sender's window-fill rule, val_frame_fill_window
// (csrc/val_wire.c), applied to many transfers at once, and its result laid out
// as the per-frame inputs of k_pack (pack_kernel.hpp). Included by
// val_crc32_hip.hip.
//
// The rule is a loop on the host, and closed-form per transfer (DESIGN.md
// section 4.11). With M = mtu - 12, frame j has room for M payload bytes, and
// for M - 8 if it is the explicit one. At most one frame is: the rule makes a
// frame explicit iff it starts at last_acked, and starts only grow. It is
// frame 0 when next == last_acked (a sender's case: last_acked <= next), and
// frame je when last_acked = next + je * M lies ahead on a frame start (what
// the host's loop does with such an input). So
//   * every frame that does not end the file has wire size mtu, explicit or
//     not, and frame j starts at j * mtu in its stream;
//   * frame j starts at file offset next + j * M, less 8 behind the explicit
//     frame;
//   * the file ends in frame F - 1, F = ceil(rem / M) with rem =
//     file_size - next, or ceil((rem + 8) / M) when the explicit frame is
//     among them;
//   * the capacity admits out_cap / mtu whole frames, and behind them the
//     file's last frame if that is the next one and fits what is left.
// Nothing walks:
//   k_fill_count  one thread per transfer: the count, stream_len, the new next.
//   k_scan_first  (scan_kernel.hpp) first = exclusive scan of the counts.
//   k_fill_desc   grid-wide over the n_files * max_frames slots: slot (s, j)
//                 with j < count[s] writes entry first[s] + j of k_pack's
//                 inputs, a slot index at or behind the total writes the
//                 padding entry: a frame k_pack rejects (pay_len above 65,535),
//                 which writes no byte and zeroes its crc_len, crc and hdr.
// Positions are 64-bit; j * M is formed only for j up to the count, where the
// product lies inside the file. No LDS, no scratch.
#pragma once

#include "crc_device.hpp"
#include "val_wire.h"

namespace vcrc {

constexpr int kFillBlock = 256;      // threads per workgroup, both kernels
constexpr int kFillBlocksPerCU = 8;  // k_fill_desc: persistent grid
constexpr uint32_t kFillReject = 0xFFFFFFFFu;  // pay_len of a padding entry: content above 65,535

struct FillParams {
    const uint64_t *file_pos;
    const uint64_t *file_size;
    uint64_t *next;              // read by k_fill_count, then updated
    const uint64_t *last_acked;
    const uint32_t *budget;      // nullable: max_frames
    uint32_t n_files;
    uint32_t max_frames;         // > 0
    uint64_t mtu;                // 21 .. 65547
    const uint64_t *stream_off;
    const uint64_t *stream_cap;
    uint64_t *stream_len;        // nullable
    uint32_t *nframes;           // nullable
    uint32_t *first;             // n_files + 1, written by k_scan_first
    uint64_t *frame_off;         // n_files * max_frames, absolute in the output
    // workspace: k_pack's inputs (n_files * max_frames entries), per transfer the count and the old next
    uint64_t *wpay_off;
    uint64_t *wfile_off;
    uint32_t *wpay_len;
    uint8_t *wexpl;
    uint64_t *wnext;
    uint32_t *wcnt;
};

constexpr uint64_t kFillNoExplicit = ~(uint64_t)0;

// Index of the explicit frame of a transfer at `next`: the frame that starts at
// last_acked, if the frame starts next + j * M reach it.
__device__ __forceinline__ uint64_t fill_explicit(uint64_t next, uint64_t last_acked, uint64_t M)
{
    if (last_acked < next) return kFillNoExplicit;
    const uint64_t d = last_acked - next;
    return d % M == 0u ? d / M : kFillNoExplicit;
}

// Payload bytes the frames in front of frame j hold when none of them ends the file.
__device__ __forceinline__ uint64_t fill_before(uint64_t j, uint64_t je, uint64_t M)
{
    return j * M - (j > je ? 8u : 0u);
}

__global__ __launch_bounds__(kFillBlock) void k_fill_count(const FillParams p)
{
    const uint64_t s = (uint64_t)blockIdx.x * kFillBlock + threadIdx.x;
    if (s >= p.n_files) return;
    const uint64_t next = p.next[s], size = p.file_size[s], cap = p.stream_cap[s];
    const uint64_t M = p.mtu - (VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE);
    const uint32_t budget = p.budget ? min(p.budget[s], p.max_frames) : p.max_frames;
    const uint64_t je = fill_explicit(next, p.last_acked[s], M);
    uint32_t cnt = 0;
    uint64_t used = 0, nnext = next;
    if (budget && next < size) {
        const uint64_t rem = size - next;
        // frames to the end of the file: the explicit one counts when the file goes on behind its start
        const bool with = je != kFillNoExplicit && rem / M >= je && rem > je * M;
        const uint64_t q = rem / M, r = rem % M;
        const uint64_t F = with ? q + (r + 8u + M - 1u) / M : q + (r ? 1u : 0u);
        const uint64_t lastpay = rem - fill_before(F - 1u, je, M);  // 1 .. M
        const uint64_t lastwire = VAL_WIRE_HEADER_SIZE + lastpay + (F - 1u == je ? 8u : 0u) + VAL_WIRE_TRAILER_SIZE;
        const uint64_t want = min(F, (uint64_t)budget);
        const uint64_t whole = cap / p.mtu;  // frames of wire size mtu that fit
        uint64_t k;
        if (whole >= want) k = want;  // frame j ends at or before (j + 1) * mtu
        else k = whole + ((whole == F - 1u && lastwire <= cap - whole * p.mtu) ? 1u : 0u);
        cnt = (uint32_t)k;  // <= budget
        if (k == F) {
            used = (k - 1u) * p.mtu + lastwire;
            nnext = size;
        } else if (k) {
            used = k * p.mtu;
            nnext = next + fill_before(k, je, M);  // the start of frame k, inside the file
        }
    }
    p.wcnt[s] = cnt;
    p.wnext[s] = next;
    p.next[s] = nnext;
    if (p.nframes) p.nframes[s] = cnt;
    if (p.stream_len) p.stream_len[s] = used;
}

// Every entry of the workspace arrays and of frame_off is written exactly once:
// entries below the total by the slot that owns them, the others as padding.
__global__ __launch_bounds__(kFillBlock) void k_fill_desc(const FillParams p)
{
    const uint64_t slots = (uint64_t)p.n_files * p.max_frames;
    const uint32_t total = p.first[p.n_files];
    const uint64_t M = p.mtu - (VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE);
    const uint64_t stride = (uint64_t)gridDim.x * kFillBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kFillBlock + threadIdx.x; e < slots; e += stride) {
        const uint32_t s = (uint32_t)e / p.max_frames, j = (uint32_t)e - s * p.max_frames;  // slots < 2^32
        if (j < p.wcnt[s]) {
            const uint32_t d = p.first[s] + j;
            const uint64_t next = p.wnext[s];
            const uint64_t je = fill_explicit(next, p.last_acked[s], M);
            const uint64_t foff = next + fill_before(j, je, M);  // < file_size
            const uint64_t room = j == je ? M - 8u : M;
            p.wpay_off[d] = p.file_pos[s] + foff;  // wraps by definition
            p.wfile_off[d] = foff;
            p.wpay_len[d] = (uint32_t)min(p.file_size[s] - foff, room);
            p.wexpl[d] = (uint8_t)(j == je);
            p.frame_off[d] = p.stream_off[s] + (uint64_t)j * p.mtu;
        }
        if (e >= total) {
            p.wpay_off[e] = 0u;
            p.wfile_off[e] = 0u;
            p.wpay_len[e] = kFillReject;
            p.wexpl[e] = 0u;
            p.frame_off[e] = 0u;
        }
    }
}

}  // namespace vcrc
