// ack_kernel.hpp -- the kernels behind val_frame_respond_files_dev and
// val_frame_apply_acks_files_dev (gfx950): the receiver's DATA_ACK / DATA_NAK
// answers to a delivered window, and the sender's handling of such answers.
// Included by val_crc32_hip.hip. DESIGN.md section 4.13.
//
// Respond, after val_frame_unpack_files_dev on the same stream:
//   k_unpack_parse<false>  grid-wide, one frame per thread: the header facts
//                          (unpack_kernel.hpp) into the workspace;
//   k_ack_respond_files    the rule of val_frame_respond_window (val_wire.h)
//                          as segmented scans: workgroups take whole files in
//                          turn, 1,024 or 256 frames per chunk (k_unpack_order_files'
//                          layout), and leave per frame the offset its
//                          responses carry and where they go;
//   k_ack_emit             grid-wide, one frame per thread: the response
//                          frames with their trailers, written where planned.
// Apply, after the verify launches over the response window:
//   k_ack_apply_files      the rule of val_frame_apply_acks as a reduction
//                          (a maximum and an "any restart") per transfer, in
//                          the same layout.
//
// None of these kernels touches the LDS table image of crc_device.hpp.
#pragma once

#include "crc_device.hpp"
#include "unpack_kernel.hpp"
#include "val_wire.h"

namespace vcrc {

constexpr int kAckBlock = kOrderBlock;  // k_ack_respond_files, k_ack_apply_files: one frame per thread and chunk
// Calls whose files own 256 frames or fewer on average run k_ack_respond_files in workgroups of 256
// threads, up to 8 per CU: a small file is a chain of a few memory round trips and barriers, and
// eight of them in flight per CU hide each other's waits where one workgroup of 1,024 threads waits
// alone. Results do not depend on it.
constexpr int kAckSmallBlock = 256;
constexpr int kAckSmallFrames = 256;
constexpr int kAckSmallPerCU = 8;
constexpr int kAckEmitBlock = 256;      // k_ack_emit

// What k_ack_respond_files leaves per frame for k_ack_emit, in one word so
// that a frame two overlapping segments own (the caller's error) still gets a
// position and sizes that belong together: the position of its first response
// in d_out (bits 0..60) and which responses are written.
constexpr uint64_t kAckPosMask = ((uint64_t)1 << 61) - 1u;
constexpr uint64_t kAckKeepAck = (uint64_t)1 << 61;
constexpr uint64_t kAckKeepNak = (uint64_t)1 << 62;
constexpr uint64_t kAckWide = (uint64_t)1 << 63;  // the ACK carries the high half: 16 wire bytes
constexpr uint32_t kAckSize = VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE;
constexpr uint32_t kNakSize = VAL_WIRE_RESPONSE_MAX;

struct AckRespondParams {
    uint32_t n, n_files;
    const uint32_t *first;  // n_files + 1 frame indices
    const uint8_t *accept;  // the unpack call's
    // workspace: k_unpack_parse's header facts (a frame with ok[i] == 0 is NOT_DATA)
    const uint64_t *foff;
    const uint32_t *plen;
    const uint64_t *written;  // after delivery
    const uint64_t *total;
    uint32_t ack_stride;
    uint32_t *since;  // in/out; unused with ack_stride == 0
    uint8_t *out;
    const uint64_t *resp_off, *resp_cap;
    uint64_t *resp_len;
    uint32_t *nresp;
    uint32_t *ndropped;  // nullable, incremented
    // workspace: per frame the offset its responses carry, and kAck* above
    uint64_t *woff, *wmeta;
};

struct AckApplyParams {
    const uint8_t *base;
    const uint64_t *off;  // NULL: strided mode
    const uint32_t *len;
    uint64_t stride;
    uint32_t flen;
    uint32_t n, n_files;
    const uint32_t *first;
    const uint8_t *ok;  // verify's verdicts
    const uint64_t *file_size;
    uint64_t *last_acked, *next;  // in/out
    uint32_t *nretrans;           // nullable, incremented
    uint32_t *file_nbad;          // nullable, incremented
};

// Exclusive scan of `mine` over the workgroup (one barrier); *total = the
// workgroup's sum. The caller alternates `wsum` between two buffers, so that
// the next scan's writes cannot overtake this scan's reads.
template <int BLOCK>
__device__ __forceinline__ uint64_t ack_scan(uint64_t mine, uint64_t *wsum, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(incl, d);
        if ((int)lane >= d) incl += o;
    }
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint64_t wbase = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; w++) {
        const uint64_t v = wsum[w];
        if (w < wave) wbase += v;
        tot += v;
    }
    *total = tot;
    return wbase + incl - mine;
}

__device__ __forceinline__ uint64_t ack_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ uint64_t ack_wave_max(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

template <int BLOCK>
struct AckShared {
    uint64_t wsum[2][BLOCK / 64];
    unsigned long long pay, bytes;
    uint32_t last, kept, drop;
};

// ---- respond ---------------------------------------------------------------
// One file's rule without a walk. The unpack call left which frames it
// accepted and the position after them, W_end; the position in front of frame
// i is W_end minus the payload bytes of the accepted frames from i on, i.e.
// W_end - (all accepted bytes) + (an exclusive scan of them). With that
// position every frame classifies itself: accepted (ACK by the stride rule),
// capacity refusal (explicit offset == position, or implied, and not accepted:
// silent), duplicate (offset below: ACK), gap (offset above: NAK, ACK).
// The stride rule in closed form: with s0 = since on entry and k the stride,
// the j-th accepted frame (j = 1, 2, ...) that does not complete the file
// emits iff j >= j1 and (j - j1) % k == 0, j1 = s0 >= k ? 1 : k - s0; from the
// first frame that reaches `total` on every accepted frame emits (W only
// grows) and since is 0. With k == 0 the emitting frames are those that reach
// `total` and the file's last accepted frame of the call.
// Pass 1 sums the accepted bytes and finds the last accepted frame; pass 2
// scans, per chunk, the accepted bytes with the accepted count beside them (one
// scan: the bytes of a chunk stay below 2^42, the count sits in bits 48 up)
// and then the response sizes.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_ack_respond_files(const AckRespondParams p)
{
    __shared__ AckShared<BLOCK> sh;
    constexpr uint64_t kLow48 = ((uint64_t)1 << 48) - 1u;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t == 0) sh.pay = 0, sh.bytes = 0, sh.last = 0, sh.kept = 0, sh.drop = 0;
    __syncthreads();
    for (uint64_t s = blockIdx.x; s < p.n_files; s += gridDim.x) {
        const uint32_t a = p.first[s], b = p.first[s + 1];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(a, p.n));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(max(a, b), p.n));
        if (lo >= hi) {  // no frames: no responses, since[] keeps its value
            if (t == 0) p.resp_len[s] = 0u, p.nresp[s] = 0u;
            continue;
        }
        const uint64_t w_end = order_uniform(p.written[s]), total = order_uniform(p.total[s]);
        const uint64_t roff = order_uniform(p.resp_off[s]);
        // an offset no buffer has leaves no room for the flag bits: nothing is written
        const uint64_t cap = (roff >> 60) ? 0u : order_uniform(p.resp_cap[s]);
        const uint32_t k = p.ack_stride;
        const uint32_t s0 = k ? (uint32_t)__builtin_amdgcn_readfirstlane((int)p.since[s]) : 0u;
        const uint64_t j1 = s0 >= k ? 1u : (uint64_t)(k - s0);
        // the file's first chunk stays in registers for both passes; pass 2 loads the next chunk
        // while it scans this one
        uint64_t fo_n = VAL_FRAME_OFFSET_NOT_DATA;
        uint32_t pl_n = 0;
        bool acc_n = false;
        if ((uint64_t)lo + t < hi) {
            fo_n = p.foff[lo + t];
            pl_n = p.plen[lo + t];
            acc_n = p.accept[lo + t] != 0 && fo_n != VAL_FRAME_OFFSET_NOT_DATA;
        }
        // pass 1
        uint64_t pay = acc_n ? pl_n : 0u;
        uint32_t last = acc_n ? t + 1u : 0u;  // 1 + the frame's index in the file; 0 = none
        // (every load unconditional, four chunks per step: the loop is a reduction, and a load that
        // waits for a verdict would make it a chain of round trips)
        for (uint64_t i0 = (uint64_t)lo + BLOCK + t; i0 < hi; i0 += 4u * BLOCK) {
            uint8_t av[4];
            uint64_t fv[4];
            uint32_t pv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t i = i0 + (uint64_t)u * BLOCK;
                const uint64_t at = i < hi ? i : i0;  // a frame of the file either way
                av[u] = p.accept[at];
                fv[u] = p.foff[at];
                pv[u] = p.plen[at];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t i = i0 + (uint64_t)u * BLOCK;
                if (i < hi && av[u] && fv[u] != VAL_FRAME_OFFSET_NOT_DATA) {
                    pay += pv[u];
                    last = (uint32_t)(i - lo) + 1u;
                }
            }
        }
        pay = ack_wave_sum(pay);
        last = (uint32_t)ack_wave_max(last);
        if (lane == 0) {
            if (pay) atomicAdd(&sh.pay, (unsigned long long)pay);
            if (last) atomicMax(&sh.last, last);
        }
        __syncthreads();
        const uint64_t w_start = w_end - sh.pay;
        const uint32_t last_acc = sh.last;
        // pass 2
        uint64_t w_run = w_start, j_run = 0, p_run = 0, bytes = 0;
        uint32_t kept = 0, drop = 0;
        for (uint64_t c0 = lo; c0 < hi; c0 += BLOCK) {
            const uint64_t i = c0 + t;
            const bool valid = i < hi;
            const uint64_t fo = fo_n;
            const uint32_t pl = pl_n;
            const bool acc = acc_n;
            fo_n = VAL_FRAME_OFFSET_NOT_DATA, pl_n = 0, acc_n = false;
            if (i + BLOCK < hi) {
                fo_n = p.foff[i + BLOCK];
                pl_n = p.plen[i + BLOCK];
                acc_n = p.accept[i + BLOCK] != 0 && fo_n != VAL_FRAME_OFFSET_NOT_DATA;
            }
            uint64_t tot1 = 0, tot2 = 0;
            const uint64_t ex = ack_scan<BLOCK>(acc ? ((uint64_t)pl | ((uint64_t)1 << 48)) : 0u, sh.wsum[0], &tot1);
            const uint64_t w_front = w_run + (ex & kLow48);
            const uint64_t j = j_run + (ex >> 48) + 1u;
            uint64_t w = w_front;
            bool ack = false, nak = false;
            if (fo != VAL_FRAME_OFFSET_NOT_DATA) {
                if (acc) {
                    w = w_front + pl;
                    if (w >= total) ack = true;
                    else if (k == 0) ack = (uint32_t)(i - lo) + 1u == last_acc;
                    else ack = j >= j1 && (uint32_t)(j - j1) % k == 0;  // j <= n: the difference has 32 bits
                } else if (fo == VAL_FRAME_OFFSET_IMPLIED || fo == w_front) {
                    // refused by capacity alone: silent
                } else if (fo < w_front) {
                    ack = true;
                } else {
                    ack = nak = true;
                }
            }
            const uint32_t asz = (w >> 32) ? kAckSize + 4u : kAckSize;
            const uint64_t pos = p_run + ack_scan<BLOCK>((nak ? kNakSize : 0u) + (ack ? asz : 0u), sh.wsum[1], &tot2);
            uint64_t meta = 0;
            if (nak) {
                if (pos + kNakSize <= cap) meta |= kAckKeepNak, kept++, bytes += kNakSize;
                else drop++;
            }
            if (ack) {
                if (pos + (nak ? kNakSize : 0u) + asz <= cap) {
                    meta |= kAckKeepAck | (asz != kAckSize ? kAckWide : 0u);
                    kept++, bytes += asz;
                } else {
                    drop++;
                }
            }
            if (meta) meta |= roff + pos;  // below 2^61: roff < 2^60, pos <= 40 * 2^32
            if (valid) {
                p.woff[i] = w;
                p.wmeta[i] = meta;
            }
            w_run += tot1 & kLow48;
            j_run += tot1 >> 48;
            p_run += tot2;
        }
        bytes = ack_wave_sum(bytes);
        kept = (uint32_t)ack_wave_sum(kept);
        drop = (uint32_t)ack_wave_sum(drop);
        if (lane == 0) {
            if (bytes) atomicAdd(&sh.bytes, (unsigned long long)bytes);
            if (kept) atomicAdd(&sh.kept, kept);
            if (drop) atomicAdd(&sh.drop, drop);
        }
        __syncthreads();
        if (t == 0) {
            p.resp_len[s] = sh.bytes;
            p.nresp[s] = sh.kept;
            if (p.ndropped && sh.drop) atomicAdd(p.ndropped + s, sh.drop);
            if (k) {
                const uint64_t m = j_run;  // the frames accepted
                uint32_t since = s0;
                if (m && w_end >= total) since = 0u;
                else if (m && m < j1) since = s0 + (uint32_t)m;  // below k
                else if (m) since = (uint32_t)(m - j1) % k;
                p.since[s] = since;
            }
            sh.pay = 0, sh.bytes = 0, sh.last = 0, sh.kept = 0, sh.drop = 0;
        }
        __syncthreads();  // the cleared sums, before the next file adds to them
    }
}

// CRC-32 (the trailer value) of nw little-endian dwords, bit by bit: 8, 12 or
// 20 bytes per response, in registers; no table, no LDS.
template <int NW>
__device__ __forceinline__ uint32_t ack_crc(const uint32_t (&w)[NW])
{
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        c ^= w[i];
        for (int b = 0; b < 32; b++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

// NW dwords to out + pos: dword stores where the address allows, else bytes.
template <int NW>
__device__ __forceinline__ void ack_store(uint8_t *out, uint64_t pos, const uint32_t (&w)[NW])
{
    const uint64_t at = (uint64_t)(uintptr_t)out + pos;
    if ((at & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) *reinterpret_cast<uw32 *>(at + 4u * i) = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++)
#pragma unroll
            for (int b = 0; b < 4; b++) *reinterpret_cast<uw8 *>(at + 4u * i + b) = (uint8_t)(w[i] >> (8 * b));
    }
}

// The wire bytes of frame i's kept responses (reference src/val_core.c:775-811
// with the trailer of :828-834), as val_frame_put_response lays them out.
__global__ __launch_bounds__(kAckEmitBlock) void k_ack_emit(const AckRespondParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * kAckEmitBlock + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t meta = p.wmeta[i];
    if (!(meta & (kAckKeepAck | kAckKeepNak))) return;
    const uint64_t w = p.woff[i];
    const uint32_t low = (uint32_t)w, high = (uint32_t)(w >> 32);
    uint64_t pos = meta & kAckPosMask;
    if (meta & kAckKeepNak) {
        uint32_t f[6] = {(uint32_t)VAL_PKT_DATA_NAK | (12u << 16), low, high, VAL_NAK_REASON_GAP, 0u, 0u};
        const uint32_t in[5] = {f[0], f[1], f[2], f[3], f[4]};
        f[5] = ack_crc<5>(in);
        ack_store<6>(p.out, pos, f);
        pos += kNakSize;
    }
    if (meta & kAckKeepAck) {
        if (meta & kAckWide) {
            uint32_t f[4] = {(uint32_t)VAL_PKT_DATA_ACK | (4u << 16), low, high, 0u};
            const uint32_t in[3] = {f[0], f[1], f[2]};
            f[3] = ack_crc<3>(in);
            ack_store<4>(p.out, pos, f);
        } else {
            uint32_t f[3] = {(uint32_t)VAL_PKT_DATA_ACK, low, 0u};
            const uint32_t in[2] = {f[0], f[1]};
            f[2] = ack_crc<2>(in);
            ack_store<3>(p.out, pos, f);
        }
    }
}

// ---- apply -----------------------------------------------------------------
// val_frame_apply_acks in closed form. last_acked only grows, to the largest
// offset of a good ACK or NAK that does not pass the file's size; a restart
// (a corrupt frame or a NAK) puts next at the last_acked of its moment, which
// the rule's last step then raises to the final one; without a restart next
// is max(next, last_acked). So a transfer needs a maximum, an "any restart"
// and two counts over its frames: per-thread over the chunks, then one
// reduction. Of a frame the first two header dwords are read, and the dword
// at +8 when it belongs to the CRC input.
__global__ __launch_bounds__(kAckBlock) void k_ack_apply_files(const AckApplyParams p)
{
    __shared__ unsigned long long s_max;
    __shared__ uint32_t s_restart, s_retr, s_bad;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t == 0) s_max = 0, s_restart = 0, s_retr = 0, s_bad = 0;
    __syncthreads();
    for (uint64_t s = blockIdx.x; s < p.n_files; s += gridDim.x) {
        const uint32_t a = p.first[s], b = p.first[s + 1];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(a, p.n));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(max(a, b), p.n));
        if (lo >= hi) continue;  // no frames: the transfer's entries keep their values
        const uint64_t fsz = order_uniform(p.file_size[s]);
        uint64_t mx = 0;
        uint32_t restart = 0, retr = 0, bad = 0;
        for (uint64_t i = (uint64_t)lo + t; i < hi; i += kAckBlock) {
            if (!p.ok[i]) {
                restart = 1u, retr++, bad++;
                continue;
            }
            const uint32_t L = p.len ? p.len[i] : p.flen;
            if (L < VAL_WIRE_HEADER_SIZE) continue;
            gu8 *f = gptr(p.base) + (p.off ? p.off[i] : i * p.stride);
            const uint32_t type = ld32(f) & 0xFFu;
            if (type != (uint32_t)VAL_PKT_DATA_ACK && type != (uint32_t)VAL_PKT_DATA_NAK) continue;
            uint64_t o = ld32(f + 4);
            if (L >= VAL_WIRE_HEADER_SIZE + 4u) o |= (uint64_t)ld32(f + 8) << 32;
            if (o <= fsz && o > mx) mx = o;
            if (type == (uint32_t)VAL_PKT_DATA_NAK) restart = 1u, retr++;
        }
        mx = ack_wave_max(mx);
        const bool any = __ballot(restart != 0) != 0;
        retr = (uint32_t)ack_wave_sum(retr);
        bad = (uint32_t)ack_wave_sum(bad);
        if (lane == 0) {
            if (mx) atomicMax(&s_max, (unsigned long long)mx);
            if (any) atomicOr(&s_restart, 1u);
            if (retr) atomicAdd(&s_retr, retr);
            if (bad) atomicAdd(&s_bad, bad);
        }
        __syncthreads();
        if (t == 0) {
            const uint64_t la0 = p.last_acked[s], nx0 = p.next[s];
            const uint64_t la = la0 > s_max ? la0 : (uint64_t)s_max;
            p.last_acked[s] = la;
            p.next[s] = s_restart ? la : (nx0 > la ? nx0 : la);
            if (p.nretrans && s_retr) atomicAdd(p.nretrans + s, s_retr);
            if (p.file_nbad && s_bad) atomicAdd(p.file_nbad + s, s_bad);
            s_max = 0, s_restart = 0, s_retr = 0, s_bad = 0;
        }
        __syncthreads();  // the cleared results, before the next transfer adds to them
    }
}

}  // namespace vcrc
