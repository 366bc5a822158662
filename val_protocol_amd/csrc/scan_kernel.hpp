// scan_kernel.hpp -- the kernels behind val_frame_scan_streams_dev (gfx950):
// received byte streams in HBM walked into frame descriptors, the device form
// of val_frame_scan (csrc/val_wire.c). Included by val_crc32_hip.hip.
//
// A frame starts where the one before it ended, and where that ended is the
// LE16 content_len in its header: the walk is a chain of dependent loads, one
// memory round trip per frame if taken literally. Real windows are runs of
// equal-size frames, so the walk predicts the run and checks the prediction
// (DESIGN.md section 4.10):
//   k_scan_streams  one front of lanes per stream: a wave, or for calls with
//                   few streams a workgroup of 16 waves. With the wire size P
//                   of the last frame, lane j looks at pos + j * P; the
//                   leading run of lanes that hold a complete frame of size P
//                   is emitted in one step, and the first lane that does not
//                   is a true frame start, judged by the host's rule.
//   k_scan_first    one workgroup: d_first = exclusive scan of the counts.
//   k_scan_compact  grid-wide: every stream's slot of the workspace copied to
//                   its place behind the streams before it, the tail padded
//                   with (0, 0).
// No kernel here uses an LDS table: the wide front holds 64 dwords of LDS for
// its waves' ballots, k_scan_first 16 for its waves' sums.
#pragma once

#include "crc_device.hpp"
#include "val_errors.h"
#include "val_wire.h"

namespace vcrc {

constexpr int kScanBlock = 256;       // threads per workgroup (4 waves), one-wave walk and compact
constexpr int kScanBlocksPerCU = 8;   // persistent grids: under 64 VGPRs
constexpr int kScanWideWaves = 16;    // the wide front: one workgroup of 1,024 lanes per stream
constexpr int kScanFirstBlock = 1024; // k_scan_first: one count per thread and chunk

struct ScanParams {
    const uint8_t *base;
    const uint64_t *stream_off;
    const uint64_t *stream_len;
    uint32_t n_streams;
    uint32_t max_frames;   // per stream, > 0
    uint64_t max_content;  // mtu - 12
    // workspace: stream s owns entries [s * max_frames, (s + 1) * max_frames)
    uint64_t *woff;        // absolute frame offsets
    uint32_t *wlen;
    uint32_t *wcnt;        // n_streams counts
    // results
    uint64_t *frame_off;
    uint32_t *crc_len;
    uint32_t *first;       // n_streams + 1
    uint32_t *nframes;     // nullable
    uint64_t *consumed;    // nullable
    int32_t *status;       // nullable
};

typedef uint32_t __attribute__((address_space(1))) sw32;
typedef uint64_t __attribute__((address_space(1))) sw64;

__device__ __forceinline__ uint32_t scan_uniform(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint64_t scan_uniform(uint64_t v)
{
    return (uint64_t)scan_uniform((uint32_t)v) | ((uint64_t)scan_uniform((uint32_t)(v >> 32)) << 32);
}

// The LE16 content_len whose first byte is at address a (header bytes 2..3,
// both inside the stream): the aligned dword that holds it, and the next one
// only when the two bytes straddle it. Both overlap the stream.
__device__ __forceinline__ uint32_t scan_content(uint64_t a)
{
    const uint64_t a0 = a & ~(uint64_t)3;
    const uint32_t m = (uint32_t)(a & 3u);
    const uint32_t w0 = *reinterpret_cast<gu32 *>(a0);
    uint32_t w1 = 0;
    if (m == 3u) w1 = *reinterpret_cast<gu32 *>(a0 + 4u);
    return __builtin_amdgcn_alignbyte(w1, w0, m) & 0xFFFFu;
}

// ---- the walk ----------------------------------------------------------------
// val_frame_scan over stream s by one front: the 64 lanes of a wave (WAVES = 1;
// a workgroup is four independent fronts), or the 64 * WAVES lanes of a whole
// workgroup. pos, k and P are uniform over the front; the loop condition is
// the host's, so pos is a true frame start whose header fits whenever a round
// begins. A round:
//   lane j loads the content_len at q = pos + j * P if a header fits there;
//   it matches iff that frame is legal, complete and of wire size P;
//   m = the leading run of matching lanes; frames k .. k + m - 1 (as far as
//   max_frames allows) are the lanes' and are emitted;
//   lane m, if the front has one, then sits on a true frame start, since every
//   frame before it had the predicted size: it stops the stream by the host's
//   rule, or its frame is emitted and its size becomes the prediction.
// Only the leading run counts: a lane behind the first mismatch may be looking
// into a payload that reads as a matching header. P starts at 0, which no
// frame matches: the first round is lane 0's alone.
// Equal-size runs advance a front of frames per memory round trip; sizes that
// alternate advance one frame per round trip, whatever the width.
// A front of several waves does not look with all its lanes at once: loads
// that a mismatch makes useless cost their round trip all the same (1,024
// scattered lines take four times as long as 64). One wave looks first, and
// every round in which all lanes that looked matched widens the next one
// fourfold, up to the whole front; a mismatch brings it back to one wave. A
// wave that does not look reports a mismatch at its lane 0, so m never
// passes the lanes that looked.
// A front of several waves finds m through LDS: every wave leaves its own
// first mismatch and that lane's content_len in this round's slot (two slots
// in turn, so one barrier per round: a wave that is a round ahead writes the
// other slot, and cannot be two ahead without everyone passing the barrier in
// between), and all read the first wave that has one.
template <int WAVES>
__global__ __launch_bounds__(WAVES == 1 ? kScanBlock : 64 * WAVES) void k_scan_streams(const ScanParams p)
{
    constexpr uint32_t kFront = 64u * WAVES;
    __shared__ uint2 slot[2][WAVES];  // WAVES > 1 only
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = WAVES == 1 ? 0u : scan_uniform(threadIdx.x >> 6);
    const uint32_t j = wv * 64u + lane;  // lane of the front
    const uint32_t front = WAVES == 1 ? scan_uniform((uint32_t)(((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6))
                                      : blockIdx.x;
    const uint32_t nfronts = WAVES == 1 ? (uint32_t)(((uint64_t)gridDim.x * kScanBlock) >> 6) : gridDim.x;
    sw64 *woff = (sw64 *)p.woff;
    sw32 *wlen = (sw32 *)p.wlen;
    uint32_t flip = 0;
    for (uint64_t s = front; s < p.n_streams; s += nfronts) {
        const uint64_t soff = scan_uniform(p.stream_off[s]);
        const uint64_t len = scan_uniform(p.stream_len[s]);
        const uint64_t src = (uint64_t)(uintptr_t)p.base + soff;  // address of stream byte 0
        const uint64_t slot0 = s * p.max_frames;
        uint64_t pos = 0;
        uint32_t k = 0, P = 0;
        uint32_t act = 64u;  // lanes of the front that look this round (WAVES > 1), whole waves
        int32_t st = VAL_OK;
        while (k < p.max_frames && len - pos >= VAL_WIRE_HEADER_SIZE) {
            const uint64_t q = pos + (uint64_t)j * P;
            const bool fits = j < act && q <= len && len - q >= VAL_WIRE_HEADER_SIZE;
            uint32_t c = 0;
            if (fits) c = scan_content(src + q + 2u);
            const uint32_t wire = VAL_WIRE_HEADER_SIZE + c + VAL_WIRE_TRAILER_SIZE;
            const bool match = fits && (uint64_t)c <= p.max_content && len - q >= (uint64_t)wire && wire == P;
            const uint64_t miss = ~__ballot(match);
            uint32_t m = miss ? (uint32_t)__builtin_ctzll(miss) : 64u;
            uint32_t cm = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)(m & 63u));
            if (WAVES > 1) {
                if (lane == 0) slot[flip][wv] = make_uint2(m, cm);
                __syncthreads();
                // lane w holds wave w's pair: one LDS read, a ballot and two lane reads
                const uint2 x = slot[flip][lane % WAVES];
                const uint32_t has = (uint32_t)__ballot(x.x < 64u) & ((1u << WAVES) - 1u);
                const uint32_t fw = has ? (uint32_t)__builtin_ctz(has) : 0u;
                m = has ? fw * 64u + (uint32_t)__builtin_amdgcn_readlane((int)x.x, (int)fw) : kFront;
                cm = (uint32_t)__builtin_amdgcn_readlane((int)x.y, (int)fw);
                flip ^= 1u;
            }
            const uint32_t e = min(m, p.max_frames - k);
            if (j < e) {
                woff[slot0 + k + j] = soff + q;
                wlen[slot0 + k + j] = VAL_WIRE_HEADER_SIZE + c;
            }
            k += e;
            pos += (uint64_t)e * P;
            // every lane that looked matched: there is no lane m, the next round looks further
            const bool all = m == (WAVES == 1 ? 64u : act);
            if (WAVES > 1) act = all ? min(act * 4u, kFront) : 64u;
            if (all || k == p.max_frames) continue;
            // lane m's position, now pos: the host's rule, in the host's order
            if (len - pos < VAL_WIRE_HEADER_SIZE) break;
            if ((uint64_t)cm > p.max_content) {
                st = VAL_ERR_PROTOCOL;
                break;
            }
            const uint32_t wm = VAL_WIRE_HEADER_SIZE + cm + VAL_WIRE_TRAILER_SIZE;
            if (len - pos < (uint64_t)wm) break;  // incomplete: wait for more bytes
            if (j == 0) {
                woff[slot0 + k] = soff + pos;
                wlen[slot0 + k] = VAL_WIRE_HEADER_SIZE + cm;
            }
            k++;
            pos += wm;
            P = wm;
        }
        if (j == 0) {
            p.wcnt[s] = k;
            if (p.nframes) p.nframes[s] = k;
            if (p.consumed) p.consumed[s] = pos;
            if (p.status) p.status[s] = st;
        }
    }
}

// ---- d_first -----------------------------------------------------------------
// Exclusive scan of the n_streams counts by one workgroup, in chunks of one
// count per thread; first[n_streams] = the total (below 2^32: the call refuses
// n_streams * max_frames beyond that).
__global__ __launch_bounds__(kScanFirstBlock) void k_scan_first(const ScanParams p)
{
    constexpr uint32_t kWaves = kScanFirstBlock / 64;
    __shared__ uint32_t wsum[kWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t carry = 0;
    for (uint64_t c0 = 0; c0 < p.n_streams; c0 += kScanFirstBlock) {
        const uint64_t i = c0 + t;
        const uint32_t v = i < p.n_streams ? p.wcnt[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if ((int)lane >= d) incl += o;
        }
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t x = wsum[w];
            if (w < wave) wbase += x;
            total += x;
        }
        if (i < p.n_streams) p.first[i] = carry + wbase + incl - v;
        carry += total;
        __syncthreads();  // the next chunk overwrites wsum
    }
    if (t == 0) p.first[p.n_streams] = carry;
}

// ---- compaction --------------------------------------------------------------
// Entry e of the n_streams * max_frames: as entry j of stream s's slot it moves
// to first[s] + j when the walk filled it, and as an output entry at or behind
// the total it becomes (0, 0). Every output entry is written exactly once.
__global__ __launch_bounds__(kScanBlock) void k_scan_compact(const ScanParams p)
{
    const uint64_t slots = (uint64_t)p.n_streams * p.max_frames;
    const uint32_t total = p.first[p.n_streams];
    const uint64_t stride = (uint64_t)gridDim.x * kScanBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x; e < slots; e += stride) {
        const uint32_t s = (uint32_t)e / p.max_frames, j = (uint32_t)e - s * p.max_frames;  // slots < 2^32
        if (j < p.wcnt[s]) {
            const uint32_t d = p.first[s] + j;
            p.frame_off[d] = p.woff[e];
            p.crc_len[d] = p.wlen[e];
        }
        if (e >= total) {
            p.frame_off[e] = 0u;
            p.crc_len[e] = 0u;
        }
    }
}

}  // namespace vcrc
