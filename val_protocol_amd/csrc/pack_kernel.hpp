// pack_kernel.hpp -- k_pack<G>: build DATA frames in HBM and hash them in the
// same pass (gfx950). Included by val_crc32_hip.hip.
//
// The device form of val_frame_data_batch + the trailer CRC +
// val_frame_put_trailers (reference src/val_core.c:733-834 per packet): every
// payload byte is read once, hashed while it sits in registers and written
// once. The frame algorithm is hash_frame's (crc_kernels.hpp): G lanes per
// frame, 64-B units counted from the frame end, a gap step between a lane's
// units, a __shfl_xor merge tree. What differs is where a unit's words come
// from and where they go:
//   * The unit grid is anchored on the DESTINATION: it ends at floor4 of the
//     frame's end address in the output, so every unit is dword-aligned there
//     and a whole unit leaves as four dwordx4 stores.
//   * A unit's words are assembled in registers. Frame byte q >= prefix (8, or
//     16 with the LE64 offset) is payload byte q - prefix; against the
//     destination grid that source address is off by a per-frame constant
//     m = 0..3 bytes, so the unit reads the 16 (m = 0) or 17 covering aligned
//     source dwords and funnel-shifts neighbours by m (v_alignbyte_b32). The
//     header and offset words are synthesised by whichever lane holds them.
//   * Only aligned dwords that overlap the frame's payload range are read, and
//     only the frame's own 12 + content wire bytes are written: the first
//     partial dword, the <= 3 bytes past the grid and the trailer go out as
//     byte stores.
// Persistent grid, plain static deal of frame groups (64 / G frames per wave
// and step), one round of source dwords in flight ahead of the one being
// hashed. No dynamic queue, tail pieces or binning: the kernel needs no
// scratch.
#pragma once

#include "crc_device.hpp"
#include "val_wire.h"

namespace vcrc {

struct PackParams {
    const uint8_t *payload;
    const uint64_t *pay_off;
    const uint32_t *pay_len;
    const uint64_t *file_off;
    const uint8_t *include_offset;  // NULL: every frame carries its offset
    uint32_t n;
    uint8_t *out;
    const uint64_t *frame_off;      // NULL: frame i at i * stride
    uint64_t stride;
    uint32_t *out_len;              // nullable: 8 + content
    uint32_t *out_crc;              // nullable: trailer value
    uint32_t *out_hdr;              // nullable: header_crc
    uint32_t *nrejected;            // nullable, incremented
    const uint32_t *consts;
};

typedef uint32_t __attribute__((address_space(1))) gw32;
typedef u32x4u __attribute__((address_space(1))) gw32x4u;
typedef uint8_t __attribute__((address_space(1))) gw8;

// One frame as a lane sees it. srcb is the (virtual) source address of frame
// byte 0: payload byte j sits at srcb + prefix + j. Addresses are integers:
// srcb itself may lie before the payload buffer and is never dereferenced.
struct PackFrame {
    uint64_t dst;      // address of frame byte 0 in the output
    uint64_t srcb;     // payload start - prefix
    uint64_t pstart, pend;  // the payload range [pstart, pend)
    uint32_t h[4];     // prefix words: header (2), LE64 file offset (2, explicit frames)
    uint32_t prefix;   // 8 or 16
    uint32_t L;        // CRC input: prefix + payload
};

// Prefix word j (frame bytes 4j..4j+3); zero outside the prefix.
__device__ __forceinline__ uint32_t pack_pword(const PackFrame &d, int j)
{
    uint32_t v = 0;
    v = j == 0 ? d.h[0] : v;
    v = j == 1 ? d.h[1] : v;
    v = (j == 2 && d.prefix == 16u) ? d.h[2] : v;
    v = (j == 3 && d.prefix == 16u) ? d.h[3] : v;
    return v;
}

// The 17 aligned source dwords covering the unit whose first byte is frame
// byte q0 (a[16] only when the source is misaligned against the grid). A unit
// wholly inside the payload reads four dwordx4 and one dword: each of those
// dwords holds a payload byte. Any other unit (it holds prefix bytes or lies
// partly before the frame) reads dword by dword, and only dwords that overlap
// the payload range.
template <bool PAYLOAD>
__device__ __forceinline__ void pack_load(uint32_t (&a)[kWords + 1], const PackFrame &d, int64_t q0)
{
    const uint64_t sb = d.srcb + (uint64_t)q0;
    const uint64_t s0 = sb & ~(uint64_t)3;
    const bool mis = (sb & 3u) != 0;
    if (PAYLOAD) {
#pragma unroll
        for (int q = 0; q < kWords / 4; q++) {
            const u32x4u v = *reinterpret_cast<gu32x4u *>(s0 + 16u * q);
            a[4 * q + 0] = v.x;
            a[4 * q + 1] = v.y;
            a[4 * q + 2] = v.z;
            a[4 * q + 3] = v.w;
        }
        a[kWords] = 0;
        if (mis) a[kWords] = *reinterpret_cast<gu32 *>(s0 + 64u);
    } else {
#pragma unroll
        for (int j = 0; j <= kWords; j++) {
            const uint64_t A = s0 + 4u * j;
            const bool in = d.pend > d.pstart && A < d.pend && A + 4u > d.pstart && (j < kWords || mis);
            a[j] = 0;
            if (in) a[j] = *reinterpret_cast<gu32 *>(A);
        }
    }
}

// Assemble the unit at frame byte q0 from its source dwords, store it, and
// feed it to the lane's register. Returns the new register.
template <bool PAYLOAD>
__device__ __forceinline__ uint32_t pack_unit(const uint32_t (&a)[kWords + 1], const PackFrame &d, int64_t q0, uint32_t acc,
                                              const SliceBases &sb)
{
    const uint32_t m = (uint32_t)((d.srcb + (uint64_t)q0) & 3u);
    uint32_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; i++) w[i] = __builtin_amdgcn_alignbyte(a[i + 1], a[i], m);
    const uint64_t up = d.dst + (uint64_t)q0;  // dword-aligned
    if (PAYLOAD) {
#pragma unroll
        for (int q = 0; q < kWords / 4; q++) {
            u32x4u v;
            v.x = w[4 * q + 0];
            v.y = w[4 * q + 1];
            v.z = w[4 * q + 2];
            v.w = w[4 * q + 3];
            *reinterpret_cast<gw32x4u *>(up + 16u * q) = v;
        }
#pragma unroll
        for (int i = 0; i < kWords; i++) acc = s4_step(acc, w[i], sb);
        return acc;
    }
    // The unit holds prefix bytes, and possibly bytes before the frame.
    const int r = (int)(q0 & 3);          // frame-byte phase of the grid (also right for q0 < 0)
    const int j0 = (int)((q0 - r) >> 2);  // prefix word holding the unit's first byte (may be < 0)
    const int pre = (int)d.prefix;
#pragma unroll
    for (int i = 0; i < kWords; i++) {
        const int q = (int)q0 + 4 * i;
        const uint32_t P = __builtin_amdgcn_alignbyte(pack_pword(d, j0 + i + 1), pack_pword(d, j0 + i), (uint32_t)r);
        const uint32_t keep = q >= pre ? ~0u : (q + 4 <= pre ? 0u : ~0u << (8 * (pre - q)));
        w[i] = P | (w[i] & keep);
    }
    if (q0 >= 0) {
#pragma unroll
        for (int q = 0; q < kWords / 4; q++) {
            u32x4u v;
            v.x = w[4 * q + 0];
            v.y = w[4 * q + 1];
            v.z = w[4 * q + 2];
            v.w = w[4 * q + 3];
            *reinterpret_cast<gw32x4u *>(up + 16u * q) = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kWords; i++) {
            const int q = (int)q0 + 4 * i;
            if (q >= 0) {
                *reinterpret_cast<gw32 *>(up + 4u * i) = w[i];
            } else if (q > -4) {  // the frame's first bytes: never a read-modify-write of the dword they sit in
#pragma unroll
                for (int b = 1; b < 4; b++)
                    if (b >= -q) *reinterpret_cast<gw8 *>(up + 4u * i + b) = (uint8_t)(w[i] >> (8 * b));
            }
        }
    }
    // The seed goes into frame bytes 0..3 of the hashed words only (unit0_word).
#pragma unroll
    for (int i = 0; i < kWords; i++) {
        const int q = (int)q0 + 4 * i;
        uint32_t x = w[i];
        if (q > -4 && q < 0) x ^= ~0u << (8 * -q);
        else if (q >= 0 && q < 4) x ^= ~0u >> (8 * q);
        acc = s4_step(acc, x, sb);
    }
    return acc;
}

// Descriptor of frame f. Returns false for a rejected frame.
__device__ __forceinline__ bool pack_desc(const PackParams &p, uint64_t f, PackFrame &d)
{
    const uint32_t plen = p.pay_len[f];
    const bool expl = p.include_offset ? p.include_offset[f] != 0 : true;
    const uint64_t content = (uint64_t)plen + (expl ? 8u : 0u);
    const uint64_t foff = p.file_off[f];
    const bool nosrc = plen && (!p.payload || !p.pay_off);
    const uint64_t po = (plen && !nosrc) ? p.pay_off[f] : 0u;
    d.prefix = expl ? 16u : 8u;
    d.L = 8u + (uint32_t)content;
    d.dst = (uint64_t)(uintptr_t)p.out + (p.frame_off ? p.frame_off[f] : f * p.stride);
    d.pstart = (uint64_t)(uintptr_t)p.payload + po;
    d.pend = d.pstart + plen;
    d.srcb = d.pstart - d.prefix;
    d.h[0] = (uint32_t)VAL_PKT_DATA | (expl ? (uint32_t)VAL_DATA_OFFSET_PRESENT << 8 : 0u) | ((uint32_t)content << 16);
    d.h[1] = 0u;
    d.h[2] = (uint32_t)foff;
    d.h[3] = (uint32_t)(foff >> 32);
    return content <= 65535u && !nosrc && (p.frame_off || 12u + content <= p.stride);
}

// Build and hash frame f with the G lanes of this lane's group. All 64 lanes
// of the wave call this together (the merge tree shuffles).
template <int G>
__device__ __forceinline__ void pack_frame(const PackParams &p, uint64_t f, bool real, int g, const SliceBases &sb)
{
    PackFrame d{};
    bool active = false;
    if (real) {
        active = pack_desc(p, f, d);
        if (!active && g == 0) {  // rejected: no byte of the output, zero results, counted
            if (p.out_len) p.out_len[f] = 0u;
            if (p.out_crc) p.out_crc[f] = 0u;
            if (p.out_hdr) p.out_hdr[f] = 0u;
            if (p.nrejected) atomicAdd(p.nrejected, 1u);
        }
    }
    const uint32_t L = active ? d.L : 0u;
    // The grid ends at floor4(frame end in the output); L >= 8, so Lg >= 5.
    const uint32_t tb = active ? (uint32_t)((d.dst + L) & 3u) : 0u;
    const uint32_t Lg = L - tb;
    const uint32_t U = (Lg + kUnit - 1) / kUnit;
    const uint32_t R = (U + G - 1) >> ilog2(G);
    const uint32_t pad = U * kUnit - Lg;
    int u = (int)U - G * (int)R + g;  // this lane's unit in round 0 (< 0: none)
    int64_t q0 = (int64_t)u * kUnit - pad;
    constexpr int64_t kStep = (int64_t)G * kUnit;
    uint32_t acc = 0, k = 0;
    // Units that hold prefix bytes or start before the frame (unit 0, and unit
    // 1 when unit 0 holds less than the prefix) are a lane's first one or two
    // rounds: peeled, one round at a time, so that the main loop carries none
    // of their registers.
#pragma nounroll
    for (int s = 0; s < 2; s++) {
        if (k < R && q0 < (int64_t)d.prefix) {
            if (u >= 0) {
                uint32_t a[kWords + 1];
                pack_load<false>(a, d, q0);
                if (G > 1 && k) acc = map_apply(acc, gap_map(ilog2(G)));
                acc = pack_unit<false>(a, d, q0, acc, sb);
            }
            k++, u += G, q0 += kStep;
        }
    }
    // Payload-only units, one round of source dwords in flight ahead.
    uint32_t nxt[kWords + 1];
    if (k < R) pack_load<true>(nxt, d, q0);
    for (; k < R; k++, q0 += kStep) {
        uint32_t a[kWords + 1];
#pragma unroll
        for (int i = 0; i <= kWords; i++) a[i] = nxt[i];
        if (k + 1 < R) pack_load<true>(nxt, d, q0 + kStep);
        if (G > 1 && k) acc = map_apply(acc, gap_map(ilog2(G)));
        acc = pack_unit<true>(a, d, q0, acc, sb);
    }
    // header_crc, by the lane holding unit 0 (as hash_frame)
    if (active && (int)U - G * (int)R + g == 0 && p.out_hdr)
        p.out_hdr[f] = s4_step(s4_step(0xFFFFFFFFu, d.h[0], sb), d.h[1], sb) ^ 0xFFFFFFFFu;
    // The tb <= 3 bytes past the grid: fetched before the merge, which hides the round trip.
    const bool last = active && g == G - 1;
    uint32_t tail[3] = {0, 0, 0};
    if (last) {
#pragma unroll
        for (uint32_t j = 0; j < 3; j++) {
            const uint32_t b = Lg + j;
            if (j < tb)
                tail[j] = b < d.prefix ? (pack_pword(d, (int)(b >> 2)) >> (8 * (b & 3u))) & 255u
                                       : (uint32_t) * reinterpret_cast<gu8 *>(d.srcb + b);
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxTree; j++) {
        if ((1 << j) >= G) break;
        const uint32_t other = __shfl_xor(acc, 1 << j);
        const bool right = (g >> j) & 1;
        const uint32_t left = right ? other : acc;
        acc = map_apply(left, tree_map(j)) ^ (right ? acc : other);
    }
    if (last) {
#pragma unroll
        for (uint32_t j = 0; j < 3; j++)
            if (j < tb) {
                *reinterpret_cast<gw8 *>(d.dst + Lg + j) = (uint8_t)tail[j];
                acc = byte_step(acc, tail[j], sb);
            }
        const uint32_t crc = acc ^ 0xFFFFFFFFu;
        // LE32 trailer at any alignment: four byte stores
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) *reinterpret_cast<gw8 *>(d.dst + L + b) = (uint8_t)(crc >> (8 * b));
        if (p.out_crc) p.out_crc[f] = crc;
        if (p.out_len) p.out_len[f] = L;
    }
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_pack(const PackParams p)
{
    constexpr int kGroups = 64 / G;
    const int lane = threadIdx.x & 63;
    const SliceBases sb = slice_bases((uint32_t)(lane & 31) << 2);
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    LdsImage im;
    lds_tables_issue(p.consts, im);
    lds_tables_write(im);
    __syncthreads();
    for (uint64_t fb = wave * kGroups; fb < p.n; fb += nwaves * kGroups) {
        const uint64_t f = fb + (uint64_t)(lane / G);
        pack_frame<G>(p, f, f < p.n, lane % G, sb);
    }
}

}  // namespace vcrc
