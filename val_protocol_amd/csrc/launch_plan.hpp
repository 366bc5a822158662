// launch_plan.hpp -- the launch policy: which kernel a batch of frames gets,
// with how many lanes, which round loop and which grid, and whether it takes
// the dynamic tail, the in-launch tail pieces or the split kernel
// (plan_frames()); and the lanes and grids of the window calls' launches: the
// framer, both unpack calls, the scan, the fill, the file windows and the
// ACK calls (plan_pack(), plan_unpack(), plan_scan(), plan_fill(),
// plan_file_windows(), plan_ack()). They map plain numbers to
// launches and call no HIP API; val_crc32_hip.hip fills in the kernels'
// params, executes a plan and decides nothing. tests/test_launch_plan.py pins
// the plans of a table of shapes through val_gpu_plan_frames() and
// val_gpu_plan_window(), tests/test_launch_plan_windows.py those of
// val_gpu_plan_file_windows(). Every threshold here is a measured result; the
// experiments are in DESIGN_EXPERIMENTS.md and DESIGN.md section 5.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "ack_kernel.hpp"
#include "crc_kernels.hpp"
#include "fill_kernel.hpp"
#include "pack_kernel.hpp"
#include "scan_kernel.hpp"
#include "unpack_kernel.hpp"
#include "val_crc32_gpu.h"
#include "windows_kernel.hpp"

namespace vcrc {

// Dynamic tail of long uniform launches (k_frames): a launch takes it when it
// is long enough for the queue to pay: 8 or 16 lanes per frame from 1.45 MiB
// of frames per wave (about 6 GB at 4,096 waves), 2 or 4 lanes from 8 group
// rounds. Shorter launches measured faster static, once the exits were counted
// per workgroup (same box, back to back,
// profiles/r06_ab_dyn_tail_rules.log): 64 KiB frames 4 / 5 rounds -2.5 /
// -0.6% with the queue, 6 / 7 rounds +0.5 / +1.0%; 16,400-B frames 6 / 8
// rounds -3.7 / -1.6%, 12 / 16 rounds +0.5 / +1.6%; 4,200-B frames (8 lanes,
// 34 KiB groups) 4 / 8 / 12 rounds -8 / -5 / -3.6%; 1,100-B and 2,000-B frames
// at 4 rounds -5% and -3.9%, 600-B and 1,100-B frames at 8 rounds +3.6% and
// +3.2%.
#ifndef VCRC_DYN_MIN_WAVE_BYTES
#define VCRC_DYN_MIN_WAVE_BYTES 1520000u
#endif
#ifndef VCRC_DYN_MIN_ROUNDS_SHORT
#define VCRC_DYN_MIN_ROUNDS_SHORT 8
#endif
// Which queue a long enough launch pulls from, by the bytes of a frame group.
// Groups of >= 128 KiB (strided) or 192 KiB (descriptors) pull from one word:
// 4,096 waves over 128 KiB groups is about 48 dequeues/us at 6 TB/s, under the
// ~88/us one word serves, and one word evens the end out better than
// partitions (cfg3 -1.5%, cfg4 -3.7% with 64). Groups under 128 KiB pull from
// 64 partitions: descriptor groups from 16 KiB (round 2: u4200d +4%, u1100d
// +6%; with one word they lost up to 2x), strided ones from 32 KiB (s4200 +3%;
// s1100's 17.6 KiB groups -3%); descriptor groups of 128-192 KiB stay static
// below 16 rounds (u16400d -1% either way: profiles/r02_ab_dynparts.log) and
// take one word above.
#ifndef VCRC_DYN_MIN_GROUP  // one-word minimum group bytes, strided / descriptor batches
#define VCRC_DYN_MIN_GROUP (128u << 10)
#endif
#ifndef VCRC_DYN_MIN_GROUP_DESC
#define VCRC_DYN_MIN_GROUP_DESC (192u << 10)
#endif
#ifndef VCRC_DYN_MIN_GROUP_PARTS  // partitioned queue minimum group bytes, strided / descriptor batches
#define VCRC_DYN_MIN_GROUP_PARTS (32u << 10)
#endif
#ifndef VCRC_DYN_MIN_GROUP_PARTS_DESC
#define VCRC_DYN_MIN_GROUP_PARTS_DESC (16u << 10)
#endif
// Descriptor groups of 128-192 KiB take the one-word queue only from 16
// rounds on: cfg3's layout through descriptors (32 rounds) +3.0%, 3 GB of
// 16,400-B frames (6 rounds) -2.8% with it (profiles/r06_ab_desc_dyn_tail.log).
#ifndef VCRC_DYN_DESC_LONG_ROUNDS
#define VCRC_DYN_DESC_LONG_ROUNDS 16
#endif
constexpr uint64_t kDynMinWaveBytes = VCRC_DYN_MIN_WAVE_BYTES;
constexpr uint64_t kDynMinRoundsShort = VCRC_DYN_MIN_ROUNDS_SHORT;
constexpr uint64_t kDynMinGroup = VCRC_DYN_MIN_GROUP, kDynMinGroupDesc = VCRC_DYN_MIN_GROUP_DESC;
constexpr uint64_t kDynMinGroupParts = VCRC_DYN_MIN_GROUP_PARTS, kDynMinGroupPartsDesc = VCRC_DYN_MIN_GROUP_PARTS_DESC;
constexpr uint64_t kDynDescLongRounds = VCRC_DYN_DESC_LONG_ROUNDS;

// The process's run-time knobs as plain values (val_crc32_hip.hip plan_knobs()).
struct PlanKnobs {
    uint32_t forced_lanes;  // 0 = none
    int forced_prefetch;    // -1 = none
    bool dyn_tail, split, tail_pieces;
    uint32_t ragged_min;
    uint32_t scan_front;  // 0 = by the number of streams
    uint32_t window_k0;   // file windows: log2 of the chunk bytes, 0 = automatic
    int stream_loads = -1;  // 1 / 0: forced on / off; -1: by the rule (Planner::stream_loads)
};

using Launch = val_gpu_launch_t;
enum : uint32_t { kKernelRagged = VAL_GPU_KERNEL_RAGGED, kKernelSplit = VAL_GPU_KERNEL_SPLIT,
                  kKernelFrames = VAL_GPU_KERNEL_FRAMES, kKernelFramesC0 = VAL_GPU_KERNEL_FRAMES_C0 };

// Zero, one or two launches; the second is the re-cut tail of the first.
struct LaunchPlan {
    uint32_t count = 0;
    Launch launch[2] = {};
};

struct Planner {
    uint32_t cus;
    bool desc, pay;
    uint32_t flen, last_len;
    PlanKnobs k;

    // Lanes that share one frame (G) in uniform batches, by length: the measured
    // best of the current kernels (profiles/r03_length_sweep.log, strided 3 GB
    // batches): 2 below 1 KiB, 4 below 2 KiB, 8 below 48 KiB,
    // 16 above. G = 8 from 2 KiB gained 3-5% over G = 4 on 2-4 KiB frames and
    // 5% on u4200d (profiles/r03_ab_geom_short.log). The ragged path keeps its
    // length classes (kClassLanes), whose buckets are rounds of their class.
    uint32_t lanes_per_frame(uint32_t len) const
    {
        const uint32_t f = k.forced_lanes;
        if (f) return f;
        return len < 1024u ? 2u : len < 2048u ? 4u : len < 49152u ? 8u : 16u;
    }

    // G for a uniform batch of n frames of len bytes: the class's G, doubled while
    // the batch would leave more than half of the machine's waves idle (a small
    // window spreads each frame over more lanes, so its serial chain is shorter),
    // up to one wave per frame and at most one 64-B unit per lane per round. The
    // doubling only acts on batches of fewer groups than half the machine's waves
    // (one pass of the grid); large batches keep the class's measured G. Capping
    // it at 16 cost small windows of long frames 1.5-2.5x (256 x 64 KiB: 103 ->
    // 41 us per call; 256 x 16 KiB: 34 -> 20 us; profiles/r02_ab_lanes_cap.log).
    uint32_t lanes_for_batch(uint32_t len, uint64_t n) const
    {
        uint32_t G = lanes_per_frame(len);
        if (k.forced_lanes) return G;
        const uint64_t waves = (uint64_t)cus * kWavesPerBlock;
        const uint64_t units = len ? (len + kUnit - 1) / kUnit : 1u;
        const uint32_t cap = 64u;
        while (G < cap && 2u * G <= units && (n + 64 / G - 1) / (64 / G) * 2u <= waves) G *= 2;
        return G;
    }

    // Load path of a planned k_frames launch: rounds >= 1 through nt LDS-DMA
    // beside the compact table image (crc_kernels.hpp hash_frame_stream)
    // instead of ordinary loads. Instances: 8 lanes per frame, the default
    // depth, no payload states. By the rule only multi-pass launches of frames
    // of at least 8 KiB take it: the stream is worth its longer prologue-to-
    // first-hash path only over many rounds (cfg3: 32 rounds a frame, 32 group
    // rounds a wave; profiles/ab_stream_loads_cfg3.jsonl), and a one-pass launch
    // is latency-bound, not stream-bound. Forced on, every launch the instances
    // can hash takes it (tests). 16 lanes: not measured, so not built.
    // the frame length the rule goes by: as frames() takes it
    uint32_t stream_len(uint32_t typical_len) const { return typical_len ? typical_len : 16384u; }
    bool stream_loads(const Launch &l, uint32_t len) const
    {
        if (k.stream_loads == 0 || pay || l.lanes != 8u || l.depth != 1) return false;
        if (l.kernel != kKernelFrames && l.kernel != kKernelFramesC0) return false;
        if (k.stream_loads == 1) return true;
        return l.kernel == kKernelFrames && len >= 8192u;
    }

    // Small batches of long frames go to k_frames_split (one workgroup per frame,
    // its chunks hashed by 16 waves at once) when that takes fewer memory rounds
    // per wave than one wave per frame: ceil(n / CUs) passes of about three
    // round-times each (a chunk round, the fold, the next frame's start) against
    // ceil(units / 64) rounds. Measured (profiles/r02_ab_split.log): 256 x 64 KiB
    // 41 -> 18 us per call, 256 x 8 KiB 21.5 -> 16 us, equal at 1024 x 64 KiB,
    // slower at 2048 x 64 KiB and 512 x 16 KiB (the rule keeps those off it).
    // Payload states and forced geometries keep the frames kernels.
    bool use_split(uint32_t n, uint32_t len) const
    {
        if (!k.split || pay || k.forced_lanes || k.forced_prefetch != -1 || len < 8192u) return false;
        const uint64_t waves = (uint64_t)cus * kWavesPerBlock;
        if ((uint64_t)n * 2u > waves) return false;
        const uint64_t rounds = ((uint64_t)len / kUnit + 1u + 63u) / 64u;  // at one wave per frame
        const uint64_t passes = ((uint64_t)n + cus - 1u) / (uint64_t)cus;
        return passes * 3u <= rounds;
    }

    Launch split(uint32_t first, uint32_t n, uint32_t len) const
    {
        Launch l{};
        l.kernel = kKernelSplit;
        l.first = first;
        l.count = n;
        // W = 2^k0 >= 1 KiB with a typical frame in at most 16 chunks (one group)
        uint32_t k0 = 10;
        while (((uint64_t)kWavesPerBlock << k0) < (uint64_t)len && k0 < 31) k0++;
        l.k0 = k0;
        l.grid = (uint32_t)std::min<uint64_t>(n, (uint64_t)cus);
        return l;
    }

    // One k_frames launch of frames [first, first + n) at G lanes; l carries the
    // in-launch tail (tail_n, tail_k0, tail_units), if any.
    Launch uniform_one(Launch l, uint32_t first, uint32_t n, uint32_t G, uint32_t len) const
    {
        l.first = first;
        l.count = n;
        l.lanes = G;
        const uint64_t groups_per_block = (uint64_t)kWavesPerBlock * (64 / G);
        uint64_t blocks = (n + groups_per_block - 1) / groups_per_block;
        blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)cus));  // persistent, 1 per CU (LDS)
        l.grid = (uint32_t)blocks;
        // Rounds kept in flight ahead of the one being hashed: 1 unless forced.
        // Measured on MI355X (profiles/r01_small_batches.log): issuing every round up
        // front (2 or 4 deep) lost 5-15% even on one-pass batches such as cfg2, since
        // the whole batch's requests then land before any wave can start hashing.
        int pf = k.forced_prefetch != -1 ? k.forced_prefetch : 1;
        // Dynamic tail for long launches: the last half of the group rounds come
        // from a queue (k_frames); the thresholds are at the top of this file.
        const uint64_t rounds = ((uint64_t)n + 64 / G - 1) / (64 / G) / (blocks * kWavesPerBlock);
        const uint64_t group_bytes = (uint64_t)(64 / G) * len;
        const bool one_word = group_bytes >= (desc ? (rounds >= kDynDescLongRounds ? kDynMinGroup : kDynMinGroupDesc)
                                                   : kDynMinGroup);
        const bool parts =
            group_bytes >= (desc ? kDynMinGroupPartsDesc : kDynMinGroupParts) && group_bytes < kDynMinGroup;
        const bool long_enough = G >= 8 ? rounds * group_bytes >= kDynMinWaveBytes : rounds >= kDynMinRoundsShort;
        if (k.dyn_tail && long_enough && (one_word || parts)) {
            l.qparts = one_word ? 1u : kDynParts;
            l.static_rounds = (uint32_t)(rounds - std::max<uint64_t>(1, rounds / 2));
        }
        // one_pass: every wave hashes at most one frame group (windows, cfg2): round
        // 0's units by dword loads (k_frames C0; crc_kernels.hpp load_unit0).
        const bool one_pass = ((uint64_t)n + 64 / G - 1) / (64 / G) <= blocks * kWavesPerBlock;
        l.kernel = kKernelFrames;
        l.depth = 1;
        if (pay) return l;  // payload states: default depth only
        // One-pass launches keep the depth-1 loop at every G: rings measured no
        // better on cfg2 (two deep +0.6% back to back, -3.7% single launch; three deep
        // -7%) and equal on 64-4,096-frame windows
        // (profiles/r04_ab_ring_prefetch_one_pass.log).
        if (pf == 1 && one_pass) {
            l.kernel = kKernelFramesC0;
            return l;
        }
        // Multi-pass short frames hash each round in its registers and refill them
        // in place (a ring of -pf rounds, crc_kernels.hpp hash_frame BURST):
        // profiles/r04_ab_ring_prefetch.log, same box against the copy-and-refill
        // PF = 1 loop: G = 2 three deep u600d +4.2% (two deep +1.8%); G = 4 two
        // deep u1100d +1.5-1.8%, s1100 0%, u2000d -0.3 to -0.6% (three deep -0.7 to
        // -3%), so 4 lanes take the ring below 1,600 B (R <= 7) only.
        if (pf == 1 && k.forced_prefetch == -1) pf = G == 2 ? -3 : (G == 4 && len < 1600u) ? -2 : 1;
        const bool ring = pf == -2 || pf == -3;
        l.depth = ring && G != 2 && G != 4 ? 1 : pf;  // a ring forced at other lanes runs depth 1
        return l;
    }

    // In-launch tail pieces (crc_kernels.hpp tail_pieces): the frames past the
    // last full wave-round, cut into pieces of W = 2^k0 bytes and hashed by the
    // oldest waves as one extra frame group each, instead of a second launch.
    // W = 1 KiB (one round at 16 lanes: the extra work per wave stays under what
    // the oldest waves gain on the youngest), doubled while the piece groups
    // outnumber the waves. Kernels with G = 8 or 16 at the default depth carry
    // the path; frames of at least 8 KiB use it.
    // log2 of the piece bytes for this tail, or 0 when the path does not apply.
    uint32_t tail_piece_k0(uint32_t G, uint32_t len, uint64_t n_tail) const
    {
        if (!k.tail_pieces || pay || (G != 8 && G != 16) || len < 8192u || n_tail == 0 || k.forced_prefetch != -1)
            return 0;
        for (uint32_t k0 = kPieceK0Min; k0 <= 16; k0++) {
            const uint64_t units = n_tail * (((uint64_t)len + (1u << k0) - 1) >> k0);
            if ((units + 64 / G - 1) / (64 / G) <= (uint64_t)cus * kWavesPerBlock) return k0;
        }
        return 0;
    }

    // Persistent waves take whole frame groups, so a launch lasts
    // ceil(groups / waves) group-times: 131,113 frames of 64 KiB at G = 16 are
    // 8.002 wave-rounds, the last one 99.8% idle. The frames of a partial last
    // round are hashed in pieces inside the launch (tail_piece_k0), else re-cut
    // with more lanes per frame (up to 64) into a second launch on the same
    // stream, so the tail costs about G / G_tail of a group-time.
    LaunchPlan uniform(uint32_t n, uint32_t G, uint32_t len) const
    {
        LaunchPlan pl;
        const uint64_t per = 64 / G, groups = (n + per - 1) / per;
        const uint64_t waves = (uint64_t)cus * kWavesPerBlock;
        const uint64_t full = groups / waves;
        uint32_t Gt = G;
        const uint64_t n_main = full * waves * per, n_tail = n - std::min<uint64_t>(n, n_main);
        if (full > 0 && n_tail > 0)
            while (Gt < 64 && (n_tail + 64 / (2 * Gt) - 1) / (64 / (2 * Gt)) <= waves) Gt *= 2;
        if (Gt == G) {
            pl.count = 1;
            pl.launch[0] = uniform_one(Launch{}, 0, n, G, len);
            return pl;
        }
        if (const uint32_t k0 = tail_piece_k0(G, len, n_tail)) {
            Launch l{};
            l.tail_n = (uint32_t)n_tail;
            l.tail_k0 = k0;
            l.tail_units = (uint32_t)(((uint64_t)len + (1u << k0) - 1) >> k0);
            pl.count = 1;
            pl.launch[0] = uniform_one(l, 0, (uint32_t)n_main, G, len);
            return pl;
        }
        pl.count = 2;
        pl.launch[0] = uniform_one(Launch{}, 0, (uint32_t)n_main, G, len);
        // a tail of a few long frames (cfg4: 41 x 64 KiB after 8 full rounds) is a
        // small batch of its own: one workgroup per frame when that is faster
        const uint32_t tl = desc ? len : std::max(flen, last_len);
        if (use_split((uint32_t)n_tail, tl)) pl.launch[1] = split((uint32_t)n_main, (uint32_t)n_tail, tl);
        else pl.launch[1] = uniform_one(Launch{}, (uint32_t)n_main, (uint32_t)n_tail, Gt, tl);
        return pl;
    }

    // Ragged descriptor batch: the grouped launch after the binning kernels.
    Launch ragged(uint32_t n) const
    {
        Launch l{};
        l.kernel = kKernelRagged;
        l.count = n;
        // persistent: enough waves for the items, at most one workgroup per CU
        const uint64_t max_items = (n + 3u) / 4u + kClasses;  // every class packs >= 4 frames per item
        l.grid = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>((uint64_t)cus, (max_items + kWavesPerBlock - 1) / kWavesPerBlock));
        // The ragged kernel keeps the copy-and-refill loop: the rings lost 9-11% on
        // cfg5 and the class-2 mix and 2-3% on 600 and 1,100-B frames through the
        // ragged path (profiles/r04_ab_ring_prefetch_ragged.log).
        l.depth = pay ? 1 : k.forced_prefetch == 0 ? 0 : 1;
        return l;
    }

    // typical_len == 0 with descriptors means "lengths unknown or mixed": bin them,
    // unless the batch is too small to fill the machine once (binning is four
    // launches; a small window runs uniform at 16 lanes per frame instead).
    LaunchPlan frames(uint32_t n, uint32_t typical_len) const
    {
        LaunchPlan pl;
        if (n == 0) return pl;
        pl.count = 1;
        if (desc && typical_len == 0 && !k.forced_lanes && n >= k.ragged_min) {
            pl.launch[0] = ragged(n);
            return pl;
        }
        const uint32_t len = typical_len ? typical_len : 16384u;
        const uint32_t longest = !desc ? std::max(flen, last_len) : len;
        if (use_split(n, longest)) {
            pl.launch[0] = split(0, n, longest);
            return pl;
        }
        return uniform(n, lanes_for_batch(len, n), len);
    }
};

// The plan of one batch: n frames on a device of `cus` compute units,
// typical_len as launch_frames receives it (0: unknown or mixed), strided
// (flen, last_len) or descriptors, with or without payload states.
inline LaunchPlan plan_frames(uint32_t cus, uint32_t n, uint32_t typical_len, bool descriptors, uint32_t flen,
                              uint32_t last_len, bool want_payload, const PlanKnobs &knobs)
{
    return Planner{cus, descriptors, want_payload, flen, last_len, knobs}.frames(n, typical_len);
}

// ---- the window calls -------------------------------------------------------
// Up to four launches on the caller's stream, in order. Their kernels use no
// library scratch, so a launch is a kernel, its grid and, where the kernel is
// instantiated by them, its lanes; count is the entries the grid covers.
struct WindowPlan {
    uint32_t count = 0;
    Launch launch[4] = {};

    void add(uint32_t kernel, uint64_t grid, uint64_t entries, uint32_t lanes = 0)
    {
        Launch &l = launch[count++];
        l.kernel = kernel;
        l.lanes = lanes;
        l.grid = (uint32_t)grid;
        l.count = (uint32_t)entries;
    }
};

// Lanes per frame of k_pack and k_unpack: forced (val_gpu_set_lanes_per_frame),
// else from len_hint as the hash kernels choose them; without a hint, the
// geometry of MTU-sized frames, which is correct for every length. `threads`
// is the kernel's whole persistent grid.
inline uint32_t window_lanes(uint32_t n, uint32_t len_hint, uint64_t threads, const PlanKnobs &k)
{
    uint32_t lanes = k.forced_lanes;
    if (!lanes) {
        lanes = Planner{0, false, false, 0, 0, k}.lanes_per_frame(len_hint ? len_hint : 1100u);
        // A batch that leaves workgroups of the grid empty doubles its lanes until it fills them
        // (65,536 frames at 2 lanes are 128 of 256 workgroups).
        while (lanes < 64u && (uint64_t)n * lanes * 2u <= threads) lanes *= 2u;
    }
    return lanes;
}

// Device framer (pack_kernel.hpp): one k_pack launch over n entries, after
// the launches of `pl` (the fill's). A persistent grid of at most one
// workgroup per CU; the kernel uses no scratch.
inline WindowPlan plan_pack(uint32_t cus, uint32_t n, uint32_t len_hint, const PlanKnobs &k, WindowPlan pl = {})
{
    if (n == 0) return pl;
    const uint32_t G = window_lanes(n, len_hint, (uint64_t)std::max(cus, 1u) * kBlock, k);
    const uint64_t groups = ((uint64_t)n + (64 / G) - 1) / (64 / G);
    const uint64_t blocks = (groups + kWavesPerBlock - 1) / kWavesPerBlock;
    pl.add(VAL_GPU_KERNEL_PACK, std::min<uint64_t>(blocks, std::max(cus, 1u)), n, G);
    return pl;
}

// Device unpacker (unpack_kernel.hpp), after the verify launches (plan_frames
// with typical_len): the header facts grid-wide, then the receiver's rule: one
// workgroup for one file, else (files) a workgroup per file up to one per CU;
// then the scatter, lanes per frame as k_pack picks them, in a persistent grid
// of at most kUnpackBlocksPerCU workgroups per CU (the kernel holds no LDS and
// no scratch).
inline WindowPlan plan_unpack(uint32_t cus, uint32_t n, bool files, uint32_t n_files, uint32_t typical_len,
                              const PlanKnobs &k)
{
    WindowPlan pl;
    if (n == 0 || (files && n_files == 0)) return pl;
    pl.add(VAL_GPU_KERNEL_UNPACK_PARSE, ((uint64_t)n + 255u) / 256u, n);
    if (files) pl.add(VAL_GPU_KERNEL_UNPACK_ORDER_FILES, std::min(n_files, std::max(cus, 1u)), n_files);
    else pl.add(VAL_GPU_KERNEL_UNPACK_ORDER, 1, n);
    // as k_pack: a batch that leaves workgroups of the grid empty doubles its lanes until it fills them
    const uint64_t threads = (uint64_t)std::max(cus, 1u) * kUnpackBlocksPerCU * kUnpackBlock;
    const uint32_t G = window_lanes(n, typical_len, threads, k);
    const uint64_t groups = ((uint64_t)n + (64 / G) - 1) / (64 / G);
    const uint64_t blocks = (groups + (kUnpackBlock / 64) - 1) / (kUnpackBlock / 64);
    pl.add(VAL_GPU_KERNEL_UNPACK, std::min<uint64_t>(blocks, (uint64_t)std::max(cus, 1u) * kUnpackBlocksPerCU), n, G);
    return pl;
}

// Device frame scan (scan_kernel.hpp). The walk, in a persistent grid: a
// workgroup of 16 waves per stream while every stream can have a CU of its
// own, else a wave per stream (the launch's lanes are
// the lanes per stream). Results do not depend on it. A slot product beyond
// 32 bits, which the call refuses, has no plan.
inline WindowPlan plan_scan(uint32_t cus32, uint32_t n_streams, uint32_t max_frames, const PlanKnobs &k)
{
    WindowPlan pl;
    const uint64_t slots = (uint64_t)n_streams * max_frames;
    if (slots == 0 || slots > UINT32_MAX) return pl;
    const uint64_t cus = (uint64_t)std::max(cus32, 1u);
    const uint64_t cap = cus * kScanBlocksPerCU;
    uint32_t front = k.scan_front;
    if (!front) front = n_streams <= cus ? 64u * kScanWideWaves : 64u;
    constexpr uint32_t per = kScanBlock / 64;
    const uint64_t wgrid = front == 64u ? std::min<uint64_t>(((uint64_t)n_streams + per - 1) / per, cap)
                                        : std::min<uint64_t>(n_streams, cus * 2u);
    pl.add(VAL_GPU_KERNEL_SCAN_STREAMS, wgrid, n_streams, front);
    pl.add(VAL_GPU_KERNEL_SCAN_FIRST, 1, n_streams);
    pl.add(VAL_GPU_KERNEL_SCAN_COMPACT, std::min<uint64_t>((slots + kScanBlock - 1) / kScanBlock, cap), slots);
    return pl;
}

// Device window fill (fill_kernel.hpp): the counts, d_first by the scan call's
// kernel, k_pack's inputs for every slot in a persistent grid, then k_pack
// over every slot with the content of a full frame as its hint.
inline WindowPlan plan_fill(uint32_t cus, uint32_t n_files, uint32_t max_frames, uint64_t mtu, const PlanKnobs &k)
{
    WindowPlan pl;
    const uint64_t slots = (uint64_t)n_files * max_frames;
    if (slots == 0 || slots > UINT32_MAX) return pl;
    pl.add(VAL_GPU_KERNEL_FILL_COUNT, ((uint64_t)n_files + kFillBlock - 1) / kFillBlock, n_files);
    pl.add(VAL_GPU_KERNEL_SCAN_FIRST, 1, n_files);
    const uint64_t cap = (uint64_t)std::max(cus, 1u) * kFillBlocksPerCU;
    pl.add(VAL_GPU_KERNEL_FILL_DESC, std::min<uint64_t>((slots + kFillBlock - 1) / kFillBlock, cap), slots);
    return plan_pack(cus, (uint32_t)slots, (uint32_t)(mtu - VAL_WIRE_TRAILER_SIZE), k, pl);
}

// File windows (windows_kernel.hpp): the count launch of one thread per file,
// the prefix sum, then the hash in a persistent grid of at most one workgroup
// per CU (the kernel holds the LDS tables), sized for the most chunks the call
// can have, n_files * ceil(max_len / W): the host does not know the lengths.
// W = 2^k0 is one chunk size for the whole call. Automatic: the smallest of
// 4 .. 64 KiB at which that bound is at most one chunk per wave of the machine
// (region_geometry's idea: a single 8 MiB window gets 4 KiB chunks, 256 MiB get
// 64 KiB), and 64 KiB when none is. Against every forced k0 on four batch
// shapes it was the fastest or within 1% of it (profiles/resume_timing.json,
// DESIGN.md section 5); other shapes have not been timed. A forced
// k0 (val_gpu_set_file_window_chunk) is taken, and like the automatic one
// raised as far as the fold needs: at most 2^16 chunks per window (16 maps) and
// fewer than 2^32 chunks in all. A call that needs more than 64 KiB for either
// (max_len above 2^32, or the bound overflowing 32 bits at 64 KiB) is refused
// and has no plan. max_len == 0 hashes nothing: the count launch alone
// finishes every file.
inline uint64_t window_chunks(uint32_t n_files, uint64_t max_len, uint32_t k0)
{
    return (uint64_t)n_files * ((max_len >> k0) + ((max_len & (((uint64_t)1 << k0) - 1u)) ? 1u : 0u));
}

inline bool file_windows_fit(uint32_t n_files, uint64_t max_len)
{
    return max_len <= kWinMaxLen && window_chunks(n_files, max_len, kWinK0Max) <= UINT32_MAX;
}

inline WindowPlan plan_file_windows(uint32_t cus32, uint32_t n_files, uint64_t max_len, const PlanKnobs &k)
{
    WindowPlan pl;
    if (n_files == 0 || !file_windows_fit(n_files, max_len)) return pl;
    const uint64_t cus = (uint64_t)std::max(cus32, 1u);
    uint32_t k0 = k.window_k0 ? k.window_k0 : kWinK0Min;
    if (!k.window_k0)
        while (k0 < kWinK0Max && window_chunks(n_files, max_len, k0) > cus * kWavesPerBlock) k0++;
    while (k0 < kWinK0Max &&
           (max_len > ((uint64_t)1 << (k0 + kNumPowMaps)) || window_chunks(n_files, max_len, k0) > UINT32_MAX))
        k0++;
    pl.add(VAL_GPU_KERNEL_WINDOWS_COUNT, ((uint64_t)n_files + kWinCountBlock - 1) / kWinCountBlock, n_files);
    pl.launch[0].k0 = k0;
    if (max_len == 0) return pl;
    pl.add(VAL_GPU_KERNEL_SCAN_FIRST, 1, n_files);
    const uint64_t chunks = window_chunks(n_files, max_len, k0);
    pl.add(VAL_GPU_KERNEL_WINDOWS_HASH, std::min<uint64_t>((chunks + kWavesPerBlock - 1) / kWavesPerBlock, cus), chunks);
    pl.launch[2].k0 = k0;
    return pl;
}

// The ACK calls (ack_kernel.hpp), after their verify launches if any.
// Respond: the header facts grid-wide (k_unpack_parse), the rule in
// k_unpack_order_files' layout (a workgroup per file up to one per CU, each
// taking whole files in turn: the scans are sequential only within a file;
// workgroups of 256 threads, up to eight per CU, when the files are small),
// then the response frames grid-wide, one frame per thread. Apply: one launch
// in the same per-file layout.
inline WindowPlan plan_ack(uint32_t call, uint32_t cus, uint32_t n, uint32_t n_files)
{
    WindowPlan pl;
    if (n == 0 || n_files == 0) return pl;
    const uint64_t files_grid = std::min(n_files, std::max(cus, 1u));
    if (call == VAL_GPU_ACK_RESPOND) {
        pl.add(VAL_GPU_KERNEL_UNPACK_PARSE, ((uint64_t)n + 255u) / 256u, n);
        // lanes = the workgroup's threads: small files run eight workgroups of 256 per CU side by side
        if (n / n_files <= (uint32_t)kAckSmallFrames)
            pl.add(VAL_GPU_KERNEL_ACK_RESPOND_FILES,
                   std::min<uint64_t>(n_files, (uint64_t)std::max(cus, 1u) * kAckSmallPerCU), n_files, kAckSmallBlock);
        else pl.add(VAL_GPU_KERNEL_ACK_RESPOND_FILES, files_grid, n_files, kAckBlock);
        pl.add(VAL_GPU_KERNEL_ACK_EMIT, ((uint64_t)n + kAckEmitBlock - 1) / kAckEmitBlock, n);
    } else if (call == VAL_GPU_ACK_APPLY) {
        pl.add(VAL_GPU_KERNEL_ACK_APPLY_FILES, files_grid, n_files);
    }
    return pl;
}

}  // namespace vcrc
