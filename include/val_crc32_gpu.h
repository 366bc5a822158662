/*
 * val_crc32_gpu.h -- C ABI of the MI355X (gfx950) CRC-32 integrity path.
 * Exported by val_protocol_amd/libval_crc_hip.so. Plain C types only; HIP
 * streams travel as `void *` (a hipStream_t; NULL = the HIP default stream).
 *
 * What each entry point replaces in the reference (VAL v0.7):
 *   val_gpu_crc32_provider  -> a crc32_func_t for val_config_t.crc32_provider
 *                              (include/val_protocol.h:163-166, :264-266),
 *                              consumed by val_internal_crc32
 *                              (src/val_core.c:399-406) and the region CRC
 *                              (src/val_core.c:431-438)
 *   val_crc32, val_crc32_{init,update,finalize}_state
 *                           -> src/val_core.c:150-183 (declared in
 *                              val_protocol.h)
 *   val_crc32_frames_*      -> the per-frame trailer CRC of the TX path
 *                              (src/val_core.c:828-834), batched over a window
 *                              (src/val_sender.c:822-841); optional header_crc
 *   val_crc32_verify_frames_* -> the RX trailer check (src/val_core.c:963-974),
 *                              batched; counts mismatches like crc_errors++
 *   val_crc32_region_dev    -> val_internal_crc32_region (src/val_core.c:414-455)
 *                              for resume tail-verify windows up to and beyond
 *                              256 MiB (src/val_receiver.c:158-181)
 *   val_crc32_combine/shift -> GF(2) algebra used to split long windows and
 *                              shard batches across GPUs (no reference
 *                              counterpart; zlib's crc32_combine identity)
 *
 *   val_crc32_*_multi       -> the same batches split over several GPUs of
 *                              one process, one host thread per device
 *                              (a window of src/val_sender.c:
 *                              822-841 sharded by contiguous frame ranges)
 *
 * Batch, region and device calls compute on the GPU only and return
 * VAL_ERR_IO on a missing device or a HIP failure. The three scalar hooks
 * (provider, val_crc32, val_crc32_update_state) take host memory, have no
 * error channel and are called by VAL under its session mutex on every
 * frame: inputs below the provider threshold (val_gpu_provider_min_bytes)
 * are answered by this library's own CPU engine, where a GPU round trip
 * cannot win, so the drop-in is never slower than the reference's byte loop;
 * longer inputs run on the GPU. On a GPU failure the hooks return the CRC
 * from the same CPU engine and count it (val_gpu_cpu_fallback_count);
 * VAL_GPU_CPU_FALLBACK=0 or val_gpu_set_cpu_fallback(0) makes them abort.
 */
#ifndef VAL_CRC32_GPU_H
#define VAL_CRC32_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "val_errors.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VAL_GPU_ABI_VERSION 1u

/* ---- lifetime ---------------------------------------------------------- */
/* Initialise HIP device `device` (0-based) and bind the calling thread to it.
 * The first device initialised is the process default, used by threads that
 * never bound one; the first CRC call initialises device 0 if none was.
 * Each device has its own streams, constant tables, staging and scratch. */
val_status_t val_gpu_init(int device);
/* Initialise devices 0..n-1 (n <= 0: all). Returns how many are usable. */
int val_gpu_init_devices(int n);
/* Bind the calling thread to `device` (initialised on first use); later calls
 * of this thread run there. hipSetDevice is per thread in HIP. */
val_status_t val_gpu_set_device(int device);
/* Device the calling thread's calls run on (-1: none initialised yet). */
int val_gpu_current_device(void);
/* Release every device context of the process (not concurrently with other
 * calls of this library; contexts are re-created on the next call). */
void val_gpu_shutdown(void);
int val_gpu_device_count(void);
uint32_t val_gpu_abi_version(void);
/* Last HIP/validation error text of the calling thread ("" if none). */
const char *val_gpu_last_error(void);
/* Scalar-hook calls answered by the CPU because the GPU path failed. */
uint64_t val_gpu_cpu_fallback_count(void);
/* 1: failed scalar hooks use the CPU (default), 0: they abort, -1: from
 * VAL_GPU_CPU_FALLBACK (unset or non-"0" = on). */
void val_gpu_set_cpu_fallback(int enable);

/* ---- scalar hooks (host memory) --------------------------------------- */
uint32_t val_gpu_crc32_provider(uint32_t seed, const void *buf, size_t len);
/* Inputs shorter than this many bytes are answered on the CPU by the scalar
 * hooks (the measured crossover). Set with
 * val_gpu_set_provider_min_bytes (-1 = VAL_GPU_PROVIDER_MIN_BYTES from the
 * environment, else the built-in default; 0 = always the GPU). */
void val_gpu_set_provider_min_bytes(int64_t bytes);
uint64_t val_gpu_provider_min_bytes(void);
/* Scalar-hook calls answered on the CPU because they were below the threshold. */
uint64_t val_gpu_cpu_small_count(void);
/* Where the calling thread's last scalar-hook call was answered. */
#define VAL_GPU_HOOK_NONE 0     /* no call yet on this thread */
#define VAL_GPU_HOOK_GPU 1      /* on the GPU */
#define VAL_GPU_HOOK_CPU 2      /* on the CPU, below the threshold */
#define VAL_GPU_HOOK_FALLBACK 3 /* on the CPU after the GPU path failed */
int val_gpu_last_hook_path(void);
/* The library's CPU engine itself: raw register after feeding data[0, len)
 * to state (val_crc32_update_state semantics). engine: 0 = the best this CPU
 * has, 1 = slice-by-16, 2 = carry-less multiply (PCLMULQDQ), 3 = 512-bit
 * carry-less multiply (VPCLMULQDQ + AVX-512); an engine the CPU lacks runs
 * the next simpler one. val_crc32_cpu_engine() = the engine 0 selects. */
uint32_t val_crc32_cpu_update_state(uint32_t state, const void *data, size_t len, int engine);
int val_crc32_cpu_engine(void);
uint32_t val_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* state * x^(8*nbytes) mod P: advance a raw register over nbytes zero bytes. */
uint32_t val_crc32_shift(uint32_t state, uint64_t nbytes);

/* ---- batch frames, device-resident (async on `stream`) ------------------
 * Frame i is the CRC input base[off_i, off_i + len_i):
 *   descriptor mode: d_off[i], d_len[i] (device arrays; stride/flen ignored)
 *   strided mode   : d_off == d_len == NULL, off_i = i*stride, len_i = flen
 * Outputs (device, n entries, any may be NULL):
 *   d_crc[i] = CRC-32 of frame i (the trailer value)
 *   d_hdr[i] = header_crc = CRC-32 of the first min(8, len_i) bytes
 * len_hint (descriptor mode): typical frame length when the batch is
 * uniform (picks the lanes-per-frame geometry directly); 0 = lengths mixed or
 * unknown: frames are binned by length class on the device and each class
 * runs its own geometry (ragged path, no host synchronisation).
 * Lengths may be 0 .. 2^32-1.                                          */
val_status_t val_crc32_frames_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len, uint64_t stride,
                                  uint32_t flen, uint32_t n, uint32_t len_hint, uint32_t *d_crc, uint32_t *d_hdr,
                                  void *stream);

/* RX verify: frame i's stored trailer is the LE32 at base + off_i + len_i.
 * d_ok[i] = 1 if it equals the recomputed CRC else 0 (nullable);
 * *d_nbad (device u32, nullable) is INCREMENTED by the number of mismatches
 * (zero it first; mirrors metrics.crc_errors++). d_crc/d_hdr as above. */
val_status_t val_crc32_verify_frames_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                         uint64_t stride, uint32_t flen, uint32_t n, uint32_t len_hint, uint8_t *d_ok,
                                         uint32_t *d_nbad, uint32_t *d_crc, uint32_t *d_hdr, void *stream);

/* RX verify plus the receiver's rolling file-CRC input as a by-product
 * (reference src/val_receiver.c:794,891,1004-1005, where
 * every in-order DATA payload goes through val_crc32_update_state): as
 * val_crc32_verify_frames_dev, and d_pay[i] (nullable) = the raw register
 * after feeding frame i's payload to a ZERO register. The payload is the CRC
 * input after the 8-byte header and, when flags (byte 1) has
 * VAL_DATA_OFFSET_PRESENT, the 8-byte offset (0 if the frame is shorter).
 * Fold the states into the file CRC with val_crc32_fold_payload_states. */
val_status_t val_crc32_verify_frames_ex_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                            uint64_t stride, uint32_t flen, uint32_t n, uint32_t len_hint,
                                            uint8_t *d_ok, uint32_t *d_nbad, uint32_t *d_crc, uint32_t *d_hdr,
                                            uint32_t *d_pay, void *stream);

/* TX framing on the device: val_frame_data_batch + the trailer CRC +
 * val_frame_put_trailers (include/val_wire.h) in one launch, async on
 * `stream` (the per-packet work of reference src/val_core.c:733-834 for a
 * whole window). All pointers are device pointers. Frame i is laid out byte
 * for byte as the host framer does: the 8-byte header (VAL_PKT_DATA, flags
 * VAL_DATA_OFFSET_PRESENT iff d_include_offset[i] != 0, NULL = every frame;
 * content_len LE16; type_data 0), the LE64 d_file_off[i] when explicit, payload
 * bytes [d_pay_off[i], d_pay_off[i] + d_pay_len[i]) of d_payload, and the LE32
 * CRC-32 of those 8 + content bytes.
 * Placement: d_frame_off[i] when given (val_frame_data_layout computes the
 * host framer's back-to-back stream once on the host), else frame i at
 * i * out_stride (a ring of slots).
 * Outputs (n entries each, any may be NULL; they feed
 * val_crc32_verify_frames_*_dev directly): d_crc_len[i] = 8 + content,
 * d_crc[i] = the trailer value, d_hdr[i] = header_crc as above.
 * Rejected frames: where the host framer refuses the whole batch, a device
 * call has no lengths to look at without a synchronise, so it rejects frame by
 * frame and counts. A frame is rejected when its content exceeds 65535 bytes,
 * in slot mode when 12 + content > out_stride, and when d_pay_len[i] > 0 while
 * d_payload or d_pay_off is NULL: no byte of d_out is written for it,
 * d_crc_len[i] = d_crc[i] = d_hdr[i] = 0, and *d_nrejected (device u32,
 * nullable) is INCREMENTED (zero it first).
 * Only the 12 + content wire bytes of accepted frames are written; every other
 * byte of d_out keeps its value. Only aligned dwords that overlap a frame's
 * payload range are read.
 * d_payload / d_pay_off may be NULL only if every d_pay_len[i] is 0 (the
 * caller's promise: it cannot be checked without a synchronise). d_out must
 * not overlap d_payload and frames must not overlap each other.
 * len_hint: typical CRC-input length (picks the lanes per frame, speed only;
 * 0 = unknown; val_gpu_set_lanes_per_frame forces it).
 * n == 0 returns VAL_OK without a launch; NULL d_out, d_pay_len or d_file_off,
 * or NULL d_frame_off with out_stride < 12, return VAL_ERR_INVALID_ARG before
 * any launch (val_gpu_last_error says which). The call runs on the stream's
 * device (else the device d_out lives on) and keeps no library scratch. */
val_status_t val_frame_data_batch_dev(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint32_t *d_pay_len,
                                      const uint64_t *d_file_off, const uint8_t *d_include_offset, uint32_t n,
                                      uint8_t *d_out, const uint64_t *d_frame_off, uint64_t out_stride,
                                      uint32_t len_hint, uint32_t *d_crc_len, uint32_t *d_crc, uint32_t *d_hdr,
                                      uint32_t *d_nrejected, void *stream);

/* RX delivery on the device, the counterpart of val_frame_data_batch_dev: a
 * window of received frames in HBM goes in, and the call leaves on the device
 * what the reference's receive loop would have produced for it (the trailer
 * check of src/val_core.c:963-993, then the ordering decision, the fwrite and
 * the rolling CRC of src/val_receiver.c:871-895): the payloads at their place
 * in the GPU-resident file d_file, *d_written, the rolling *d_file_state and
 * the per-frame verdicts. Async on `stream`, no host synchronisation. All
 * pointers are device pointers; frames are described as for
 * val_crc32_verify_frames_ex_dev (d_base, d_off, d_len, stride, flen, n,
 * len_hint; descriptor lengths are the caller's and may be 0 .. 2^32-1, not
 * only what the LE16 content_len can say).
 * It is a short pipeline on the stream, not one launch (DESIGN.md section
 * 4.9): a payload may be written only after its own CRC matched and the
 * verdicts of all earlier frames are known.
 *   1. verify: the launches of val_crc32_verify_frames_ex_dev. d_ok[i]
 *      (nullable) and *d_nbad (nullable, INCREMENTED) as there.
 *   2. order: the rule of val_frame_accept (val_wire.h) over the header facts
 *      of val_frame_data_offsets / val_frame_payload_lens, with
 *      W = *d_written. Frame i is accepted iff its trailer matched, it is a
 *      DATA frame, its effective offset (the explicit LE64, or W when implied)
 *      equals W, and W + pay_len <= file_cap (no 64-bit wrap-around). An
 *      accepted frame is delivered at W and advances W by pay_len; every other
 *      frame (corrupt, control, duplicate, gap, too short for its offset) is
 *      skipped and later frames are still judged one by one. d_accept[i]
 *      (nullable) = 1 / 0; *d_naccepted and *d_noverflow (device u32,
 *      nullable) are INCREMENTED by the frames accepted and by the frames
 *      refused by the capacity test alone (zero them first). *d_written = W.
 *      *d_file_state (raw register, nullable) becomes
 *      shift(state, pay_len) ^ pay_state over the accepted frames in order,
 *      i.e. val_crc32_fold_payload_states_at's result.
 *   3. scatter: accepted payload i is copied to d_file + its offset. Bytes of
 *      d_file outside the accepted ranges keep their values (no
 *      read-modify-write of a neighbouring dword); only aligned dwords of
 *      d_base that overlap an accepted payload are read for the copy.
 * d_file must hold file_cap bytes and must not overlap d_base.
 * d_work: the caller's workspace of at least val_frame_unpack_work_bytes(n)
 * bytes, 8-byte aligned (verdicts, payload states, destinations, header
 * facts); its contents after the call are unspecified. The call keeps no
 * library scratch beyond what the verify stage uses per stream.
 * Two calls on one stream chain: the second continues from the first's
 * *d_written and *d_file_state.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when d_off and d_len are not both set or both NULL, d_work is NULL or
 * misaligned, work_bytes is below val_frame_unpack_work_bytes(n), and, with
 * n > 0, when d_file, d_written or d_base is NULL. Otherwise n == 0 returns
 * VAL_OK, launches nothing and changes nothing. The call runs on the stream's
 * device (else the device d_file lives on). */
uint64_t val_frame_unpack_work_bytes(uint32_t n);
val_status_t val_frame_unpack_batch_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                        uint64_t stride, uint32_t flen, uint32_t n, uint32_t len_hint, uint8_t *d_file,
                                        uint64_t file_cap, uint64_t *d_written, uint32_t *d_file_state, uint8_t *d_ok,
                                        uint32_t *d_nbad, uint8_t *d_accept, uint32_t *d_naccepted,
                                        uint32_t *d_noverflow, void *d_work, uint64_t work_bytes, void *stream);

/* RX delivery for many receivers at once: one window that holds frames of
 * n_files transfers, delivered in one asynchronous call. For every file it
 * leaves what val_frame_unpack_batch_dev, called on that file's frames alone,
 * would have left, bit for bit: the file bytes, written, the state, ok[],
 * accept[] and the counters (the ordering decision of
 * src/val_receiver.c:871-895 once per file). The pipeline is that call's with
 * one launch per stage: one verify over all n frames, one parse, one order
 * launch whose workgroups each take whole files (the rule is sequential only
 * within a file), one scatter over all n frames. All pointers are device
 * pointers; nothing is synchronised.
 * Frames are described as for val_frame_unpack_batch_dev (d_base, d_off,
 * d_len, stride, flen, n, len_hint; any length 0 .. 2^32-1; len_hint 0 = the
 * ragged verify path). The caller groups the DESCRIPTORS by file: file s owns
 * frames [d_first[s], d_first[s+1]) of the n (d_first has n_files + 1
 * entries); the frames themselves may lie anywhere in d_base, in any order.
 * Per file s, with W = d_written[s] and cap = d_file_cap[s], the rule of
 * val_frame_accept runs over its frames in index order; accepted payloads are
 * copied to d_file_ptr[s] + W (d_file_ptr[s] is the device address of a file
 * of at least d_file_cap[s] bytes); d_written[s] is updated;
 * d_file_state[s] (raw registers, array nullable) folds
 * shift(state, pay_len) ^ pay_state over the file's accepted frames;
 * d_naccepted[s], d_noverflow[s] and d_file_nbad[s] (frames of file s whose
 * trailer did not match) are INCREMENTED (arrays nullable; zero them first).
 * d_ok[i] and d_accept[i] (n entries, nullable) and *d_nbad (whole batch,
 * nullable, INCREMENTED) are as in the single-file call. Only bytes of
 * accepted ranges are written, per file, with no read-modify-write of a
 * neighbouring dword.
 * The segment boundaries live on the device and cannot be checked without a
 * synchronise, so they are made safe rather than trusted: file s owns
 * [min(d_first[s], n), min(max(d_first[s+1], d_first[s]), n)); a decreasing
 * pair is an empty file, which changes nothing of that file's entries. A frame
 * that no file owns is still verified (d_ok[i], *d_nbad), gets
 * d_accept[i] = 0 and is never delivered. Overlapping segments are the
 * caller's error: a frame owned twice may land in either file, and d_accept[i]
 * may speak for either; it never lands outside that file's capacity and no
 * out-of-bounds access happens. Files must not overlap each other or d_base.
 * d_work: val_frame_unpack_work_bytes(n) bytes, 8-byte aligned, as in the
 * single-file call; there is no per-file workspace and no library scratch
 * beyond what the verify stage keeps per stream. Two calls on one stream
 * chain, file by file.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when d_off and d_len are not both set or both NULL, d_work is NULL or
 * misaligned, work_bytes is below val_frame_unpack_work_bytes(n), and, with
 * n > 0 and n_files > 0, when d_first, d_file_ptr, d_file_cap, d_written or
 * d_base is NULL. Otherwise n == 0 or n_files == 0 returns VAL_OK, launches
 * nothing and changes nothing. The call runs on the stream's device (else the
 * device d_written lives on). */
val_status_t val_frame_unpack_files_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                        uint64_t stride, uint32_t flen, uint32_t n, uint32_t len_hint, uint32_t n_files,
                                        const uint32_t *d_first, const uint64_t *d_file_ptr, const uint64_t *d_file_cap,
                                        uint64_t *d_written, uint32_t *d_file_state, uint32_t *d_naccepted,
                                        uint32_t *d_noverflow, uint32_t *d_file_nbad, uint8_t *d_ok, uint32_t *d_nbad,
                                        uint8_t *d_accept, void *d_work, uint64_t work_bytes, void *stream);

/* RX scan on the device, the step in front of the verify and unpack calls:
 * received byte streams that lie in HBM are walked into frame descriptors
 * without a host round trip. It replaces, for a whole window of every
 * connection, the per-packet receive framing of the reference (the header
 * read that tells the receiver how many bytes the frame has, and the
 * content_len check of src/val_core.c:915-921), i.e. val_frame_scan (val_wire.h)
 * once per stream. Async on `stream`; all pointers are device pointers;
 * nothing is synchronised and no library scratch is kept.
 * Stream s is d_base[d_stream_off[s], d_stream_off[s] + d_stream_len[s]), one
 * per connection. For each stream the call leaves exactly what
 * val_frame_scan(stream, len, mtu, max_frames, ...) returns for those bytes:
 * d_nframes[s] the frame count, d_consumed[s] the bytes consumed (relative to
 * the stream start: the bytes behind them are carried into the next window),
 * d_status[s] VAL_OK or VAL_ERR_PROTOCOL (each array nullable), and the
 * frames' (frame_off, crc_len) pairs with frame_off made absolute in d_base
 * by adding d_stream_off[s]. The stop rules are the host's, in its order:
 * max_frames reached; fewer than 8 bytes left; content_len > mtu - 12
 * (VAL_ERR_PROTOCOL; the frames before it are kept); the frame is incomplete.
 * Layout: the descriptors of all streams are compacted in stream order into
 * d_frame_off / d_crc_len (n_streams * max_frames entries each);
 * d_first[s] is the exclusive prefix sum of the counts and d_first[n_streams]
 * the total (n_streams + 1 entries), so d_frame_off, d_crc_len and d_first
 * feed val_frame_unpack_files_dev unchanged as d_off, d_len and d_first with
 * n_files = n_streams. Entries [total, n_streams * max_frames) are set to
 * (0, 0).
 * Without reading the total back: pass n = n_streams * max_frames to
 * val_frame_unpack_files_dev. By its clamping no file owns the padding
 * entries; they are verified as zero-length frames at d_base and never
 * delivered. Two conditions: such a caller passes d_nbad = NULL and reads the
 * per-file d_file_nbad[], because the whole-batch counter would count the
 * padding too (d_ok[i] of a padding entry says nothing); and d_base must hold
 * at least 4 bytes, the trailer a zero-length frame at offset 0 is checked
 * against.
 * Only aligned dwords that overlap [stream start, stream start + len) are
 * read, and of every header only the dwords that hold bytes 2..3. Positions
 * are 64-bit. The walk advances 64 frames per memory round trip through runs
 * of equal-size frames (up to 1,024 where a workgroup walks the stream,
 * val_gpu_set_scan_front) and one frame per round trip where sizes alternate
 * (DESIGN.md section 4.10).
 * d_work: val_frame_scan_work_bytes(n_streams, max_frames) bytes, 8-byte
 * aligned (every stream's descriptors before compaction, the counts); its
 * contents after the call are unspecified. It must not overlap the outputs.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when mtu < 12, n_streams * max_frames overflows 32 bits, d_work is
 * NULL or misaligned, work_bytes is below val_frame_scan_work_bytes, and, with
 * n_streams > 0 and max_frames > 0, when d_stream_off, d_stream_len,
 * d_frame_off, d_crc_len, d_first or d_base is NULL. Otherwise n_streams == 0
 * returns VAL_OK and launches nothing; max_frames == 0 is valid: all counts,
 * d_consumed and d_status are 0 and d_first (when given) is all zeros. The
 * call runs on the stream's device (else the device d_base lives on). */
uint64_t val_frame_scan_work_bytes(uint32_t n_streams, uint32_t max_frames);
val_status_t val_frame_scan_streams_dev(const uint8_t *d_base, const uint64_t *d_stream_off,
                                        const uint64_t *d_stream_len, uint32_t n_streams, uint64_t mtu,
                                        uint32_t max_frames, uint64_t *d_frame_off, uint32_t *d_crc_len,
                                        uint32_t *d_first, uint32_t *d_nframes, uint64_t *d_consumed,
                                        int32_t *d_status, void *d_work, uint64_t work_bytes, void *stream);

/* TX window fill on the device, the step in front of val_frame_data_batch_dev
 * and the send-side counterpart of the scan call: the send state of n_files
 * transfers whose files lie in HBM goes in, and the call leaves in HBM the wire
 * bytes the reference sender's window-fill loop would have sent for each of
 * them (src/val_sender.c:822-841 with send_data_packet, :258-315, and the
 * explicit-offset rule of :833), trailers included, plus the descriptors the
 * verify, scan and unpack calls consume. It replaces, for a whole window of
 * every transfer, the host's per-transfer plan and the upload of
 * val_frame_data_batch_dev's per-frame inputs. Async on `stream`; all pointers
 * are device pointers; nothing is synchronised and no library scratch is kept.
 * Addressing: file s is d_file_size[s] bytes at d_payload + d_file_pos[s],
 * which is val_frame_data_batch_dev's addressing of a payload byte; the sum
 * wraps modulo 2^64 by definition, so any device address can be expressed
 * against any non-NULL d_payload.
 * Per transfer s the call applies val_frame_fill_window (val_wire.h) with
 * next = d_next[s], last_acked = d_last_acked[s], file_size = d_file_size[s],
 * mtu, budget = min(d_budget[s], max_frames) (d_budget nullable = max_frames)
 * and out_cap = d_stream_cap[s]. The frames it makes are written back to back
 * from d_out + d_stream_off[s], byte for byte as val_frame_data_batch_dev
 * writes them; d_next[s] becomes the rule's new next; d_nframes[s] the frame
 * count and d_stream_len[s] the bytes used (each array nullable). With
 * last_acked <= next only a call's first frame can be explicit
 * (next == last_acked), so two calls on one stream chain: the second
 * continues at the first's next with implied offsets. A go-back-N restart is
 * d_next[s] = d_last_acked[s].
 * Layout of the per-frame outputs, the scan call's: compacted in transfer
 * order into arrays of n_files * max_frames entries; d_first[s] (n_files + 1
 * entries) is the exclusive prefix sum of the counts and d_first[n_files] the
 * total. d_frame_off[i] is the frame's start, absolute in d_out;
 * d_crc_len[i] = 8 + content, d_crc[i] the trailer value, d_hdr[i] the
 * header_crc (each nullable). Entries [total, n_files * max_frames) of all
 * four are 0. d_out, d_frame_off, d_crc_len and d_first feed
 * val_crc32_verify_frames_dev and val_frame_unpack_files_dev unchanged (with
 * n = n_files * max_frames as described for the scan call); the wire bytes of
 * transfer s, d_stream_off[s] and d_stream_len[s], feed
 * val_frame_scan_streams_dev.
 * Only the wire bytes of the frames made are written; every other byte of
 * d_out keeps its value. Only aligned dwords that overlap a payload range are
 * read from the files (val_frame_data_batch_dev's guarantees: the frames are
 * built by the same kernel). Streams must not overlap each other or the files;
 * that is the caller's promise.
 * It is a short pipeline on the stream: a count
 * launch of one thread per transfer (the rule is closed-form: every frame that
 * does not end the file has wire size mtu), the prefix sum, a launch that
 * writes val_frame_data_batch_dev's per-frame inputs into the workspace, and
 * that call's launch over all n_files * max_frames entries, lanes picked from
 * len_hint = mtu - 4 (val_gpu_set_lanes_per_frame forces them).
 * d_work: val_frame_fill_work_bytes(n_files, max_frames) bytes, 8-byte
 * aligned; its contents after the call are unspecified. It must not overlap
 * the inputs or the outputs.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when mtu < 21 or mtu > 65547 (val_frame_fill_window's bounds),
 * n_files * max_frames overflows 32 bits, d_work is NULL or misaligned,
 * work_bytes is below val_frame_fill_work_bytes, and, with n_files > 0 and
 * max_frames > 0, when d_payload, d_file_pos, d_file_size, d_next,
 * d_last_acked, d_out, d_stream_off, d_stream_cap, d_first or d_frame_off is
 * NULL. Otherwise n_files == 0 returns VAL_OK and launches nothing;
 * max_frames == 0 is valid: d_nframes and d_stream_len are 0, d_first (when
 * given) is all zeros and d_next is unchanged. The call runs on the stream's
 * device (else the device d_out lives on). */
uint64_t val_frame_fill_work_bytes(uint32_t n_files, uint32_t max_frames);
val_status_t val_frame_fill_files_dev(const uint8_t *d_payload, const uint64_t *d_file_pos,
                                      const uint64_t *d_file_size, uint64_t *d_next, const uint64_t *d_last_acked,
                                      const uint32_t *d_budget, uint32_t n_files, uint64_t mtu, uint32_t max_frames,
                                      uint8_t *d_out, const uint64_t *d_stream_off, const uint64_t *d_stream_cap,
                                      uint64_t *d_stream_len, uint32_t *d_nframes, uint32_t *d_first,
                                      uint64_t *d_frame_off, uint32_t *d_crc_len, uint32_t *d_crc, uint32_t *d_hdr,
                                      void *d_work, uint64_t work_bytes, void *stream);

/* The receiver's answers to a delivered window, on the device: the DATA_ACK /
 * DATA_NAK frames the reference's receive loop sends for the DATA frames of a
 * window (src/val_receiver.c:871-1000, encoded as src/val_core.c:775-811 with
 * the trailer of :828-834), for n_files transfers in one asynchronous call.
 * It runs on the stream right after val_frame_unpack_files_dev, over the same
 * window and that call's results. Async on `stream`; all pointers are device
 * pointers; nothing is synchronised and no library scratch is kept.
 * Inputs: the frame descriptors as there (d_base, d_off, d_len, stride, flen,
 * n, n_files, d_first, clamped the same way, so a frame that no file owns gets
 * no response); that call's d_ok[] and d_accept[] (both required) and its
 * d_written[], the positions AFTER delivery; d_total[s], the incoming file's
 * size; ack_stride (the handshake's ack_stride_packets) and d_since[s], the
 * frames accepted since the last stride ACK (in/out; may be NULL when
 * ack_stride == 0, which neither reads nor writes it).
 * Per file s the call writes the wire bytes of exactly the responses
 * val_frame_respond_window (val_wire.h) lists for that file's frames, each as
 * val_frame_put_response lays it out, trailer included, back to back from
 * d_out + d_resp_off[s]; d_resp_len[s] = the bytes used, d_nresp[s] = the
 * frames written (both set; 0 for a file without frames); d_ndropped[s]
 * (nullable) is INCREMENTED by the responses that did not fit.
 * Capacity: with pos_r the sum of the wire sizes of the file's earlier
 * responses, response r is written iff pos_r + size_r <= d_resp_cap[s]. That
 * keeps a prefix; every later response is dropped and counted.
 * val_frame_respond_bytes_max(frames) = 40 * frames bounds a file's stream (a
 * gap answers with a 24-byte NAK and an ACK of up to 16 bytes).
 * Only the wire bytes of kept responses are written; every other byte of d_out
 * keeps its value. Of each frame only the header dwords and, for an explicit
 * DATA frame, its offset dwords are read. d_out, d_resp_off and d_resp_len
 * feed val_frame_scan_streams_dev unchanged.
 * No position before the unpack call exists in HBM: the position in front of
 * frame i is d_written[s] minus the payload bytes of the file's accepted
 * frames at indices >= i. A DATA frame with d_accept[i] == 0, d_ok[i] != 0 and
 * an offset (explicit or implied) equal to that position was refused by
 * capacity alone and is silent.
 * It is a short pipeline on the stream: the header
 * facts grid-wide, the rule as segmented scans (workgroups take whole files in
 * turn, 1,024 or 256 frames per chunk), and the response frames grid-wide, each
 * trailer computed where its frame is written.
 * d_work: val_frame_respond_work_bytes(n) bytes, 8-byte aligned (the header
 * facts and every frame's planned responses); its contents after the call are
 * unspecified. Overlapping segments are the caller's error: a frame owned
 * twice is answered in either file's stream, never outside that stream's
 * capacity. Response streams must not overlap each other.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when d_off and d_len are not both set or both NULL, d_work is NULL or
 * misaligned, work_bytes is below val_frame_respond_work_bytes(n), and, with
 * n > 0 and n_files > 0, when d_first, d_ok, d_accept, d_written, d_total,
 * d_out, d_resp_off, d_resp_cap, d_resp_len, d_nresp or d_base is NULL, or
 * d_since is NULL with ack_stride > 0. Otherwise n == 0 or n_files == 0
 * returns VAL_OK, launches nothing and changes nothing (d_resp_len included).
 * The call runs on the stream's device (else the device d_written lives on). */
uint64_t val_frame_respond_bytes_max(uint64_t frames);
uint64_t val_frame_respond_work_bytes(uint32_t n);
val_status_t val_frame_respond_files_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                         uint64_t stride, uint32_t flen, uint32_t n, uint32_t n_files,
                                         const uint32_t *d_first, const uint8_t *d_ok, const uint8_t *d_accept,
                                         const uint64_t *d_written, const uint64_t *d_total, uint32_t ack_stride,
                                         uint32_t *d_since, uint8_t *d_out, const uint64_t *d_resp_off,
                                         const uint64_t *d_resp_cap, uint64_t *d_resp_len, uint32_t *d_nresp,
                                         uint32_t *d_ndropped, void *d_work, uint64_t work_bytes, void *stream);

/* The sender's handling of the answers, on the device: a window of received
 * DATA_ACK / DATA_NAK frames of n_files transfers (what
 * val_frame_scan_streams_dev described) moves every transfer's d_last_acked[s]
 * and d_next[s] as wait_for_window_ack does (reference
 * src/val_sender.c:404-555), in one asynchronous call. Async on `stream`; all
 * pointers are device pointers; nothing is synchronised.
 * Frames are described as for val_frame_unpack_files_dev (d_base, d_off,
 * d_len, stride, flen, n, len_hint, n_files, d_first, clamped the same way).
 * The pipeline is the verify launches of val_crc32_verify_frames_dev (d_ok[i]
 * nullable, *d_nbad nullable and INCREMENTED, as in the unpack call), then one
 * apply launch: per transfer s, d_last_acked[s] and d_next[s] become exactly
 * what val_frame_apply_acks (val_wire.h) leaves for that transfer's frames,
 * with val_frame_ack_offsets' kinds and offsets, the trailer verdicts as ok[]
 * and file_size = d_file_size[s]; d_nretrans[s] and d_file_nbad[s] (arrays
 * nullable; zero them first) are INCREMENTED by the rule's retransmits and CRC
 * errors. The rule reduces to a maximum and an "any restart" per transfer, so
 * the launch is a reduction in the respond call's per-file layout. A transfer
 * without frames keeps its entries; a frame that no transfer owns is verified
 * and otherwise ignored. d_next and d_last_acked then feed
 * val_frame_fill_files_dev unchanged. Timeouts stay the host's: a go-back-N
 * restart after silence is d_next[s] = d_last_acked[s].
 * Of each frame the verify stage reads the CRC input and the trailer; the
 * apply launch reads the two header dwords and the dword behind them when it
 * belongs to the CRC input.
 * d_work: val_frame_apply_acks_work_bytes(n) bytes, 8-byte aligned (the
 * verdicts when d_ok is NULL); no library scratch beyond what the verify stage
 * keeps per stream.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when d_off and d_len are not both set or both NULL, d_work is NULL or
 * misaligned, work_bytes is below val_frame_apply_acks_work_bytes(n), and,
 * with n > 0 and n_files > 0, when d_first, d_file_size, d_last_acked, d_next
 * or d_base is NULL. Otherwise n == 0 or n_files == 0 returns VAL_OK, launches
 * nothing and changes nothing. The call runs on the stream's device (else the
 * device d_last_acked lives on). */
uint64_t val_frame_apply_acks_work_bytes(uint32_t n);
val_status_t val_frame_apply_acks_files_dev(const uint8_t *d_base, const uint64_t *d_off, const uint32_t *d_len,
                                            uint64_t stride, uint32_t flen, uint32_t n, uint32_t len_hint,
                                            uint32_t n_files, const uint32_t *d_first, const uint64_t *d_file_size,
                                            uint64_t *d_last_acked, uint64_t *d_next, uint32_t *d_nretrans,
                                            uint32_t *d_file_nbad, uint8_t *d_ok, uint32_t *d_nbad, void *d_work,
                                            uint64_t work_bytes, void *stream);

/* CRC-32 of one byte window of each of n_files GPU-resident files, in one
 * device call: the many-files form of val_crc32_region_dev, for callers whose
 * file sizes and windows exist only in HBM (a receiver that has just delivered
 * a window with val_frame_unpack_files_dev has its files' sizes in d_written).
 * Async on `stream`; all pointers are device pointers; nothing is synchronised
 * and no library scratch is kept: the per-file accumulators and arrival counts
 * live in the caller's d_work.
 * For each file s, d_crc[s] is the finalized CRC-32 (seed 0xFFFFFFFF, final
 * XOR: what the reference's val_internal_crc32_region returns) of bytes
 * [d_win_off[s], d_win_off[s] + d_win_len[s]) of the file of d_file_size[s]
 * bytes whose byte 0 is at device address d_file_ptr[s]; an empty window
 * gives 0. Window starts and ends have any byte alignment.
 * Windows are made safe, not trusted: a window with
 * d_win_off[s] + d_win_len[s] > d_file_size[s] (judged without 64-bit
 * wrap-around) or d_win_len[s] > max_len gets d_status[s] =
 * VAL_ERR_INVALID_ARG and d_crc[s] = 0, and no byte of it is read; every
 * other file gets d_status[s] = VAL_OK (d_status nullable). That a file's
 * d_file_size bytes at d_file_ptr are readable is the caller's promise.
 * max_len is the caller's bound on any window and fixes the geometry on the
 * host: 0 .. 2^32 (a VERIFY request carries 32 bits). max_len == 0 is valid:
 * only empty windows are VAL_OK.
 * Reads: only aligned dwords that overlap an accepted window are read from a
 * file (whole 64-byte units inside it, its first and last dwords, or, for a
 * window of fewer than 4 bytes, those bytes); nothing is written but the
 * outputs and d_work.
 * It is a short pipeline on the stream: a count
 * launch of one thread per file that validates the window and counts its
 * chunks, the prefix sum, and a hash launch in a persistent grid over all
 * chunks of all files, so one long window among many short ones still spreads
 * over the machine. The chunk size is one for the call, 2^k0 bytes with k0 in
 * 12..16, chosen from max_len and n_files (val_gpu_plan_file_windows shows it;
 * val_gpu_set_file_window_chunk forces it). Chunk states are folded into the
 * file's accumulator with device-scope atomics; the last chunk of a file to
 * arrive writes its outputs; no workgroup waits for another, and the result is
 * bit-exact whatever the arrival order.
 * d_work: val_file_windows_work_bytes(n_files) bytes, 8-byte aligned. The call
 * zeroes what it needs itself: the contents on entry are unspecified, as they
 * are after the call, and calls on one stream may share one d_work. It must
 * not overlap the inputs or the outputs.
 * Returns VAL_ERR_INVALID_ARG before any launch (val_gpu_last_error says
 * which) when d_work is NULL or misaligned, work_bytes is below
 * val_file_windows_work_bytes(n_files), max_len is above 2^32, n_files times
 * the chunks of a max_len window (at 64 KiB chunks) overflows 32 bits, and,
 * with n_files > 0, when d_file_ptr, d_file_size, d_win_off, d_win_len or
 * d_crc is NULL. Otherwise n_files == 0 returns VAL_OK and launches nothing.
 * The call runs on the stream's device (else the device d_work lives on). */
uint64_t val_file_windows_work_bytes(uint32_t n_files);
val_status_t val_crc32_file_windows_dev(const uint64_t *d_file_ptr, const uint64_t *d_file_size,
                                        const uint64_t *d_win_off, const uint64_t *d_win_len, uint32_t n_files,
                                        uint64_t max_len, uint32_t *d_crc, int32_t *d_status,
                                        void *d_work, uint64_t work_bytes, void *stream);

/* The VAL_RESUME_TAIL handshake of n_files GPU-resident files, three calls
 * thin over that pipeline: each is the count launch with one of the rules of
 * val_wire.h applied per file, the prefix sum, the hash launch, and the finish
 * in the last chunk to arrive. They share val_crc32_file_windows_dev's
 * addressing (d_file_ptr), workspace (val_file_windows_work_bytes(n_files)),
 * read guarantee, stream and device semantics, and its argument checks: d_work
 * and work_bytes, max_len, the chunk product, and with n_files > 0 every
 * pointer not called nullable below; n_files == 0 returns VAL_OK and launches
 * nothing. Actions are val_resume_action_t values and results val_status_t
 * values, both as int32.
 *
 * val_resume_tail_files_dev, the receiver's proposal: per file
 * val_resume_tail_window(d_existing[s], d_incoming[s], tail_cap_bytes,
 * min_verify_bytes, mismatch_skip) gives d_action[s], d_resume_off[s] and
 * d_verify_len[s]; for VAL_RESUME_VERIFY_FIRST files d_verify_crc[s] is the
 * CRC of the last d_verify_len[s] bytes of the local file of d_existing[s]
 * bytes, and 0 for every other action. d_existing can be the d_written of
 * val_frame_unpack_files_dev on the same stream, with no read-back. max_len is
 * derived on the host, max(the clamped cap, min_verify_bytes); a
 * min_verify_bytes above 2^32 is refused. All outputs are required.
 *
 * val_resume_request_files_dev, the sender's answer, over its own copies of
 * the files: for files with d_action[s] == VAL_RESUME_VERIFY_FIRST for which
 * val_resume_request_window(d_resume_off[s], d_verify_len[s]) gives a
 * non-empty window, d_req_off[s] and d_req_len[s] are that window and
 * d_req_crc[s] its CRC in the file of d_file_size[s] bytes; d_status[s]
 * (nullable) is as in the generic call (a window outside the file or above
 * max_len: VAL_ERR_INVALID_ARG and d_req_crc[s] = 0). For every other file
 * d_req_off[s] = d_resume_off[s], d_req_len[s] = d_req_crc[s] = 0,
 * d_status[s] = VAL_OK, and nothing is read.
 *
 * val_resume_check_files_dev, the receiver's check of the VERIFY request: for
 * files with d_action[s] == VAL_RESUME_VERIFY_FIRST (d_action NULL: every
 * file), the CRC of [d_req_off[s], d_req_off[s] + d_req_len[s]) of the local
 * file of d_existing[s] bytes goes to d_local_crc[s] (nullable; what the
 * VERIFY response carries), and val_resume_verdict(window_ok, that CRC,
 * d_req_crc[s], mismatch_skip, d_rec_resume_off[s], d_incoming[s]) gives
 * d_result[s] and d_written[s], the offset the transfer resumes at. window_ok
 * is 0 when the window does not lie inside the local file or exceeds max_len;
 * then nothing is read and d_local_crc[s] = 0. Files with any other action are
 * left untouched in every output. d_written then feeds the next
 * val_frame_unpack_files_dev call unchanged, and d_next / d_last_acked of a
 * val_frame_fill_files_dev call on the peer.
 *
 * Out of scope: the rolling d_file_state of a resumed file (it needs the CRC
 * of the whole prefix, not of a window: val_crc32_file_windows_dev with the
 * window [0, d_written[s]) gives its finalized form); the NEVER and
 * SKIP_EXISTING modes, which hash nothing; and building or parsing the
 * RESUME_RESP and VERIFY control frames, whose codecs exist on the host
 * (val_wire.h). */
val_status_t val_resume_tail_files_dev(const uint64_t *d_file_ptr, const uint64_t *d_existing,
                                       const uint64_t *d_incoming, uint32_t n_files, uint64_t tail_cap_bytes,
                                       uint64_t min_verify_bytes, int mismatch_skip, int32_t *d_action,
                                       uint64_t *d_resume_off, uint64_t *d_verify_len, uint32_t *d_verify_crc,
                                       void *d_work, uint64_t work_bytes, void *stream);
val_status_t val_resume_request_files_dev(const uint64_t *d_file_ptr, const uint64_t *d_file_size,
                                          const int32_t *d_action, const uint64_t *d_resume_off,
                                          const uint64_t *d_verify_len, uint32_t n_files, uint64_t max_len,
                                          uint64_t *d_req_off, uint32_t *d_req_len, uint32_t *d_req_crc,
                                          int32_t *d_status, void *d_work, uint64_t work_bytes, void *stream);
val_status_t val_resume_check_files_dev(const uint64_t *d_file_ptr, const uint64_t *d_existing,
                                        const uint64_t *d_incoming, const int32_t *d_action,
                                        const uint64_t *d_req_off, const uint32_t *d_req_len,
                                        const uint32_t *d_req_crc, const uint64_t *d_rec_resume_off, uint32_t n_files,
                                        uint64_t max_len, int mismatch_skip, uint32_t *d_local_crc, int32_t *d_result,
                                        uint64_t *d_written, void *d_work, uint64_t work_bytes, void *stream);

/* Region CRC of one long device buffer: *d_state_out = raw register after
 * feeding d_ptr[0, len) to `state_in` (val_crc32_update_state semantics;
 * finalize with ^0xFFFFFFFF). One launch at any length: windows up to 8
 * KiB are one 64-lane frame; longer ones are chunked over the whole machine
 * and folded inside the same launch through a 128-byte library-owned device
 * accumulator kept per stream (calls on one stream are ordered by it; calls
 * on different streams use different accumulators; hipStreamPerThread is
 * keyed per calling thread). The call runs on the stream's device (else the
 * device d_ptr lives on). */
val_status_t val_crc32_region_dev(const uint8_t *d_ptr, uint64_t len, uint32_t state_in, uint32_t *d_state_out,
                                  void *stream);
/* Scratch bytes the region call needs for a given length (informational). */
uint64_t val_crc32_region_scratch_bytes(uint64_t len);

/* ---- batch frames, host memory (synchronous; H2D + kernel + D2H, or the
 * CPU engine below val_gpu_host_batch_min_bytes) ---------------------------
 * base_len bounds every frame: off[i] + len[i] (+4 for verify) <= base_len,
 * else VAL_ERR_INVALID_ARG. off/len NULL = strided mode as above.
 * Frames travel H2D in chunks of whole frames on a copy stream while the
 * previous chunk is hashed (descriptor batches chunk when their offsets are
 * non-decreasing). A pinned `base` (val_gpu_host_alloc, hipHostMalloc or
 * hipHostRegister) is copied by DMA in place; pageable memory goes through
 * two internal pinned bounce buffers (host memcpy, val_gpu_host_copy_threads).
 * Mixed-length descriptor batches take the device-binned ragged path.   */
val_status_t val_crc32_frames_host(const uint8_t *base, uint64_t base_len, const uint64_t *off, const uint32_t *len,
                                   uint64_t stride, uint32_t flen, uint32_t n, uint32_t *crc, uint32_t *hdr);
val_status_t val_crc32_verify_frames_host(const uint8_t *base, uint64_t base_len, const uint64_t *off,
                                          const uint32_t *len, uint64_t stride, uint32_t flen, uint32_t n, uint8_t *ok,
                                          uint32_t *nbad);

/* Host batches whose CRC input totals fewer bytes than this are answered by
 * this library's CPU engine instead of the GPU, with identical outputs: a
 * host batch on the GPU pays a launch, a completion wait and PCIe for every
 * byte, and below the measured crossover one CPU core
 * is faster. -1 = VAL_GPU_HOST_BATCH_MIN_BYTES from the environment (read
 * once), else the built-in default, which depends on the batch's mean CRC
 * input per frame: 64 MiB from 4 KiB frames up, 32 MiB below (the getter
 * reports the former); 0 = always the GPU. Such batches need no device and
 * are counted by val_gpu_cpu_batch_count. */
void val_gpu_set_host_batch_min_bytes(int64_t bytes);
uint64_t val_gpu_host_batch_min_bytes(void);
/* The threshold a batch whose mean CRC input per frame is mean_len bytes is
 * held to (what val_crc32_frames_host applies to it). */
uint64_t val_gpu_host_batch_min_bytes_for(uint64_t mean_len);
uint64_t val_gpu_cpu_batch_count(void);
/* Threads the CPU engine uses for one such batch: the calling thread plus
 * threads - 1 helpers over byte-balanced frame ranges, at most one thread
 * per 4 MiB of CRC input (default 1), never more than the process's CPU
 * budget (its affinity set capped by the cgroup CPU quota). */
void val_gpu_set_host_cpu_threads(uint32_t threads);
/* The *_host_multi calls decide CPU or GPU once for the whole batch: below
 * val_gpu_host_batch_min_bytes() * T / N_eff bytes of CRC input, with T the
 * CPU engine's threads, the CPU engine answers it.
 * N_eff = N, the distinct devices the shards land on, for pinned input;
 * pageable input also passes through host bounce copies that all shards
 * share within the process's CPU budget, so N_eff = min(N, the measured
 * aggregate bounce-copy rate / one GPU's pageable rate). Returns that
 * threshold for `devices` devices and pageable input (_ex: pinned or not,
 * and a batch's mean CRC input per frame). */
uint64_t val_gpu_host_multi_min_bytes(int devices);
uint64_t val_gpu_host_multi_min_bytes_ex(int devices, int pinned, uint64_t mean_len);

/* Host-memory form of val_crc32_verify_frames_ex_dev (pay: n entries, nullable). */
val_status_t val_crc32_verify_frames_ex_host(const uint8_t *base, uint64_t base_len, const uint64_t *off,
                                             const uint32_t *len, uint64_t stride, uint32_t flen, uint32_t n,
                                             uint8_t *ok, uint32_t *nbad, uint32_t *pay);
/* The receiver's rolling CRC over frames 0..n-1 in order, stopping before the
 * first frame with ok[i] == 0 (ok nullable = all): for each frame
 * state = shift(state, pay_len[i]) ^ pay_state[i], i.e.
 * val_crc32_update_state(state, payload_i) without touching the bytes again.
 * The caller passes only in-order DATA frames (each payload starts where the
 * previous one ended); for a window that may hold duplicates, gaps or control
 * frames use val_crc32_fold_payload_states_at. *n_folded (nullable) = frames
 * folded. Host only (no GPU call). */
uint32_t val_crc32_fold_payload_states(uint32_t state, const uint32_t *pay_state, const uint32_t *pay_len,
                                       const uint8_t *ok, uint32_t n, uint32_t *n_folded);
/* The same fold with the receiver's ordering rule (reference
 * src/val_receiver.c:871-891): file_off[i] from val_frame_data_offsets
 * (val_wire.h). A frame is folded, and *written advanced by its payload,
 * only when it is a DATA frame with ok[i] != 0 whose effective offset
 * (file_off[i], or *written for VAL_FRAME_OFFSET_IMPLIED) equals *written;
 * duplicates (earlier offsets) and gaps (later ones) are skipped and the
 * frames after them are still judged one by one, as the receiver does.
 * *n_folded (nullable) = frames folded. Host only. */
uint32_t val_crc32_fold_payload_states_at(uint32_t state, const uint32_t *pay_state, const uint32_t *pay_len,
                                          const uint64_t *file_off, const uint8_t *ok, uint32_t n, uint64_t *written,
                                          uint32_t *n_folded);

/* ---- several GPUs in one process ----------------------------------------
 * The *_host batches above split into ndev shards (ndev <= 0: one per
 * visible device): contiguous frame ranges balanced by CRC-input bytes
 * (val_shard_frames), one host thread per shard running the single-device
 * path on device (shard % device count);
 * outputs are disjoint ranges of crc/hdr/ok, nbad is the sum. No collective
 * and no peer copies: frames are independent.                           */
val_status_t val_crc32_frames_host_multi(const uint8_t *base, uint64_t base_len, const uint64_t *off,
                                         const uint32_t *len, uint64_t stride, uint32_t flen, uint32_t n, uint32_t *crc,
                                         uint32_t *hdr, int ndev);
val_status_t val_crc32_verify_frames_host_multi(const uint8_t *base, uint64_t base_len, const uint64_t *off,
                                                const uint32_t *len, uint64_t stride, uint32_t flen, uint32_t n,
                                                uint8_t *ok, uint32_t *nbad, int ndev);
/* Raw register after feeding the host window data[0, len) to state_in, the
 * window cut into ndev 4 KiB-aligned byte ranges hashed on devices
 * (range % device count) and
 * folded with the GF(2) shift (val_crc32_update_state semantics). */
val_status_t val_crc32_region_host_multi(const void *data, uint64_t len, uint32_t state_in, uint32_t *state_out,
                                         int ndev);
/* [*start, *start + *count) = the frames shard `rank` of `world` owns:
 * contiguous, balanced by len[] (NULL: by count). Host only. */
void val_shard_frames(uint32_t n, const uint32_t *len, uint32_t world, uint32_t rank, uint32_t *start,
                      uint32_t *count);
/* Fold k partial raw states in order: state[0] carries the initial register,
 * state[i] (i >= 1) covers nbytes[i] bytes from a zero register.
 * acc = state[0]; acc = shift(acc, nbytes[i]) ^ state[i]. Host only. */
uint32_t val_crc32_fold_partials(const uint32_t *state, const uint64_t *nbytes, uint32_t k);

/* ---- pinned host staging ------------------------------------------------
 * Page-locked host memory for frame windows (e.g. the TX window staging
 * buffer of INTEGRATION.md section 3): the *_frames_host calls copy it by DMA
 * without a bounce. NULL on failure (val_gpu_last_error). */
void *val_gpu_host_alloc(size_t bytes);
void val_gpu_host_free(void *p);
/* Host threads one pageable-to-pinned copy of `bytes` uses when
 * `concurrent_copies` run at once (one per device in the *_host_multi
 * calls): one per 4 MiB, at most 8, and all copies together within the
 * process's CPU affinity set. */
uint32_t val_gpu_host_copy_threads(uint64_t bytes, uint32_t concurrent_copies);
/* Measurement of the pageable half of the host path, with no device work:
 * `copies` concurrent copy streams (as the shards of a *_host_multi call),
 * each copying `bytes` from resident pageable memory into its own bounce
 * buffer `reps` times through the library's own bounce copy (its thread
 * policy above). pinned_dst = 1: page-locked destinations (hipHostMalloc, as
 * the real bounce buffers); 0: malloc'd ones (no HIP runtime needed).
 * *gbs = copies * reps * bytes / the span from the common start to the last
 * copy's end, in GB/s. DESIGN.md section 1.3 folds it into the N-device
 * crossover. */
val_status_t val_gpu_host_copy_probe(uint32_t copies, uint64_t bytes, uint32_t reps, int pinned_dst, double *gbs);
/* Uniform batches whose frame groups do not fill the last round of the
 * persistent grid (e.g. 131,113 x 64 KiB frames: 8 rounds and 41 frames)
 * hash the frames past the last full round in pieces inside the same
 * launch (1-4 KiB pieces; 8 or 16 lanes per frame, frames of 8 KiB and more), instead of a
 * second launch. 1 / 0 switch it on / off, -1 = VAL_GPU_TAIL_PIECES (unset:
 * on). Speed only; results never change. _launches counts the launches that
 * used it. */
void val_gpu_set_tail_pieces(int enable);
uint64_t val_gpu_tail_piece_launches(void);
/* Multi-pass launches of long frames (8 lanes per frame, frames of 8 KiB and
 * more, no payload states) read every round after a frame's first through
 * non-temporal LDS-DMA beside a compact table image, instead of ordinary
 * loads. 1 / 0 force the path on (for every launch its kernels can hash,
 * one-pass launches included) / off, -1 = VAL_GPU_STREAM_LOADS (unset: the
 * rule). Speed only; results never change. _launches counts the launches that
 * used it. */
void val_gpu_set_stream_loads(int enable);
uint64_t val_gpu_stream_load_launches(void);
/* Wire bytes per H2D chunk of the *_frames_host calls; 0 = default (64 MiB).
 * Device memory use is two chunks. Speed and memory only; results never change. */
val_status_t val_gpu_set_host_chunk_bytes(size_t bytes);

/* ---- build and introspection --------------------------------------------
 * Diagnostic compile-time switches this library was built with, as a
 * space-separated list ("" for a product build). Switches that change
 * results can only be enabled in a VCRC_DIAG_BUILD, and such a build reports
 * "VCRC_DIAG_BUILD" here; tests/test_build.py asserts the in-tree library
 * reports nothing. */
const char *val_gpu_build_flags(void);
/* ---- introspection for benchmarks ---------------------------------------
 * Lanes per frame the library would pick for a given typical length. */
uint32_t val_gpu_lanes_per_frame(uint32_t typical_len);
/* The launches the library would make for one batch of n frames on a device
 * of `cus` compute units, with the process's current knobs (forced lanes and
 * prefetch, tail pieces, ragged minimum, the VAL_GPU_* environment). Needs no
 * device and initialises none. typical_len: flen for strided batches, the
 * length hint for descriptor batches (0 = unknown or mixed); flen / last_len:
 * strided batches only. Writes up to two launches (the second is the re-cut
 * tail of the first) and returns their number. */
enum {
    VAL_GPU_KERNEL_RAGGED = 0,    /* binned by length, then one grouped launch */
    VAL_GPU_KERNEL_SPLIT = 1,     /* one workgroup per frame */
    VAL_GPU_KERNEL_FRAMES = 2,    /* lanes per frame, persistent waves */
    VAL_GPU_KERNEL_FRAMES_C0 = 3, /* the same with one-pass loads of round 0 */
    /* the window calls' kernels (val_gpu_plan_window) */
    VAL_GPU_KERNEL_PACK = 4,
    VAL_GPU_KERNEL_UNPACK_PARSE = 5,
    VAL_GPU_KERNEL_UNPACK_ORDER = 6,
    VAL_GPU_KERNEL_UNPACK_ORDER_FILES = 7,
    VAL_GPU_KERNEL_UNPACK = 8,
    VAL_GPU_KERNEL_SCAN_STREAMS = 9,
    VAL_GPU_KERNEL_SCAN_FIRST = 10,
    VAL_GPU_KERNEL_SCAN_COMPACT = 11,
    VAL_GPU_KERNEL_FILL_COUNT = 12,
    VAL_GPU_KERNEL_FILL_DESC = 13,
    /* the file-window calls' kernels (val_gpu_plan_file_windows) */
    VAL_GPU_KERNEL_WINDOWS_COUNT = 14,
    VAL_GPU_KERNEL_WINDOWS_HASH = 15,
    /* the ACK calls' kernels (val_gpu_plan_ack_calls) */
    VAL_GPU_KERNEL_ACK_RESPOND_FILES = 16,
    VAL_GPU_KERNEL_ACK_EMIT = 17,
    VAL_GPU_KERNEL_ACK_APPLY_FILES = 18
};
typedef struct val_gpu_launch {
    uint32_t kernel;        /* VAL_GPU_KERNEL_* */
    uint32_t lanes;         /* lanes per frame (frames kernels) */
    int32_t depth;          /* round loop instantiated: 0, 1, 2, 4, -2 or -3 */
    uint32_t grid;          /* workgroups */
    uint32_t first, count;  /* frames [first, first + count) */
    uint32_t k0;            /* split kernel: log2 of the chunk bytes */
    uint32_t qparts;        /* dynamic-tail queue partitions; 0 = static deal */
    uint32_t static_rounds; /* with a queue: group rounds dealt before it */
    uint32_t tail_n;        /* frames after `count` hashed in pieces inside this launch */
    uint32_t tail_k0;       /* log2 of the piece bytes */
    uint32_t tail_units;    /* pieces per tail frame */
} val_gpu_launch_t;
uint32_t val_gpu_plan_frames(uint32_t cus, uint32_t n, int descriptors, uint32_t typical_len, uint32_t flen,
                             uint32_t last_len, int want_payload, val_gpu_launch_t out_plan[2]);
/* The load path of each of those launches, same arguments: out_stream[i] = 1
 * where launch i reads through LDS-DMA (val_gpu_set_stream_loads), else 0.
 * Returns the number of launches. */
uint32_t val_gpu_plan_stream_loads(uint32_t cus, uint32_t n, int descriptors, uint32_t typical_len, uint32_t flen,
                                   uint32_t last_len, int want_payload, int out_stream[2]);
/* The launches one window call would make after its verify launches, if any
 * (those are val_gpu_plan_frames), in order, with the process's current knobs
 * (forced lanes, scan front); of a launch, kernel, lanes, grid and count (the
 * entries the grid covers) are set, and for k_scan_streams lanes means lanes
 * per stream. */
enum { VAL_GPU_WINDOW_PACK = 0, VAL_GPU_WINDOW_UNPACK = 1, VAL_GPU_WINDOW_UNPACK_FILES = 2,
       VAL_GPU_WINDOW_SCAN = 3, VAL_GPU_WINDOW_FILL = 4 };
/* n: frames (pack, unpack) or streams / transfers (scan, fill); groups: files of
 * UNPACK_FILES, else 0; max_frames: scan and fill, else 0; len_hint as the call takes
 * it (strided unpack: flen; fill: the mtu). Needs no device. Returns the number of
 * launches written: 0 for an unknown call or one that launches nothing. */
uint32_t val_gpu_plan_window(uint32_t call, uint32_t cus, uint32_t n, uint32_t groups,
                             uint32_t max_frames, uint32_t len_hint, val_gpu_launch_t out[4]);
/* The launches val_crc32_file_windows_dev and the three resume calls would
 * make for n_files files and windows of at most max_len bytes on a device of
 * `cus` compute units, in order: the count launch, the prefix sum
 * (VAL_GPU_KERNEL_SCAN_FIRST) and the hash launch; kernel, grid, count (the
 * files, or the most chunks the call can have) and, on the count and hash
 * launches, k0 (log2 of the call's chunk bytes) are set. max_len == 0 is the
 * count launch alone. Needs no device. Returns the number of launches written:
 * 0 for n_files == 0 and for a call that is refused (max_len above 2^32, or
 * the chunk product overflowing 32 bits). */
uint32_t val_gpu_plan_file_windows(uint32_t cus, uint32_t n_files, uint64_t max_len, val_gpu_launch_t out[3]);
/* The launches val_frame_respond_files_dev (VAL_GPU_ACK_RESPOND: the header
 * facts, the rule, the response frames) and val_frame_apply_acks_files_dev
 * (VAL_GPU_ACK_APPLY: one launch after its verify launches, which are
 * val_gpu_plan_frames) would make for n frames of n_files files on a device of
 * `cus` compute units, in order; kernel, grid and count (the frames or files
 * the grid covers) are set, and on the respond call's rule launch lanes, the
 * threads of a workgroup (256 when the files own 256 frames or fewer on
 * average, else 1,024; speed only). Needs no device. Returns the number of launches
 * written: 0 for an unknown call, n == 0 or n_files == 0. */
enum { VAL_GPU_ACK_RESPOND = 0, VAL_GPU_ACK_APPLY = 1 };
uint32_t val_gpu_plan_ack_calls(uint32_t call, uint32_t cus, uint32_t n, uint32_t n_files, val_gpu_launch_t out[3]);
/* Chunk bytes 2^k0 of the file-window calls: 12..16 force them, 0 restores
 * the automatic choice (the smallest of 4 .. 64 KiB at which n_files windows
 * of max_len bytes are at most one chunk per wave of the device); any other
 * value returns VAL_ERR_INVALID_ARG. A forced value is raised as far as a
 * call's max_len needs (a window has at most 2^16 chunks) and its chunk
 * product allows. Speed only; results never change (tests force 12, so that
 * the multi-chunk paths run on kilobytes). */
val_status_t val_gpu_set_file_window_chunk(uint32_t k0);
/* Force the lanes-per-frame geometry (1,2,4,...,64) for later calls of this
 * process; 0 restores the automatic choice. Returns VAL_ERR_INVALID_ARG for
 * other values. Results never depend on it; only speed does. */
val_status_t val_gpu_set_lanes_per_frame(uint32_t lanes);
/* Rounds of each lane's input kept in flight ahead of the one being hashed:
 * 0, 1, 2 or 4 (copy and refill), or -2 / -3 (a ring of 2 or 3 rounds hashed
 * in their registers and refilled in place; 2 and 4 lanes per frame only,
 * others run 1); -1 = automatic: the 3-ring at 2 lanes, the 2-ring at 4 lanes
 * for frames under 1,600 B,
 * 1 otherwise. Speed only; results never change. */
val_status_t val_gpu_set_prefetch(int depth);
/* Lanes that walk one stream in val_frame_scan_streams_dev: 64 (a wave per
 * stream) or 1024 (a workgroup per stream); 0 = automatic: 1024 while the call
 * has no more streams than the device has CUs, 64 beyond. Any other value
 * returns VAL_ERR_INVALID_ARG. Speed only; results never change. */
val_status_t val_gpu_set_scan_front(uint32_t lanes);
/* Mixed-length descriptor batches (len_hint 0) of at least this many frames
 * are binned by length on the device; smaller ones run uniform. -1 restores
 * VAL_GPU_RAGGED_MIN_FRAMES from the environment (read once), else 4096.
 * Speed only; results never change (tests pin the binned path with 1). */
void val_gpu_set_ragged_min_frames(int64_t frames);
uint32_t val_gpu_ragged_min_frames(void);
/* Streams of `device` that hold library scratch (region accumulator, ragged
 * binning, dynamic-tail queue); *evictions (nullable) = entries dropped so
 * far, least recently used first, once more than 64 streams held scratch.
 * Introspection for tests. */
uint32_t val_gpu_scratch_entries(int device, uint64_t *evictions);

#ifdef __cplusplus
}
#endif
#endif /* VAL_CRC32_GPU_H */
