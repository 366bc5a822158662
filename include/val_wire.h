/*
 * val_wire.h -- VAL v0.7 wire surface (frame layout, control payloads and
 * their codecs, as reference include/val_wire.h) plus the host-side batch
 * framing helpers of the MI355X CRC path.
 *
 * Frame (reference include/val_wire.h:14,21,32-38):
 *   [0] type  [1] flags  [2..3] content_len LE16  [4..7] type_data LE32
 *   [8 .. 8+content_len)  content   (DATA + OFFSET_PRESENT: LE64 offset, payload)
 *   [8+content_len .. +4) trailer = LE32 CRC-32 over bytes [0, 8+content_len)
 *
 * "CRC input" of a frame = its first 8 + content_len bytes.
 * header_crc (this build's definition): CRC-32 of the
 * 8 header bytes, i.e. the finished CRC of the first 8 bytes of the CRC input.
 */
#ifndef VAL_WIRE_H
#define VAL_WIRE_H

#include <stddef.h>
#include <stdint.h>

#include "val_protocol.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Wire sizes of the frame parts and control payloads (reference :14-25). */
#define VAL_WIRE_HEADER_SIZE 8u
#define VAL_WIRE_TRAILER_SIZE 4u
#define VAL_WIRE_HANDSHAKE_SIZE 44u
#define VAL_WIRE_META_SIZE ((VAL_MAX_FILENAME + 1u) + (VAL_MAX_PATH + 1u) + 8u)
#define VAL_WIRE_RESUME_RESP_SIZE 24u
#define VAL_WIRE_VERIFY_REQ_SIZE 16u
#define VAL_WIRE_VERIFY_RESP_SIZE 8u
#define VAL_WIRE_ERROR_PAYLOAD_SIZE 8u
#define VAL_WIRE_VERIFY_REQ_PAYLOAD_SIZE 16u  /* offset u64, crc u32, length u32 */
#define VAL_WIRE_VERIFY_RESP_PAYLOAD_SIZE 8u  /* status i32, receiver crc u32 */
#define VAL_FRAME_HEADER_SIZE VAL_WIRE_HEADER_SIZE
#define VAL_FRAME_TRAILER_SIZE VAL_WIRE_TRAILER_SIZE
#define VAL_WIRE_MAX_CONTENT 0xFFFFu /* content_len is a 16-bit field */

/* RESUME / VERIFY option bits (reserved by v0.7) */
#define VAL_RESUMERESP_VERIFY_REQUIRED (1u << 0)
#define VAL_RESUMERESP_HAS_VERIFY_WINDOW (1u << 1)
#define VAL_VERIFY_REQUEST (1u << 0)

/* DATA flags (byte 1): OFFSET_PRESENT = content starts with the LE64 file offset */
#define VAL_DATA_OFFSET_PRESENT (1u << 0)
#define VAL_DATA_FINAL_CHUNK (1u << 1)
/* DATA_ACK flags */
#define VAL_ACK_FEEDBACK_PRESENT (1u << 0)
#define VAL_ACK_DONE_FILE (1u << 1)
#define VAL_ACK_EOT (1u << 2)

/* HELLO payload, host form (wire: 44 bytes, little-endian, by the codec
 * below; reference :53-75). The window fields carry the flow-control
 * capabilities; the negotiated window is the natural batch size of the
 * GPU TX/RX calls. */
typedef struct {
    uint32_t magic;
    uint8_t version_major;
    uint8_t version_minor;
    uint16_t reserved;
    uint32_t packet_size;
    uint32_t features;
    uint32_t required;
    uint32_t requested;
    uint16_t tx_max_window_packets;
    uint16_t rx_max_window_packets;
    uint8_t ack_stride_packets; /* 0 = one ACK per window */
    uint8_t reserved_capabilities[3];
    uint16_t supported_features16;
    uint16_t required_features16;
    uint16_t requested_features16;
    uint32_t reserved2;
} val_handshake_t;

/* ERROR payload (wire: code i32, detail u32). */
typedef struct {
    int32_t code;
    uint32_t detail;
} val_error_payload_t;

/* Control codecs, same signatures and bytes as the reference
 * (include/val_wire.h:86-105, src/val_wire.c); NULL arguments are no-ops. */
void val_serialize_frame_header(uint8_t type, uint8_t flags, uint16_t content_len, uint32_t type_data, uint8_t *wiredata);
void val_deserialize_frame_header(const uint8_t *wiredata, uint8_t *type, uint8_t *flags, uint16_t *content_len,
                                  uint32_t *type_data);
void val_serialize_handshake(const val_handshake_t *hs, uint8_t *wire_data);
void val_deserialize_handshake(const uint8_t *wire_data, val_handshake_t *hs);
void val_serialize_meta(const val_meta_payload_t *meta, uint8_t *wire_data);
void val_deserialize_meta(const uint8_t *wire_data, val_meta_payload_t *meta);
void val_serialize_resume_resp(const val_resume_resp_t *resp, uint8_t *wire_data);
void val_deserialize_resume_resp(const uint8_t *wire_data, val_resume_resp_t *resp);
void val_serialize_verify_request(uint64_t offset, uint32_t crc, uint32_t length, uint8_t *wire_data);
void val_deserialize_verify_request(const uint8_t *wire_data, uint64_t *offset, uint32_t *crc, uint32_t *length);
void val_serialize_verify_response(val_status_t result, uint32_t receiver_crc, uint8_t *wire_data);
void val_deserialize_verify_response(const uint8_t *wire_data, val_status_t *result, uint32_t *receiver_crc);
void val_serialize_error_payload(const val_error_payload_t *payload, uint8_t *wire_data);
void val_deserialize_error_payload(const uint8_t *wire_data, val_error_payload_t *payload);

/*
 * TX batch framing (the window-fill loop of src/val_sender.c:822-841 turned
 * into one staging pass). Lays `n` DATA frames back to back
 * in `out`: frame i carries payload bytes [pay_off[i], pay_off[i]+pay_len[i])
 * of `payload`, file offset file_off[i], and an LE64 offset prefix when
 * include_offset[i] != 0 (NULL = all explicit, as val_internal_send_packet).
 * Trailers are left zero for the GPU kernel to fill. Writes each frame's
 * start into frame_off[i] and its CRC-input length into crc_len[i].
 * Unlike the reference (src/val_core.c:747, which silently truncates), a
 * content_len above 65535 is rejected with VAL_ERR_INVALID_ARG.
 * *out_used receives the bytes written.
 */
val_status_t val_frame_data_batch(const uint8_t *payload, const uint64_t *pay_off, const uint32_t *pay_len,
                                  const uint64_t *file_off, const uint8_t *include_offset, uint32_t n, uint8_t *out,
                                  size_t out_cap, uint64_t *frame_off, uint32_t *crc_len, size_t *out_used);

/*
 * Where val_frame_data_batch would put each frame, without writing one (host
 * only, no GPU): frame_off[i], crc_len[i] (either may be NULL) and *total,
 * the stream's length. The framer's own positions come from this function.
 * Upload frame_off to place val_frame_data_batch_dev's frames back to back
 * (include/val_crc32_gpu.h). A content_len above 65535 returns
 * VAL_ERR_INVALID_ARG, as the framer does.
 */
val_status_t val_frame_data_layout(const uint32_t *pay_len, const uint8_t *include_offset, uint32_t n,
                                   uint64_t *frame_off, uint32_t *crc_len, uint64_t *total);

/* Write LE32 trailers crc[i] after each frame's CRC input. */
void val_frame_put_trailers(uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, const uint32_t *crc,
                            uint32_t n);

/*
 * RX batch scan: walk a byte stream of concatenated frames (what the
 * receiver's transport delivered) and emit descriptors for the batch verify
 * kernel. Stops at the first incomplete frame or after `max_frames`, or when
 * a header announces content beyond `mtu` - 12 (reference check at
 * src/val_core.c:915-921 -> VAL_ERR_PROTOCOL). *n_frames / *consumed report
 * what was parsed.
 */
val_status_t val_frame_scan(const uint8_t *stream, size_t len, size_t mtu, uint32_t max_frames, uint64_t *frame_off,
                            uint32_t *crc_len, uint32_t *n_frames, size_t *consumed);

/*
 * Payload length of each scanned frame: CRC input minus the 8-byte header
 * and, when flags has VAL_DATA_OFFSET_PRESENT, the 8-byte file offset (the
 * bytes the receiver writes and feeds to its rolling CRC, reference
 * src/val_receiver.c:880-891); 0 for a frame shorter than that prefix.
 * Pairs with the payload states of val_crc32_verify_frames_ex_*.
 */
void val_frame_payload_lens(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                            uint32_t *pay_len);

/*
 * File offset of each scanned frame as the receiver reads it (reference
 * src/val_core.c:981-993): the LE64 after the header for a DATA frame with
 * VAL_DATA_OFFSET_PRESENT, VAL_FRAME_OFFSET_IMPLIED for a DATA frame without
 * it (the receiver's current position), VAL_FRAME_OFFSET_NOT_DATA for other
 * frames (and a DATA frame too short to hold its offset). Pairs with
 * val_crc32_fold_payload_states_at.
 */
#define VAL_FRAME_OFFSET_IMPLIED UINT64_MAX
#define VAL_FRAME_OFFSET_NOT_DATA (UINT64_MAX - 1u)
void val_frame_data_offsets(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                            uint64_t *file_off);

/*
 * The receiver's ordering rule over a scanned batch (reference
 * src/val_receiver.c:871-895), host only: which frames are delivered into the
 * file and where. file_off[] from val_frame_data_offsets, pay_len[] from
 * val_frame_payload_lens, ok[] the trailer verdicts (NULL = all good). With
 * W = *written, frame after frame: a frame is accepted iff ok[i] != 0, it is a
 * DATA frame (file_off[i] != VAL_FRAME_OFFSET_NOT_DATA), its effective offset
 * (file_off[i], or W for VAL_FRAME_OFFSET_IMPLIED) equals W, and
 * W + pay_len[i] <= file_cap (judged without 64-bit wrap-around). An accepted
 * frame gets dst_off[i] = W and advances W by pay_len[i]; every other frame
 * gets dst_off[i] = VAL_FRAME_NOT_ACCEPTED and leaves W alone (duplicates,
 * gaps, corrupt and control frames; later frames are still judged one by
 * one). A frame refused by the capacity test alone is counted in *n_overflow.
 * *written = W on return; *n_accepted / *n_overflow (nullable) are set, not
 * incremented; dst_off may be NULL. With file_cap = UINT64_MAX the accepted
 * frames are exactly those val_crc32_fold_payload_states_at folds. It states
 * the rule val_frame_unpack_batch_dev (val_crc32_gpu.h) applies on the device.
 */
#define VAL_FRAME_NOT_ACCEPTED UINT64_MAX
void val_frame_accept(const uint64_t *file_off, const uint32_t *pay_len, const uint8_t *ok, uint32_t n,
                      uint64_t file_cap, uint64_t *written, uint64_t *dst_off, uint32_t *n_accepted,
                      uint32_t *n_overflow);

/*
 * The sender's window-fill rule (reference src/val_sender.c:822-841 with
 * send_data_packet, :258-315, and the explicit-offset rule of :833), host
 * only: which DATA frames a sender that stands at file offset `next`, whose
 * last acknowledged offset is `last_acked`, puts into a window of at most
 * `budget` frames and `out_cap` wire bytes of a file of `file_size` bytes.
 * With M = mtu - 12, while fewer than `budget` frames were made and
 * next < file_size: the frame is explicit (it carries its LE64 file offset)
 * iff next == last_acked; last_acked does not move during the call, so with
 * last_acked <= next, as a sender has it, only the call's first frame can be
 * (a last_acked ahead of next makes the frame explicit that starts exactly
 * there, if one does). Its payload is
 * min(file_size - next, explicit ? M - 8 : M) bytes from file offset next, its
 * content the payload plus 8 when explicit, its wire size 12 + content. A
 * frame whose wire size exceeds what is left of out_cap ends the call without
 * being made (judged as val_frame_accept does: need <= cap - used); otherwise
 * it lies back to back behind the previous one and next advances by the
 * payload. Every frame that does not end the file therefore has wire size mtu.
 * Per frame i (arrays of `budget` entries, each nullable): file_off[i],
 * pay_len[i], include_offset[i] (1 / 0), frame_off[i] (relative to the
 * stream start) and crc_len[i] = 8 + content: the inputs and the placement of
 * val_frame_data_batch / val_frame_data_batch_dev. *n_frames, *out_used (the
 * stream's length) and *next_out (each nullable) are set. next >= file_size
 * makes no frame and leaves *next_out = next. All arithmetic is 64-bit and
 * never wraps. Returns VAL_ERR_INVALID_ARG, with the three results set to
 * (0, 0, next), for mtu < 21 (the reference refuses an explicit frame whose
 * payload room is 8 or less) and for mtu > 65547 (content would pass 65535,
 * which the framer rejects). It states the rule val_frame_fill_files_dev
 * (val_crc32_gpu.h) applies on the device.
 */
#define VAL_FILL_MTU_MIN 21u
#define VAL_FILL_MTU_MAX (VAL_WIRE_MAX_CONTENT + VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE)
val_status_t val_frame_fill_window(uint64_t next, uint64_t last_acked, uint64_t file_size, uint64_t mtu,
                                   uint32_t budget, uint64_t out_cap, uint64_t *file_off, uint32_t *pay_len,
                                   uint8_t *include_offset, uint64_t *frame_off, uint32_t *crc_len,
                                   uint32_t *n_frames, uint64_t *out_used, uint64_t *next_out);

/*
 * The three rules of a VAL_RESUME_TAIL handshake, host only: which window of a
 * partial file is hashed, by whom, and what follows from the two CRCs. Each is
 * stated once; the device calls of val_crc32_gpu.h (val_resume_tail_files_dev,
 * val_resume_request_files_dev, val_resume_check_files_dev) apply the same
 * code per file. All arithmetic is 64-bit and never wraps. The NEVER and
 * SKIP_EXISTING modes hash nothing and are not stated here.
 *
 * val_resume_tail_window: the receiver's proposal, the TAIL branch of
 * determine_resume_action (reference src/val_receiver.c:119-181), for a local
 * file of `existing` bytes and an incoming file of `incoming` bytes. Returns
 * the val_resume_action_t value. existing == 0 gives VAL_RESUME_START_ZERO;
 * existing > incoming gives VAL_RESUME_SKIP_FILE when mismatch_skip is set,
 * else VAL_RESUME_START_ZERO. Otherwise, with
 * cap = clamp(tail_cap_bytes ? tail_cap_bytes : 8 MiB, 1, 256 MiB),
 * verify_len = min(existing, cap), and if min_verify_bytes > 0 and
 * verify_len < min_verify_bytes then verify_len = min(existing,
 * min_verify_bytes); the action is VAL_RESUME_VERIFY_FIRST with
 * *resume_offset = existing, and the window to hash is
 * [existing - verify_len, existing). For every other action both outputs are
 * 0. (The reference's remaining START_ZERO exits, a missing receive buffer
 * and a failed read, are the host's own and not part of the rule.) The
 * outputs are nullable.
 */
#define VAL_RESUME_TAIL_CAP_DEFAULT ((uint64_t)8u << 20)
#define VAL_RESUME_TAIL_CAP_MAX ((uint64_t)256u << 20)
int val_resume_tail_window(uint64_t existing, uint64_t incoming, uint64_t tail_cap_bytes, uint64_t min_verify_bytes,
                           int mismatch_skip, uint64_t *resume_offset, uint64_t *verify_len);
/*
 * val_resume_request_window: the sender's clamp of a VERIFY_FIRST answer
 * (reference src/val_sender.c:208-215): *vlen32 =
 * (uint32_t)min(verify_len, resume_offset), *start = resume_offset - *vlen32.
 * The truncation to 32 bits is the reference's (the VERIFY request carries a
 * 32-bit length) and is kept: a verify_len of 2^32 asks for nothing. Returns 0
 * when *vlen32 == 0: no VERIFY is sent and the transfer starts at
 * resume_offset; else 1, and the window to hash in the sender's file is
 * [*start, *start + *vlen32). The outputs are nullable.
 */
int val_resume_request_window(uint64_t resume_offset, uint64_t verify_len, uint64_t *start, uint32_t *vlen32);
/*
 * val_resume_verdict: the result the receiver puts into its VERIFY response
 * and the offset it resumes at (reference src/val_receiver.c:689-721). VAL_OK
 * iff window_ok && local_crc == sender_crc; otherwise VAL_SKIPPED when
 * mismatch_skip is set, else VAL_ERR_RESUME_VERIFY. *resume_off_out (nullable)
 * is rec_resume_off for VAL_OK, file_size (the incoming file's: the file is
 * skipped) for VAL_SKIPPED and 0 for VAL_ERR_RESUME_VERIFY. window_ok == 0 is
 * the reference's short read: a requested window that does not lie inside the
 * local file makes val_internal_crc32_region fail, and the verdict is a
 * mismatch. This is the rule of :662-722; the reference's earlier site
 * (:429-456) answers the same request without the skip branch and is not
 * stated.
 */
val_status_t val_resume_verdict(int window_ok, uint32_t local_crc, uint32_t sender_crc, int mismatch_skip,
                                uint64_t rec_resume_off, uint64_t file_size, uint64_t *resume_off_out);

/*
 * DATA_ACK / DATA_NAK: the receiver's answers to DATA frames and the sender's
 * handling of them (reference src/val_receiver.c:871-1000, src/val_core.c:
 * 775-811,828-834,995-1009, src/val_sender.c:404-555), host only. The device
 * calls val_frame_respond_files_dev and val_frame_apply_acks_files_dev
 * (val_crc32_gpu.h) apply the same rules per file.
 *
 * val_frame_put_response: one response frame with its trailer (the library's
 * CPU engine hashes it) into out[]; returns its wire size, 0 for another kind
 * or a NULL out.
 *   VAL_PKT_DATA_ACK (6): flags 0, type_data = low 32 bits of `offset`; no
 *     content (12 wire bytes) when offset < 2^32, else the LE32 high half
 *     (16 wire bytes). `reason` is unused.
 *   VAL_PKT_DATA_NAK (13): flags 0, content_len 12, type_data = low 32 bits;
 *     content LE32 high, LE32 reason, LE32 0 (24 wire bytes).
 * out needs VAL_WIRE_RESPONSE_MAX bytes.
 */
#define VAL_WIRE_RESPONSE_MAX 24u
#define VAL_NAK_REASON_GAP 1u
uint32_t val_frame_put_response(uint8_t kind, uint64_t offset, uint32_t reason, uint8_t *out);

/*
 * The inverse over scanned frames (val_frame_scan's frame_off / crc_len):
 * kind[i] = 6 or 13 when byte 0 says so and crc_len[i] >= 8, else 0;
 * ack_off[i] = type_data | (crc_len[i] >= 12 ? LE32 at +8 : 0) << 32 for
 * those, 0 for kind 0. Either output may be NULL.
 */
void val_frame_ack_offsets(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                           uint8_t *kind, uint64_t *ack_off);

/*
 * The receiver's answer to one file's window: val_frame_accept's inputs
 * (file_off[], pay_len[], ok[] (NULL = all good), n, file_cap, *written), plus
 * `total`, the incoming file's size from SEND_META, ack_stride (the
 * handshake's ack_stride_packets) and *since, the frames accepted since the
 * last stride ACK (in/out). The responses come in frame order:
 * resp_frame[r] is the index of the frame that caused response r,
 * resp_kind[r] 6 or 13, resp_off[r] its offset (room for 2n entries each, each
 * nullable), *n_resp their number (nullable, set).
 * With W = *written, frame after frame; frames with ok[i] == 0 and non-DATA
 * frames are skipped. eff = W for an implied offset, else file_off[i].
 *   eff == W: a frame that val_frame_accept's capacity test refuses gets no
 *     response. Otherwise W += pay_len[i]; if W >= total: ACK(W), since = 0;
 *     else since++ (saturating), and when ack_stride >= 1 and
 *     since >= ack_stride: ACK(W), since = 0.
 *   eff <  W: ACK(W): a duplicate is reaffirmed; since is left alone.
 *   eff >  W: NAK(W), then ACK(W).
 * ack_stride == 0 is the handshake's "one ACK per window": since is neither
 * read nor written (it may be NULL); an accepted frame emits ACK(W) only when
 * W >= total, and the last accepted frame of the call also emits ACK(W) if it
 * emitted nothing.
 * The accepted frames and the final *written are val_frame_accept's for the
 * same inputs. All arithmetic is 64-bit and never wraps.
 * Two differences from the reference: a frame refused by capacity alone is
 * silent here, where the reference aborts the transfer on a failed fwrite; and
 * stride values other than 1 follow the reference's formula
 * (src/val_receiver.c:975-1000), which the reference itself only ever runs at
 * 1.
 */
void val_frame_respond_window(const uint64_t *file_off, const uint32_t *pay_len, const uint8_t *ok, uint32_t n,
                              uint64_t file_cap, uint64_t total, uint32_t ack_stride, uint64_t *written,
                              uint32_t *since, uint32_t *resp_frame, uint8_t *resp_kind, uint64_t *resp_off,
                              uint32_t *n_resp);

/*
 * The sender's handling of one transfer's response window
 * (wait_for_window_ack, reference src/val_sender.c:404-555): kind[] and
 * ack_off[] from val_frame_ack_offsets, ok[] the trailer verdicts (NULL = all
 * good). With la = *last_acked and nx = *next, frame after frame:
 *   ok[i] == 0: nx = la; a retransmit and a CRC error are counted (the
 *     restart of :542-553).
 *   kind 6:  if la < off && off <= file_size then la = off; any other ACK is
 *     stale and ignored.
 *   kind 13: the same advance, then nx = la; a retransmit is counted
 *     (:432-453, :317-346).
 *   kind 0:  ignored.
 * After the last frame, nx < la becomes nx = la. *n_retrans and *n_crc
 * (nullable) are set, not incremented. All arithmetic is 64-bit and never
 * wraps.
 * One addition to the reference: it does not test an ACK's offset against
 * file_size; this rule does, which keeps last_acked <= file_size, as
 * val_frame_fill_window relies on.
 */
void val_frame_apply_acks(const uint8_t *kind, const uint64_t *ack_off, const uint8_t *ok, uint32_t n,
                          uint64_t file_size, uint64_t *last_acked, uint64_t *next, uint32_t *n_retrans,
                          uint32_t *n_crc);

#ifdef __cplusplus
}
#endif
#endif /* VAL_WIRE_H */
