/*
 * val_wire.c -- host-side frame codec and batch framing for the MI355X CRC
 * path (C99). The GPU kernels hash what these helpers lay out.
 *
 * Header and control codecs: same byte layouts as the reference
 * (src/val_wire.c:27-192).
 * Batch framing: the per-frame body of val__internal_send_packet_core
 * (src/val_core.c:733-832) applied to a whole window of DATA frames at once,
 * so one kernel launch can fill every trailer.
 * Stream scan: the header/length checks of val_internal_recv_packet
 * (src/val_core.c:893-921) applied to a buffered byte stream (8(f) f2).
 */
#include <string.h>

#include "val_byte_order.h"
#include "val_wire.h"

#include "resume_rules.h"

void val_serialize_frame_header(uint8_t type, uint8_t flags, uint16_t content_len, uint32_t type_data, uint8_t *wiredata)
{
    if (!wiredata)
        return;
    wiredata[0] = type;
    wiredata[1] = flags;
    val_put_le16(wiredata + 2, content_len);
    val_put_le32(wiredata + 4, type_data);
}

void val_deserialize_frame_header(const uint8_t *wiredata, uint8_t *type, uint8_t *flags, uint16_t *content_len,
                                  uint32_t *type_data)
{
    if (!wiredata)
        return;
    if (type)
        *type = wiredata[0];
    if (flags)
        *flags = wiredata[1];
    if (content_len)
        *content_len = val_get_le16(wiredata + 2);
    if (type_data)
        *type_data = val_get_le32(wiredata + 4);
}

/* ---- control payload codecs: field by field, little-endian (the byte
 * layouts of reference src/val_wire.c:47-192; pinned by
 * tests/test_header_surface.py against the reference's own codec). */
void val_serialize_handshake(const val_handshake_t *hs, uint8_t *wire_data)
{
    if (!hs || !wire_data)
        return;
    uint8_t *w = wire_data;
    val_put_le32(w + 0, hs->magic);
    w[4] = hs->version_major;
    w[5] = hs->version_minor;
    val_put_le16(w + 6, hs->reserved);
    val_put_le32(w + 8, hs->packet_size);
    val_put_le32(w + 12, hs->features);
    val_put_le32(w + 16, hs->required);
    val_put_le32(w + 20, hs->requested);
    val_put_le16(w + 24, hs->tx_max_window_packets);
    val_put_le16(w + 26, hs->rx_max_window_packets);
    w[28] = hs->ack_stride_packets;
    memcpy(w + 29, hs->reserved_capabilities, 3);
    val_put_le16(w + 32, hs->supported_features16);
    val_put_le16(w + 34, hs->required_features16);
    val_put_le16(w + 36, hs->requested_features16);
    w[38] = w[39] = 0; /* padding on the wire */
    val_put_le32(w + 40, hs->reserved2);
}

void val_deserialize_handshake(const uint8_t *wire_data, val_handshake_t *hs)
{
    if (!wire_data || !hs)
        return;
    const uint8_t *w = wire_data;
    hs->magic = val_get_le32(w + 0);
    hs->version_major = w[4];
    hs->version_minor = w[5];
    hs->reserved = val_get_le16(w + 6);
    hs->packet_size = val_get_le32(w + 8);
    hs->features = val_get_le32(w + 12);
    hs->required = val_get_le32(w + 16);
    hs->requested = val_get_le32(w + 20);
    hs->tx_max_window_packets = val_get_le16(w + 24);
    hs->rx_max_window_packets = val_get_le16(w + 26);
    hs->ack_stride_packets = w[28];
    memcpy(hs->reserved_capabilities, w + 29, 3);
    hs->supported_features16 = val_get_le16(w + 32);
    hs->required_features16 = val_get_le16(w + 34);
    hs->requested_features16 = val_get_le16(w + 36);
    hs->reserved2 = val_get_le32(w + 40);
}

#define VAL_META_NAME_BYTES (VAL_MAX_FILENAME + 1u)
#define VAL_META_PATH_BYTES (VAL_MAX_PATH + 1u)

void val_serialize_meta(const val_meta_payload_t *meta, uint8_t *wire_data)
{
    if (!meta || !wire_data)
        return;
    memcpy(wire_data, meta->filename, VAL_META_NAME_BYTES);
    memcpy(wire_data + VAL_META_NAME_BYTES, meta->sender_path, VAL_META_PATH_BYTES);
    val_put_le64(wire_data + VAL_META_NAME_BYTES + VAL_META_PATH_BYTES, meta->file_size);
}

void val_deserialize_meta(const uint8_t *wire_data, val_meta_payload_t *meta)
{
    if (!wire_data || !meta)
        return;
    memcpy(meta->filename, wire_data, VAL_META_NAME_BYTES);
    memcpy(meta->sender_path, wire_data + VAL_META_NAME_BYTES, VAL_META_PATH_BYTES);
    meta->file_size = val_get_le64(wire_data + VAL_META_NAME_BYTES + VAL_META_PATH_BYTES);
}

void val_serialize_resume_resp(const val_resume_resp_t *resp, uint8_t *wire_data)
{
    if (!resp || !wire_data)
        return;
    val_put_le32(wire_data, (uint32_t)resp->action);
    val_put_le64(wire_data + 4, resp->resume_offset);
    val_put_le32(wire_data + 12, resp->verify_crc);
    val_put_le64(wire_data + 16, resp->verify_length);
}

void val_deserialize_resume_resp(const uint8_t *wire_data, val_resume_resp_t *resp)
{
    if (!wire_data || !resp)
        return;
    resp->action = (val_resume_action_t)val_get_le32(wire_data);
    resp->resume_offset = val_get_le64(wire_data + 4);
    resp->verify_crc = val_get_le32(wire_data + 12);
    resp->verify_length = val_get_le64(wire_data + 16);
}

void val_serialize_verify_request(uint64_t offset, uint32_t crc, uint32_t length, uint8_t *wire_data)
{
    if (!wire_data)
        return;
    val_put_le64(wire_data, offset);
    val_put_le32(wire_data + 8, crc);
    val_put_le32(wire_data + 12, length);
}

void val_deserialize_verify_request(const uint8_t *wire_data, uint64_t *offset, uint32_t *crc, uint32_t *length)
{
    if (!wire_data)
        return;
    if (offset)
        *offset = val_get_le64(wire_data);
    if (crc)
        *crc = val_get_le32(wire_data + 8);
    if (length)
        *length = val_get_le32(wire_data + 12);
}

void val_serialize_verify_response(val_status_t result, uint32_t receiver_crc, uint8_t *wire_data)
{
    if (!wire_data)
        return;
    val_put_le32(wire_data, (uint32_t)result);
    val_put_le32(wire_data + 4, receiver_crc);
}

void val_deserialize_verify_response(const uint8_t *wire_data, val_status_t *result, uint32_t *receiver_crc)
{
    if (!wire_data)
        return;
    if (result)
        *result = (val_status_t)(int32_t)val_get_le32(wire_data);
    if (receiver_crc)
        *receiver_crc = val_get_le32(wire_data + 4);
}

void val_serialize_error_payload(const val_error_payload_t *payload, uint8_t *wire_data)
{
    if (!payload || !wire_data)
        return;
    val_put_le32(wire_data, (uint32_t)payload->code);
    val_put_le32(wire_data + 4, payload->detail);
}

void val_deserialize_error_payload(const uint8_t *wire_data, val_error_payload_t *payload)
{
    if (!wire_data || !payload)
        return;
    payload->code = (int32_t)val_get_le32(wire_data);
    payload->detail = val_get_le32(wire_data + 4);
}

/* ---- batch framing ------------------------------------------------------ */
val_status_t val_frame_data_layout(const uint32_t *pay_len, const uint8_t *include_offset, uint32_t n,
                                   uint64_t *frame_off, uint32_t *crc_len, uint64_t *total)
{
    if (total)
        *total = 0;
    if (n && !pay_len)
        return VAL_ERR_INVALID_ARG;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; i++) {
        const int explicit_off = include_offset ? (include_offset[i] != 0) : 1;
        const uint64_t content = (uint64_t)pay_len[i] + (explicit_off ? 8u : 0u);
        if (content > VAL_WIRE_MAX_CONTENT)
            return VAL_ERR_INVALID_ARG; /* the reference would wrap content_len here */
        if (frame_off)
            frame_off[i] = pos;
        if (crc_len)
            crc_len[i] = (uint32_t)(VAL_WIRE_HEADER_SIZE + content);
        pos += VAL_WIRE_HEADER_SIZE + content + VAL_WIRE_TRAILER_SIZE;
    }
    if (total)
        *total = pos;
    return VAL_OK;
}

val_status_t val_frame_data_batch(const uint8_t *payload, const uint64_t *pay_off, const uint32_t *pay_len,
                                  const uint64_t *file_off, const uint8_t *include_offset, uint32_t n, uint8_t *out,
                                  size_t out_cap, uint64_t *frame_off, uint32_t *crc_len, size_t *out_used)
{
    if (out_used)
        *out_used = 0;
    if (n && (!pay_len || !file_off || !out || !frame_off || !crc_len))
        return VAL_ERR_INVALID_ARG;
    /* Every frame's position comes from val_frame_data_layout, one frame at a
     * time: the frames before a refused one are laid out as they always were. */
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *inc = include_offset ? include_offset + i : NULL;
        uint64_t at = 0, wire = 0;
        uint32_t clen = 0;
        if (val_frame_data_layout(pay_len + i, inc, 1, &at, &clen, &wire) != VAL_OK)
            return VAL_ERR_INVALID_ARG;
        if (pay_len[i] && (!payload || !pay_off))
            return VAL_ERR_INVALID_ARG;
        if (wire > (uint64_t)out_cap - pos)
            return VAL_ERR_INVALID_ARG;
        const uint32_t content = clen - VAL_WIRE_HEADER_SIZE;
        const int explicit_off = content != pay_len[i];
        uint8_t *f = out + pos + at;
        val_serialize_frame_header((uint8_t)VAL_PKT_DATA, explicit_off ? (uint8_t)VAL_DATA_OFFSET_PRESENT : 0u,
                                   (uint16_t)content, 0u, f);
        uint8_t *c = f + VAL_WIRE_HEADER_SIZE;
        if (explicit_off) {
            val_put_le64(c, file_off[i]);
            c += 8;
        }
        if (pay_len[i])
            memcpy(c, payload + pay_off[i], pay_len[i]);
        memset(f + clen, 0, VAL_WIRE_TRAILER_SIZE);
        frame_off[i] = pos + at;
        crc_len[i] = clen;
        pos += wire;
    }
    if (out_used)
        *out_used = (size_t)pos;
    return VAL_OK;
}

void val_frame_put_trailers(uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, const uint32_t *crc,
                            uint32_t n)
{
    for (uint32_t i = 0; i < n; i++)
        val_put_le32(stream + frame_off[i] + crc_len[i], crc[i]);
}

val_status_t val_frame_scan(const uint8_t *stream, size_t len, size_t mtu, uint32_t max_frames, uint64_t *frame_off,
                            uint32_t *crc_len, uint32_t *n_frames, size_t *consumed)
{
    if (n_frames)
        *n_frames = 0;
    if (consumed)
        *consumed = 0;
    if ((!stream && len) || !frame_off || !crc_len)
        return VAL_ERR_INVALID_ARG;
    if (mtu < VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE)
        return VAL_ERR_INVALID_ARG;
    const size_t max_content = mtu - VAL_WIRE_HEADER_SIZE - VAL_WIRE_TRAILER_SIZE;
    size_t pos = 0;
    uint32_t k = 0;
    val_status_t st = VAL_OK;
    while (k < max_frames && len - pos >= VAL_WIRE_HEADER_SIZE) {
        uint16_t content = 0;
        val_deserialize_frame_header(stream + pos, NULL, NULL, &content, NULL);
        if ((size_t)content > max_content) {
            st = VAL_ERR_PROTOCOL;
            break;
        }
        const size_t wire = VAL_WIRE_HEADER_SIZE + (size_t)content + VAL_WIRE_TRAILER_SIZE;
        if (len - pos < wire)
            break; /* incomplete frame: wait for more bytes */
        frame_off[k] = pos;
        crc_len[k] = (uint32_t)(VAL_WIRE_HEADER_SIZE + content);
        k++;
        pos += wire;
    }
    if (n_frames)
        *n_frames = k;
    if (consumed)
        *consumed = pos;
    return st;
}

void val_frame_payload_lens(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                            uint32_t *pay_len)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t L = crc_len[i];
        uint32_t pre = VAL_WIRE_HEADER_SIZE;
        if (L >= VAL_WIRE_HEADER_SIZE && (stream[frame_off[i] + 1] & VAL_DATA_OFFSET_PRESENT))
            pre += 8u;
        pay_len[i] = L >= pre ? L - pre : 0u;
    }
}

void val_frame_data_offsets(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                            uint64_t *file_off)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *f = stream + frame_off[i];
        const uint32_t L = crc_len[i];
        if (L < VAL_WIRE_HEADER_SIZE || f[0] != (uint8_t)VAL_PKT_DATA)
            file_off[i] = VAL_FRAME_OFFSET_NOT_DATA;
        else if (!(f[1] & VAL_DATA_OFFSET_PRESENT))
            file_off[i] = VAL_FRAME_OFFSET_IMPLIED;
        else if (L < VAL_WIRE_HEADER_SIZE + 8u)
            file_off[i] = VAL_FRAME_OFFSET_NOT_DATA; /* no room for the offset: never folded */
        else
            file_off[i] = val_get_le64(f + VAL_WIRE_HEADER_SIZE);
    }
}

void val_frame_accept(const uint64_t *file_off, const uint32_t *pay_len, const uint8_t *ok, uint32_t n,
                      uint64_t file_cap, uint64_t *written, uint64_t *dst_off, uint32_t *n_accepted,
                      uint32_t *n_overflow)
{
    uint32_t accepted = 0, overflow = 0;
    if (n_accepted)
        *n_accepted = 0;
    if (n_overflow)
        *n_overflow = 0;
    if (!written || (n && (!file_off || !pay_len)))
        return;
    uint64_t w = *written;
    for (uint32_t i = 0; i < n; i++) {
        if (dst_off)
            dst_off[i] = VAL_FRAME_NOT_ACCEPTED;
        if ((ok && !ok[i]) || file_off[i] == VAL_FRAME_OFFSET_NOT_DATA)
            continue;
        const uint64_t eff = file_off[i] == VAL_FRAME_OFFSET_IMPLIED ? w : file_off[i];
        if (eff != w)
            continue; /* duplicate or gap */
        if (w > file_cap || (uint64_t)pay_len[i] > file_cap - w) { /* w + pay_len > file_cap, without the wrap */
            overflow++;
            continue;
        }
        if (dst_off)
            dst_off[i] = w;
        w += pay_len[i];
        accepted++;
    }
    *written = w;
    if (n_accepted)
        *n_accepted = accepted;
    if (n_overflow)
        *n_overflow = overflow;
}

val_status_t val_frame_fill_window(uint64_t next, uint64_t last_acked, uint64_t file_size, uint64_t mtu,
                                   uint32_t budget, uint64_t out_cap, uint64_t *file_off, uint32_t *pay_len,
                                   uint8_t *include_offset, uint64_t *frame_off, uint32_t *crc_len,
                                   uint32_t *n_frames, uint64_t *out_used, uint64_t *next_out)
{
    uint32_t k = 0;
    uint64_t used = 0;
    val_status_t st = VAL_OK;
    if (mtu < VAL_FILL_MTU_MIN || mtu > VAL_FILL_MTU_MAX) {
        st = VAL_ERR_INVALID_ARG;
        budget = 0;
    }
    const uint64_t room = mtu - (VAL_WIRE_HEADER_SIZE + VAL_WIRE_TRAILER_SIZE); /* M; unused when refused */
    while (k < budget && next < file_size) {
        const int explicit_off = next == last_acked;
        const uint64_t left = file_size - next;
        const uint64_t most = explicit_off ? room - 8u : room;
        const uint64_t pay = left < most ? left : most;
        const uint64_t content = pay + (explicit_off ? 8u : 0u);
        const uint64_t need = VAL_WIRE_HEADER_SIZE + content + VAL_WIRE_TRAILER_SIZE;
        if (need > out_cap - used) /* used <= out_cap */
            break;
        if (file_off)
            file_off[k] = next;
        if (pay_len)
            pay_len[k] = (uint32_t)pay;
        if (include_offset)
            include_offset[k] = (uint8_t)explicit_off;
        if (frame_off)
            frame_off[k] = used;
        if (crc_len)
            crc_len[k] = (uint32_t)(VAL_WIRE_HEADER_SIZE + content);
        used += need;
        next += pay; /* <= file_size */
        k++;
    }
    if (n_frames)
        *n_frames = k;
    if (out_used)
        *out_used = used;
    if (next_out)
        *next_out = next;
    return st;
}

/* The resume rules: bodies in resume_rules.h, which the device code shares. */
int val_resume_tail_window(uint64_t existing, uint64_t incoming, uint64_t tail_cap_bytes, uint64_t min_verify_bytes,
                           int mismatch_skip, uint64_t *resume_offset, uint64_t *verify_len)
{
    uint64_t off = 0, len = 0;
    const int action = val_rule_tail_window(existing, incoming, tail_cap_bytes, min_verify_bytes, mismatch_skip, &off, &len);
    if (resume_offset)
        *resume_offset = off;
    if (verify_len)
        *verify_len = len;
    return action;
}

int val_resume_request_window(uint64_t resume_offset, uint64_t verify_len, uint64_t *start, uint32_t *vlen32)
{
    uint64_t s = 0;
    uint32_t v = 0;
    const int send = val_rule_request_window(resume_offset, verify_len, &s, &v);
    if (start)
        *start = s;
    if (vlen32)
        *vlen32 = v;
    return send;
}

val_status_t val_resume_verdict(int window_ok, uint32_t local_crc, uint32_t sender_crc, int mismatch_skip,
                                uint64_t rec_resume_off, uint64_t file_size, uint64_t *resume_off_out)
{
    uint64_t off = 0;
    const val_status_t st = val_rule_verdict(window_ok, local_crc, sender_crc, mismatch_skip, rec_resume_off, file_size, &off);
    if (resume_off_out)
        *resume_off_out = off;
    return st;
}

/* ---- DATA_ACK / DATA_NAK: the receiver's answers and the sender's handling ---- */
void val_frame_ack_offsets(const uint8_t *stream, const uint64_t *frame_off, const uint32_t *crc_len, uint32_t n,
                           uint8_t *kind, uint64_t *ack_off)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *f = stream + frame_off[i];
        const uint32_t L = crc_len[i];
        uint8_t k = 0;
        uint64_t off = 0;
        if (L >= VAL_WIRE_HEADER_SIZE && (f[0] == (uint8_t)VAL_PKT_DATA_ACK || f[0] == (uint8_t)VAL_PKT_DATA_NAK)) {
            k = f[0];
            off = val_get_le32(f + 4);
            if (L >= VAL_WIRE_HEADER_SIZE + 4u)
                off |= (uint64_t)val_get_le32(f + VAL_WIRE_HEADER_SIZE) << 32;
        }
        if (kind)
            kind[i] = k;
        if (ack_off)
            ack_off[i] = off;
    }
}

/* The frames val_frame_accept would accept: whether frame i, judged at w, is one. */
static int respond_accepts(uint64_t file_off, uint32_t pay_len, uint64_t w, uint64_t file_cap)
{
    if (file_off != VAL_FRAME_OFFSET_IMPLIED && file_off != w)
        return 0;
    return !(w > file_cap || (uint64_t)pay_len > file_cap - w);
}

void val_frame_respond_window(const uint64_t *file_off, const uint32_t *pay_len, const uint8_t *ok, uint32_t n,
                              uint64_t file_cap, uint64_t total, uint32_t ack_stride, uint64_t *written,
                              uint32_t *since, uint32_t *resp_frame, uint8_t *resp_kind, uint64_t *resp_off,
                              uint32_t *n_resp)
{
    if (n_resp)
        *n_resp = 0;
    if (!written || (n && (!file_off || !pay_len)) || (ack_stride && !since))
        return;
    uint64_t w = *written;
    /* one ACK per window: the call's last accepted frame is known only after a walk of its own */
    uint32_t last = n;
    if (ack_stride == 0) {
        for (uint32_t i = 0; i < n; i++) {
            if ((ok && !ok[i]) || file_off[i] == VAL_FRAME_OFFSET_NOT_DATA)
                continue;
            if (respond_accepts(file_off[i], pay_len[i], w, file_cap)) {
                w += pay_len[i];
                last = i;
            }
        }
        w = *written;
    }
    uint32_t s = ack_stride ? *since : 0u;
    uint32_t r = 0;
#define VAL_RESPOND_EMIT(k_, off_)           \
    do {                                     \
        if (resp_frame)                      \
            resp_frame[r] = i;               \
        if (resp_kind)                       \
            resp_kind[r] = (uint8_t)(k_);    \
        if (resp_off)                        \
            resp_off[r] = (off_);            \
        r++;                                 \
    } while (0)
    for (uint32_t i = 0; i < n; i++) {
        if ((ok && !ok[i]) || file_off[i] == VAL_FRAME_OFFSET_NOT_DATA)
            continue;
        const uint64_t eff = file_off[i] == VAL_FRAME_OFFSET_IMPLIED ? w : file_off[i];
        if (eff == w) {
            if (!respond_accepts(file_off[i], pay_len[i], w, file_cap))
                continue; /* refused by capacity alone: silent */
            w += pay_len[i];
            if (w >= total) {
                VAL_RESPOND_EMIT(VAL_PKT_DATA_ACK, w);
                s = 0;
            } else if (ack_stride == 0) {
                if (i == last)
                    VAL_RESPOND_EMIT(VAL_PKT_DATA_ACK, w);
            } else {
                if (s != UINT32_MAX)
                    s++;
                if (s >= ack_stride) {
                    VAL_RESPOND_EMIT(VAL_PKT_DATA_ACK, w);
                    s = 0;
                }
            }
        } else if (eff < w) {
            VAL_RESPOND_EMIT(VAL_PKT_DATA_ACK, w); /* duplicate: reaffirm */
        } else {
            VAL_RESPOND_EMIT(VAL_PKT_DATA_NAK, w); /* gap */
            VAL_RESPOND_EMIT(VAL_PKT_DATA_ACK, w);
        }
    }
#undef VAL_RESPOND_EMIT
    *written = w;
    if (ack_stride)
        *since = s;
    if (n_resp)
        *n_resp = r;
}

void val_frame_apply_acks(const uint8_t *kind, const uint64_t *ack_off, const uint8_t *ok, uint32_t n,
                          uint64_t file_size, uint64_t *last_acked, uint64_t *next, uint32_t *n_retrans,
                          uint32_t *n_crc)
{
    uint32_t retrans = 0, crc = 0;
    if (n_retrans)
        *n_retrans = 0;
    if (n_crc)
        *n_crc = 0;
    if (!last_acked || !next || (n && (!kind || !ack_off)))
        return;
    uint64_t la = *last_acked, nx = *next;
    for (uint32_t i = 0; i < n; i++) {
        if (ok && !ok[i]) {
            nx = la;
            retrans++;
            crc++;
            continue;
        }
        if (kind[i] != (uint8_t)VAL_PKT_DATA_ACK && kind[i] != (uint8_t)VAL_PKT_DATA_NAK)
            continue;
        if (la < ack_off[i] && ack_off[i] <= file_size)
            la = ack_off[i];
        if (kind[i] == (uint8_t)VAL_PKT_DATA_NAK) {
            nx = la;
            retrans++;
        }
    }
    if (nx < la)
        nx = la;
    *last_acked = la;
    *next = nx;
    if (n_retrans)
        *n_retrans = retrans;
    if (n_crc)
        *n_crc = crc;
}
