/*
 * val_ack.c -- the DATA_ACK / DATA_NAK encoder of include/val_wire.h (C99).
 * It lives beside val_wire.c, not in it: a response carries its trailer, so
 * the encoder needs the library's CPU CRC engine (cpu_crc32.c), and
 * val_wire.c links on its own (tests/test_header_surface.py builds it against
 * the reference's codec without the rest of the library).
 * Layout: reference src/val_core.c:775-811, trailer :828-834.
 */
#include "val_byte_order.h"
#include "val_wire.h"

#include "cpu_crc32.h"

uint32_t val_frame_put_response(uint8_t kind, uint64_t offset, uint32_t reason, uint8_t *out)
{
    if (!out)
        return 0;
    const uint32_t low = (uint32_t)(offset & 0xFFFFFFFFu), high = (uint32_t)(offset >> 32);
    uint16_t content = 0;
    if (kind == (uint8_t)VAL_PKT_DATA_ACK) {
        if (high) {
            content = 4u;
            val_put_le32(out + VAL_WIRE_HEADER_SIZE, high);
        }
    } else if (kind == (uint8_t)VAL_PKT_DATA_NAK) {
        content = 12u;
        val_put_le32(out + VAL_WIRE_HEADER_SIZE, high);
        val_put_le32(out + VAL_WIRE_HEADER_SIZE + 4u, reason);
        val_put_le32(out + VAL_WIRE_HEADER_SIZE + 8u, 0u);
    } else {
        return 0;
    }
    val_serialize_frame_header(kind, 0, content, low, out);
    const uint32_t used = VAL_WIRE_HEADER_SIZE + content;
    val_put_le32(out + used, vcrc_cpu_update(0xFFFFFFFFu, out, used) ^ 0xFFFFFFFFu);
    return used + VAL_WIRE_TRAILER_SIZE;
}
