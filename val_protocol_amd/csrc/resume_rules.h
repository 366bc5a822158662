/* resume_rules.h -- the three rules of a VAL_RESUME_TAIL handshake, stated
 * once for the host (val_wire.c exports them as val_resume_tail_window,
 * val_resume_request_window and val_resume_verdict; include/val_wire.h says
 * what they are) and for the device (windows_kernel.hpp applies them per
 * file). Plain C; all arithmetic is 64-bit and never wraps. */
#ifndef VAL_RESUME_RULES_H
#define VAL_RESUME_RULES_H

#include <stdint.h>

#include "val_wire.h"

#if defined(__HIPCC__)
#define VAL_RULE_FN __host__ __device__ static inline
#else
#define VAL_RULE_FN static inline
#endif

/* The cap on a tail window: tail_cap_bytes, 0 = the default, clamped to 1 .. 256 MiB. */
VAL_RULE_FN uint64_t val_rule_tail_cap(uint64_t tail_cap_bytes)
{
    const uint64_t cap = tail_cap_bytes ? tail_cap_bytes : VAL_RESUME_TAIL_CAP_DEFAULT;
    return cap > VAL_RESUME_TAIL_CAP_MAX ? VAL_RESUME_TAIL_CAP_MAX : cap; /* >= 1 */
}

/* The longest window the tail rule can ask for under a policy. */
VAL_RULE_FN uint64_t val_rule_tail_max_len(uint64_t tail_cap_bytes, uint64_t min_verify_bytes)
{
    const uint64_t cap = val_rule_tail_cap(tail_cap_bytes);
    return min_verify_bytes > cap ? min_verify_bytes : cap;
}

VAL_RULE_FN int val_rule_tail_window(uint64_t existing, uint64_t incoming, uint64_t tail_cap_bytes,
                                     uint64_t min_verify_bytes, int mismatch_skip, uint64_t *resume_offset,
                                     uint64_t *verify_len)
{
    *resume_offset = 0;
    *verify_len = 0;
    if (existing == 0)
        return VAL_RESUME_START_ZERO;
    if (existing > incoming)
        return mismatch_skip ? VAL_RESUME_SKIP_FILE : VAL_RESUME_START_ZERO;
    const uint64_t cap = val_rule_tail_cap(tail_cap_bytes);
    uint64_t vlen = existing < cap ? existing : cap;
    if (min_verify_bytes > 0 && vlen < min_verify_bytes)
        vlen = existing < min_verify_bytes ? existing : min_verify_bytes;
    *resume_offset = existing;
    *verify_len = vlen; /* 1 .. existing: the window [existing - vlen, existing) */
    return VAL_RESUME_VERIFY_FIRST;
}

VAL_RULE_FN int val_rule_request_window(uint64_t resume_offset, uint64_t verify_len, uint64_t *start, uint32_t *vlen32)
{
    const uint32_t v = (uint32_t)(verify_len > resume_offset ? resume_offset : verify_len); /* the reference's cast */
    *vlen32 = v;
    *start = resume_offset - v; /* v <= resume_offset */
    return v != 0;
}

VAL_RULE_FN val_status_t val_rule_verdict(int window_ok, uint32_t local_crc, uint32_t sender_crc, int mismatch_skip,
                                          uint64_t rec_resume_off, uint64_t file_size, uint64_t *resume_off_out)
{
    if (window_ok && local_crc == sender_crc) {
        *resume_off_out = rec_resume_off;
        return VAL_OK;
    }
    if (mismatch_skip) {
        *resume_off_out = file_size;
        return VAL_SKIPPED;
    }
    *resume_off_out = 0;
    return VAL_ERR_RESUME_VERIFY;
}

#endif /* VAL_RESUME_RULES_H */
