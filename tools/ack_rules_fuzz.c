/*
 * ack_rules_fuzz.c -- a stand-alone fuzz of the DATA_ACK / DATA_NAK host rules
 * (include/val_wire.h) for a sanitizer build on the CPU:
 *
 *   gcc -std=gnu99 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Iinclude -Ival_protocol_amd/csrc tools/ack_rules_fuzz.c \
 *       val_protocol_amd/csrc/val_wire.c val_protocol_amd/csrc/val_ack.c \
 *       val_protocol_amd/csrc/cpu_crc32.c -o ack_rules_fuzz && ./ack_rules_fuzz
 *
 * Every array is allocated at exactly the size the header asks for, so a
 * write past 2n responses or a read past n frames is a report. Beside memory
 * safety it checks what must hold for any input: the accepted set and the
 * final position are val_frame_accept's, responses come in frame order and
 * carry the position of their moment, every encoded response scans and parses
 * back to itself, and val_frame_apply_acks keeps last_acked <= next and, from
 * a last_acked inside the file, last_acked <= file_size.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "val_wire.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s (case %u)\n", __FILE__, __LINE__, #c, iter); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main(void)
{
    static const uint64_t starts[] = {0, 17, 0xFFFFF000ull, 0x100000005ull, UINT64_MAX - 5000};
    static const uint32_t strides[] = {0, 1, 2, 3, 64, UINT32_MAX};
    unsigned long responses = 0;
    for (unsigned iter = 0; iter < 20000; iter++) {
        const uint32_t n = (uint32_t)(rnd() % 48);
        const uint64_t w0 = starts[rnd() % 5];
        const uint32_t stride = strides[rnd() % 6];
        uint64_t *fo = malloc(n * sizeof *fo + 1), *dst = malloc(n * sizeof *dst + 1);
        uint32_t *pl = malloc(n * sizeof *pl + 1);
        uint8_t *ok = malloc(n + 1u);
        uint32_t *rf = malloc(2u * n * sizeof *rf + 1);
        uint8_t *rk = malloc(2u * n + 1u);
        uint64_t *ro = malloc(2u * n * sizeof *ro + 1);
        uint64_t w = w0, span = 0;
        for (uint32_t i = 0; i < n; i++) {
            const unsigned r = (unsigned)(rnd() % 100);
            pl[i] = rnd() % 10 ? (uint32_t)(rnd() % 3000) : (rnd() % 2 ? 0u : UINT32_MAX);
            ok[i] = r >= 90 ? 0 : 1;
            if (r < 55) {
                fo[i] = rnd() % 2 ? w : VAL_FRAME_OFFSET_IMPLIED;
                w += pl[i];
            } else if (r < 65) {
                fo[i] = w - rnd() % 4000; /* may wrap: any value is an input */
            } else if (r < 75) {
                fo[i] = w + 1 + rnd() % 4000;
            } else if (r < 82) {
                fo[i] = VAL_FRAME_OFFSET_NOT_DATA;
            } else {
                fo[i] = rnd();
            }
            span += pl[i];
        }
        const uint64_t cap = rnd() % 3 ? UINT64_MAX : w0 + span / 2;
        const uint64_t total = rnd() % 4 ? w0 + span / 3 : (rnd() % 2 ? 0 : UINT64_MAX);
        uint64_t wa = w0, wr = w0;
        uint32_t nacc = 0, novf = 0, nr = 0, since = (uint32_t)(rnd() % 3 ? rnd() % 70 : UINT32_MAX);
        const uint8_t *okp = rnd() % 8 ? ok : NULL;
        val_frame_accept(fo, pl, okp, n, cap, &wa, dst, &nacc, &novf);
        val_frame_respond_window(fo, pl, okp, n, cap, total, stride, &wr, stride ? &since : NULL, rf, rk, ro, &nr);
        CHECK(wr == wa);
        CHECK(nr <= 2u * n);
        CHECK(!stride || since < stride || nacc == 0);
        uint8_t wirebuf[2 * 48 * VAL_WIRE_RESPONSE_MAX];
        uint32_t used = 0;
        for (uint32_t r = 0; r < nr; r++) {
            CHECK(rf[r] < n && (r == 0 || rf[r] >= rf[r - 1]));
            CHECK(rk[r] == VAL_PKT_DATA_ACK || rk[r] == VAL_PKT_DATA_NAK);
            CHECK(r == 0 || ro[r] >= ro[r - 1]);
            CHECK(ro[r] >= w0 && ro[r] <= wa);
            used += val_frame_put_response(rk[r], ro[r], VAL_NAK_REASON_GAP, wirebuf + used);
        }
        responses += nr;
        /* the wire bytes scan and parse back */
        uint64_t *so = malloc(nr * sizeof *so + 1), *ao = malloc(nr * sizeof *ao + 1);
        uint32_t *sl = malloc(nr * sizeof *sl + 1);
        uint8_t *kd = malloc(nr + 1u);
        uint32_t nf = 0;
        size_t consumed = 0;
        CHECK(val_frame_scan(wirebuf, used, 64, nr, so, sl, &nf, &consumed) == VAL_OK);
        CHECK(nf == nr && consumed == used);
        val_frame_ack_offsets(wirebuf, so, sl, nf, kd, ao);
        for (uint32_t r = 0; r < nr; r++)
            CHECK(kd[r] == rk[r] && ao[r] == ro[r]);
        /* the sender's side over them, with a few frames declared corrupt */
        for (uint32_t r = 0; r < nr; r++)
            kd[r] = rnd() % 10 ? kd[r] : (uint8_t)(rnd() % 16);
        uint8_t *vk = malloc(nr + 1u);
        for (uint32_t r = 0; r < nr; r++)
            vk[r] = rnd() % 12 ? 1 : 0;
        const uint64_t fsize = rnd() % 2 ? wa : w0 + span / 4;
        uint64_t la = w0 <= fsize ? w0 : fsize, nx = la + rnd() % 3000;
        if (nx < la)
            nx = la;
        uint32_t retr = 0, ncrc = 0;
        val_frame_apply_acks(kd, ao, rnd() % 8 ? vk : NULL, nr, fsize, &la, &nx, &retr, &ncrc);
        CHECK(la <= fsize && la <= nx && ncrc <= retr && retr <= nr);
        val_frame_apply_acks(kd, ao, vk, nr, fsize, &la, &nx, NULL, NULL);
        free(fo), free(dst), free(pl), free(ok), free(rf), free(rk), free(ro);
        free(so), free(ao), free(sl), free(kd), free(vk);
    }
    printf("ack_rules_fuzz: 20000 windows, %lu responses, clean\n", responses);
    return 0;
}
