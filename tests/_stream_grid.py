"""CPU model of the streaming frame geometry measured by bench/micro/mb16.hip
(DESIGN_EXPERIMENTS A17): the unit grid of a long frame anchored at
floor128(frame end), so that every round after round 0 is whole 128-B lines of
its frame and can be fetched by LDS-DMA, one request per line; the batch image
a wave's DMA instructions leave in LDS; and the rotated compact slice tables.
Beside tests/test_unit_grid_model.py, whose grid is anchored at floor4(end).
"""
import zlib

M = 0xFFFFFFFF
POLY = 0xEDB88320
ONE = 0x80000000  # x^0, reflected
X8 = 0x00800000   # x^8
LINE = 128
UNIT = 64


def gf2_mul(a: int, b: int) -> int:
    prod = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            prod ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return prod


def gf2_pow(x: int, n: int) -> int:
    r = ONE
    while n:
        if n & 1:
            r = gf2_mul(r, x)
        x = gf2_mul(x, x)
        n >>= 1
    return r


def raw_update(reg: int, data: bytes) -> int:
    """Raw (no pre/post inversion) register update, via zlib's finished CRC."""
    return (~zlib.crc32(data, (~reg) & M)) & M


class Grid:
    """Geometry of one frame at address fp (any byte alignment), L bytes, G lanes.

    tail   T = min((fp + L) mod 128, L) bytes past the grid, fed after the merge
    Lg     bytes on the grid, U units of 64 B counted back from the grid end E,
           R rounds of G units; unit 0 front-padded with pad virtual zero bytes
    head   [fp, body) read by ordinary loads (round 0: unit 0 from inside the
           frame's first line, the other units whole)
    body   [body, E): rounds 1..R-1, whole lines, one DMA request per line
    Frames with Lg < 4 take the byte path (no grid: everything is head)."""

    def __init__(self, fp: int, L: int, G: int):
        self.fp, self.L, self.G = fp, L, G
        self.T = min((fp + L) % LINE, L)
        self.Lg = L - self.T
        self.E = fp + self.Lg
        self.tiny = self.Lg < 4
        self.U = -(-self.Lg // UNIT) if self.Lg else 1
        self.R = -(-self.U // G)
        self.pad = UNIT * self.U - self.Lg
        self.body = fp if self.tiny else self.E - (self.R - 1) * G * UNIT

    def head_range(self):
        return (self.fp, self.fp + self.L) if self.tiny else (self.fp, self.body)

    def tail_range(self):
        return (self.fp + self.L, self.fp + self.L) if self.tiny else (self.E, self.fp + self.L)

    def round_lines(self, k: int):
        """Line addresses of round k >= 1 (G * 64 / 128 lines)."""
        assert 1 <= k < self.R
        lo = self.body + (k - 1) * self.G * UNIT
        return list(range(lo, lo + self.G * UNIT, LINE))

    def body_lines(self):
        if self.tiny:
            return []
        return [a for k in range(1, self.R) for a in self.round_lines(k)]


def model_frame(mem: bytes, fp: int, L: int, G: int, seed: int = M, xorout: int = M) -> int:
    """The frame's CRC by the streaming decomposition (as the kernel computes it)."""
    gr = Grid(fp, L, G)
    if gr.tiny:
        return raw_update(seed, mem[fp:fp + L]) ^ xorout
    frame = bytearray(mem[fp:fp + gr.Lg])
    for j in range(4):  # seed XORed into frame bytes 0..3
        frame[j] ^= (seed >> (8 * j)) & 0xFF
    grid = bytes(gr.pad) + bytes(frame)
    gap = gf2_pow(X8, UNIT * (G - 1))
    lanes = []
    for g in range(G):
        acc = 0
        for k in range(gr.R):
            u = gr.U - G * gr.R + g + G * k
            if k > 0:
                acc = gf2_mul(acc, gap)
            if u >= 0:
                acc = raw_update(acc, grid[UNIT * u:UNIT * u + UNIT])
        lanes.append(acc)
    width = 1
    while width < G:
        sh = gf2_pow(X8, UNIT * width)
        lanes = [gf2_mul(lanes[i], sh) ^ lanes[i + 1] for i in range(0, len(lanes), 2)]
        width *= 2
    return raw_update(lanes[0], mem[gr.E:fp + L]) ^ xorout  # the tail, after the merge


# ---- the batch image of one wave round (mb16.hip ring_group) ------------------
# A wave hashes 64 / G frames, hash lane m = frame (m // G), unit (m % G). Its
# 4 KiB slot holds unit m at 64 m with 16-B piece k at position (k + (m >> 2)) & 3.
# DMA instruction q, lane l writes slot + 1024 q + 16 l (lane-linear).

# lanes one pass of a ds_read_b128 serves together (MI355X LDS)
B128_PASSES = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               [32 + x for x in list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))],
               [32 + x for x in list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]]


def dma_source(q: int, l: int, G: int):
    """(frame in the wave, byte offset in the frame's round) DMA lane l of instruction q fetches."""
    m = 16 * q + (l >> 2)
    k = ((l & 3) - (m >> 2)) & 3
    return m // G, (m % G) * UNIT + 16 * k


def readback_offset(lane: int, k: int) -> int:
    """Slot offset of hash lane `lane`'s k-th ds_read_b128 (piece k of its unit)."""
    return lane * UNIT + 16 * ((k + (lane >> 2)) & 3)


# ---- rotated compact tables -------------------------------------------------
# Row per byte value, slot s = T_{3-s}, which consumes byte s of the word.
def lookup_64k(lane: int, i: int):
    """(slot, LDS byte address for byte value b -> lambda) of lookup instruction i: 16 replicas, 256-B rows."""
    c = (lane >> 4) & 1
    slot = (c, 1 - c, 2 + c, 3 - c)[i]
    return slot, lambda b: b * 256 + slot * 64 + (lane & 15) * 4


def lookup_32k(lane: int, i: int):
    """8 replicas, 128-B rows, lane class c = (lane >> 3) & 3 reads slot (i + c) & 3."""
    slot = (i + ((lane >> 3) & 3)) & 3
    return slot, lambda b: b * 128 + slot * 32 + (lane & 7) * 4
