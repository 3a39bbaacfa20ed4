"""A BC7 decoder for modes 1 and 6, from the format's definition (the BPTC chapter of the Khronos Data Format Specification), independent
of the encoder under test.  decode(block) -> (16, 4) uint8 rgba.

A block is 128 bits, least significant bit of byte 0 first.  The mode is the number of zero bits before the first one.
  mode 1: 2 subsets; 6 partition bits; per channel r, g, b: endpoint 0 and 1 of subset 0, then of subset 1, 6 bits each; one p-bit per
          subset, shared by its two endpoints; 3-bit indices, the anchor pixel of each subset one bit short; alpha is 255.
  mode 6: 1 subset; per channel r, g, b, a: endpoint 0, endpoint 1, 7 bits each; a p-bit per endpoint; 4-bit indices, pixel 0 one short.
An endpoint channel is (bits << 1 | p-bit), widened to 8 bits by repeating its high bits; a pixel is
(e0 * (64 - w) + e1 * w + 32) >> 6 with w the weight of its index."""
import numpy as np

WEIGHTS3 = (0, 9, 18, 27, 37, 46, 55, 64)
WEIGHTS4 = (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)

# the 64 two-subset partitions, four rows of four pixels each, '1' = subset 1
_ROWS = """
0011 0011 0011 0011|0001 0001 0001 0001|0111 0111 0111 0111|0001 0011 0011 0111|0000 0001 0001 0011|0011 0111 0111 1111|0001 0011 0111 1111|0000 0001 0011 0111
0000 0000 0001 0011|0011 0111 1111 1111|0000 0001 0111 1111|0000 0000 0001 0111|0001 0111 1111 1111|0000 0000 1111 1111|0000 1111 1111 1111|0000 0000 0000 1111
0000 1000 1110 1111|0111 0001 0000 0000|0000 0000 1000 1110|0111 0011 0001 0000|0011 0001 0000 0000|0000 1000 1100 1110|0000 0000 1000 1100|0111 0011 0011 0001
0011 0001 0001 0000|0000 1000 1000 1100|0110 0110 0110 0110|0011 0110 0110 1100|0001 0111 1110 1000|0000 1111 1111 0000|0111 0001 1000 1110|0011 1001 1001 1100
0101 0101 0101 0101|0000 1111 0000 1111|0101 1010 0101 1010|0011 0011 1100 1100|0011 1100 0011 1100|0101 0101 1010 1010|0110 1001 0110 1001|0101 1010 1010 0101
0111 0011 1100 1110|0001 0011 1100 1000|0011 0010 0100 1100|0011 1011 1101 1100|0110 1001 1001 0110|0011 1100 1100 0011|0110 0110 1001 1001|0000 0110 0110 0000
0100 1110 0100 0000|0010 0111 0010 0000|0000 0010 0111 0010|0000 0100 1110 0100|0110 1100 1001 0011|0011 0110 1100 1001|0110 0011 1001 1100|0011 1001 1100 0110
0110 1100 1100 1001|0110 0011 0011 1001|0111 1110 1000 0001|0001 1000 1110 0111|0000 1111 0011 0011|0011 0011 1111 0000|0010 0010 1110 1110|0100 0100 0111 0111
"""
PARTITIONS = [[int(ch) for ch in p.replace(" ", "")] for line in _ROWS.strip().splitlines() for p in line.split("|")]
assert len(PARTITIONS) == 64 and all(len(p) == 16 and p[0] == 0 for p in PARTITIONS)

ANCHOR_SECOND = (15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
                 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
                 15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6,
                 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15)
assert all(PARTITIONS[p][ANCHOR_SECOND[p]] == 1 for p in range(64))


class _Bits:
    def __init__(self, block):
        self.v = int.from_bytes(bytes(block), "little")
        self.pos = 0

    def take(self, n):
        r = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return r


def mode_of(block):
    b0 = bytes(block)[0]
    for m in range(8):
        if (b0 >> m) & 1:
            return m
    return -1


def _widen(v, bits):
    v <<= 8 - bits
    return v | (v >> bits)


def decode(block):
    block = bytes(block)
    assert len(block) == 16
    mode = mode_of(block)
    if mode not in (1, 6):
        raise ValueError(f"mode {mode} is not decoded here")
    b = _Bits(block)
    b.take(mode + 1)
    out = np.zeros((16, 4), np.uint8)
    if mode == 6:
        ep = [[0] * 4, [0] * 4]
        for c in range(4):
            for e in range(2):
                ep[e][c] = b.take(7)
        pb = [b.take(1), b.take(1)]
        ep = [[_widen(ep[e][c] << 1 | pb[e], 8) for c in range(4)] for e in range(2)]
        for i in range(16):
            w = WEIGHTS4[b.take(3 if i == 0 else 4)]
            out[i] = [(ep[0][c] * (64 - w) + ep[1][c] * w + 32) >> 6 for c in range(4)]
        assert b.pos == 128
        return out
    part = b.take(6)
    ep = [[[0] * 3 for _ in range(2)] for _ in range(2)]          # [subset][endpoint][channel]
    for c in range(3):
        for s in range(2):
            for e in range(2):
                ep[s][e][c] = b.take(6)
    pb = [b.take(1), b.take(1)]
    ep = [[[_widen(ep[s][e][c] << 1 | pb[s], 7) for c in range(3)] for e in range(2)] for s in range(2)]
    anchors = (0, ANCHOR_SECOND[part])
    for i in range(16):
        s = PARTITIONS[part][i]
        w = WEIGHTS3[b.take(2 if i in anchors else 3)]
        out[i] = [(ep[s][0][c] * (64 - w) + ep[s][1][c] * w + 32) >> 6 for c in range(3)] + [255]
    assert b.pos == 128
    return out


# the encoder's yardstick (bc7enc16's perceptual distance on the weights 128, 64, 16, 32 as compress_block scales them), restated
# here so the tests can weigh decoded pixels without calling anything under test
ERR_WEIGHTS = (512, 103, 18, 128)


def perceptual_error(decoded, source, with_alpha):
    total = 0
    for d, s in zip(np.asarray(decoded, np.int64).reshape(16, 4).tolist(), np.asarray(source, np.int64).reshape(16, 4).tolist()):
        l1, l2 = d[0] * 109 + d[1] * 366 + d[2] * 37, s[0] * 109 + s[1] * 366 + s[2] * 37
        dl, dcr, dcb = (l1 - l2) >> 8, ((d[0] * 512 - l1) - (s[0] * 512 - l2)) >> 8, ((d[2] * 512 - l1) - (s[2] * 512 - l2)) >> 8
        total += ERR_WEIGHTS[0] * dl * dl + ERR_WEIGHTS[1] * dcr * dcr + ERR_WEIGHTS[2] * dcb * dcb
        if with_alpha:
            total += ERR_WEIGHTS[3] * (d[3] - s[3]) ** 2
    return total
