"""A second, independent reading of the baseline JPEG writer the GPU encoder reproduces: numpy float32 for the
transform, a plain Python bit writer for the entropy coding.  tests/c/jpeg_write_ref.c is the first reading; the CPU suite checks
that the two agree byte for byte, and the C one (faster) is the GPU suite's oracle.

Float constants are given as float32 bit patterns (the correctly rounded value of each decimal literal), so no decimal -> double ->
float double rounding can enter.  numpy rounds every float32 operation on its own (no contraction).
"""
import numpy as np


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


C_R_Y, C_G_Y, C_B_Y = _f(0x3E991687), _f(0x3F1645A2), _f(0x3DE978D5)          # 0.29900 0.58700 0.11400
C_R_U, C_G_U, HALF = _f(0x3E2CCA2E), _f(0x3EA99AE9), _f(0x3F000000)            # 0.16874 0.33126 0.5
C_G_V, C_B_V = _f(0x3ED65E89), _f(0x3DA685DB)                                  # 0.41869 0.08131
C4, C6, C2MC6, C2PC6 = _f(0x3F3504F3), _f(0x3EC3EF15), _f(0x3F0A8BD4), _f(0x3FA73D75)   # 0.707106781 0.382683433 0.541196100 1.306562965
QUARTER, F128 = _f(0x3E800000), np.float32(128)
_SQRT8 = _f(0x403504F3)                                                        # 2.828427125
_AASF_BASE = [_f(0x3F800000), _f(0x3FB18A86), _f(0x3FA73D75), _f(0x3F968317), _f(0x3F800000), _f(0x3F49234E), _f(0x3F0A8BD4),
              _f(0x3E8D42AF)]                                                  # 1, 1.387039845, 1.306562965, 1.175875602, 1, 0.785694958, 0.5411961, 0.275899379
AASF = np.array([np.float32(a * _SQRT8) for a in _AASF_BASE], np.float32)


def _zigzag_order():
    """natural index k -> zig-zag position, by walking the anti-diagonals (T.81 Figure A.6)"""
    pos = np.zeros(64, np.int64)
    n = 0
    for s in range(15):
        cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        if s % 2 == 0:
            cells.reverse()                    # even diagonals go up-right: row decreasing
        for r, c in cells:
            pos[r * 8 + c] = n
            n += 1
    return pos


ZIGZAG = _zigzag_order()

# T.81 Annex K.1: luminance and chrominance quantisation tables, natural order
LUMA_Q = np.array("""16 11 10 16 24 40 51 61 12 12 14 19 26 58 60 55 14 13 16 24 40 57 69 56 14 17 22 29 51 87 80 62
                     18 22 37 56 68 109 103 77 24 35 55 64 81 104 113 92 49 64 78 87 103 121 120 101 72 92 95 98 112 100 103 99""".split(), int)
CHROMA_Q = np.array([17, 18, 24, 47] + [99] * 4 + [18, 21, 26, 66] + [99] * 4 + [24, 26, 56] + [99] * 5 + [47, 66] + [99] * 38, int)

# T.81 Annex K.3: BITS (number of codes of each length 1..16) and HUFFVAL
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209 0a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa".replace(" ", "")),
           bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa".replace(" ", "")))
assert len(AC_VALS[0]) == len(AC_VALS[1]) == 162 == sum(AC_BITS[0]) == sum(AC_BITS[1])


def huffman(bits, vals):
    """symbol -> (code, length), T.81 Annex C; a symbol the table lacks maps to (0, 0)"""
    table = {}
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return [table.get(s, (0, 0)) for s in range(256)]


HDC = [huffman(DC_BITS[c], DC_VALS) for c in range(2)]
HAC = [huffman(AC_BITS[c], list(AC_VALS[c])) for c in range(2)]


def quality_setup(quality):
    """(subsample, luma table, chroma table) -- tables in zig-zag order as DQT carries them -- and the two fdtbl arrays"""
    quality = quality or 90
    sub = quality <= 90
    quality = min(max(quality, 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - quality * 2
    tabs = []
    for base in (LUMA_Q, CHROMA_Q):
        t = np.zeros(64, np.int64)
        t[ZIGZAG] = np.clip((base * scale + 50) // 100, 1, 255)
        tabs.append(t)
    fd = []
    for t in tabs:
        f = np.zeros(64, np.float32)
        for r in range(8):
            for c in range(8):
                k = r * 8 + c
                f[k] = np.float32(1) / ((np.float32(t[ZIGZAG[k]]) * AASF[r]) * AASF[c])
        fd.append(f.reshape(8, 8))
    return sub, tabs[0], tabs[1], fd


def _dct(a, axis):
    d = [np.take(a, i, axis=axis) for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o4 = t10 + t11, t10 - t11
    z1 = (t12 + t13) * C4
    o2, o6 = t13 + z1, t13 - z1
    t10, t11, t12 = t4 + t5, t5 + t6, t6 + t7
    z5 = (t10 - t12) * C6
    z2 = t10 * C2MC6 + z5
    z4 = t12 * C2PC6 + z5
    z3 = t11 * C4
    z11, z13 = t7 + z3, t7 - z3
    out = [o0, z11 + z4, o2, z13 - z2, o4, z13 + z2, o6, z11 - z4]
    return np.stack(out, axis=axis)


def _quantise(blocks, fd):
    """blocks (..., 8, 8) float32 samples -> (..., 64) ints in zig-zag order"""
    coef = _dct(_dct(blocks, -1), -2)
    v = coef * fd
    q = np.where(v < 0, v - HALF, v + HALF).astype(np.int32)          # truncation toward zero
    out = np.zeros(q.shape[:-2] + (64,), np.int32)
    out[..., ZIGZAG] = q.reshape(q.shape[:-2] + (64,))
    return out


def _to_blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def blocks(img, quality):
    """img: (h, w, comp) uint8.  Returns (subsample, tables, [(class, zig-zag coefficients)] in stream order)."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, comp = img.shape
    sub, qy, quv, fd = quality_setup(quality)
    m = 16 if sub else 8
    H, W = -(-h // m) * m, -(-w // m) * m
    p = np.pad(img, ((0, H - h), (0, W - w), (0, 0)), mode="edge").astype(np.float32)   # edge clamping
    r = p[:, :, 0]
    g = p[:, :, 1] if comp > 2 else r
    b = p[:, :, 2] if comp > 2 else r
    Y = ((C_R_Y * r + C_G_Y * g) + C_B_Y * b) - F128
    U = (-C_R_U * r - C_G_U * g) + HALF * b
    V = (HALF * r - C_G_V * g) - C_B_V * b
    qY = _quantise(_to_blocks(Y), fd[0])
    if sub:
        su = (((U[0::2, 0::2] + U[0::2, 1::2]) + U[1::2, 0::2]) + U[1::2, 1::2]) * QUARTER
        sv = (((V[0::2, 0::2] + V[0::2, 1::2]) + V[1::2, 0::2]) + V[1::2, 1::2]) * QUARTER
    else:
        su, sv = U, V
    qU, qV = _quantise(_to_blocks(su), fd[1]), _quantise(_to_blocks(sv), fd[1])
    out = []
    for my in range(qU.shape[0]):
        for mx in range(qU.shape[1]):
            if sub:
                for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    out.append((0, qY[2 * my + dy, 2 * mx + dx]))
            else:
                out.append((0, qY[my, mx]))
            out.append((1, qU[my, mx]))
            out.append((2, qV[my, mx]))
    return sub, (qy, quv), out


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        for i in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((v >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc = self.n = 0


def _size(v):
    return abs(int(v)).bit_length() or 1


def _magnitude(v, n):
    return (v - 1 if v < 0 else v) & ((1 << n) - 1)


def header(w, h, sub, qy, quv):
    hdr = bytearray(b"\xFF\xD8\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    hdr += b"\xFF\xDB\x00\x84\x00" + bytes(int(x) for x in qy) + b"\x01" + bytes(int(x) for x in quv)
    hdr += bytes([0xFF, 0xC0, 0, 0x11, 8, h >> 8 & 255, h & 255, w >> 8 & 255, w & 255, 3, 1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    hdr += b"\xFF\xC4\x01\xA2"
    for cls in range(2):
        hdr += bytes([cls]) + bytes(DC_BITS[cls]) + bytes(DC_VALS)
        hdr += bytes([0x10 | cls]) + bytes(AC_BITS[cls]) + AC_VALS[cls]
    hdr += b"\xFF\xDA\x00\x0C\x03\x01\x00\x02\x11\x03\x11\x00\x3F\x00"
    assert len(hdr) == 607
    return bytes(hdr)


def encode(img, quality=90):
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    sub, (qy, quv), blks = blocks(img, quality)
    bw = BitWriter()
    pred = [0, 0, 0]
    for comp_id, du in blks:
        cls = 0 if comp_id == 0 else 1
        du = [int(x) for x in du]
        diff = du[0] - pred[comp_id]
        pred[comp_id] = du[0]
        if diff == 0:
            bw.bits(*HDC[cls][0])
        else:
            n = _size(diff)
            bw.bits(*HDC[cls][n])
            bw.bits(_magnitude(diff, n), n)
        nz = [k for k in range(1, 64) if du[k]]
        if not nz:
            bw.bits(*HAC[cls][0])
            continue
        last = 0
        for k in nz:
            run = k - last - 1
            while run >= 16:
                bw.bits(*HAC[cls][0xF0])
                run -= 16
            n = _size(du[k])
            bw.bits(*HAC[cls][((run << 4) + n) & 255])
            bw.bits(_magnitude(du[k], n), n)
            last = k
        if nz[-1] != 63:
            bw.bits(*HAC[cls][0])
    bw.bits(0x7F, 7)
    return header(w, h, sub, qy, quv) + bytes(bw.out) + b"\xFF\xD9"
