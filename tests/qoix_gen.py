"""Writers of QOIX test files, from the format description (no code of the reference): op builders, a plain QOI2AVG encoder, an LZ4
block writer that takes explicit (literals, offset, match length) sequences, a small greedy matcher and the 25-byte container."""
import struct

import numpy as np

PAD = b"\xff\xff\xff\xff"                                                   # the four closing bytes; the decoder never looks at them


# ---- ops (first byte ranges: < 0x80 LUMA, < 0xc0 INDEX, < 0xe0 LUMA2, < 0xe8 LUMA3, < 0xf0 ADIFF, < 0xf8 RUN, < 0xfc RUN2, fc GRAY, fd RGB, fe RGBA, ff END)
def LUMA(vg, fr, fb):
    """green delta vg in -4..3; fr / fb: the 2-bit red / blue fields (red = ref + vg - bias + fr, bias 1 when vg < 0 else 2)"""
    assert -4 <= vg <= 3 and 0 <= fr <= 3 and 0 <= fb <= 3
    return bytes([(vg + 4) << 4 | fr << 2 | fb])


def INDEX(i):
    return bytes([0x80 | (i & 63)])


def LUMA2(vg, fr, fb):
    """vg in -16..15; fr / fb 4-bit fields (red = ref + vg - 8 + fr)"""
    assert -16 <= vg <= 15 and 0 <= fr <= 15 and 0 <= fb <= 15
    return bytes([0xc0 | (vg + 16), fr << 4 | fb])


def LUMA3(vg, fr, fb):
    """vg in -64..63; fr / fb 6-bit fields (red = ref + vg + fr - 32)"""
    assert -64 <= vg <= 63 and 0 <= fr <= 63 and 0 <= fb <= 63
    v = 0xe00000 | (vg + 64) << 12 | fr << 6 | fb
    return bytes([v >> 16, (v >> 8) & 255, v & 255])


def ADIFF(d):
    assert -4 <= d <= 3
    return bytes([0xe8 | (d + 4)])


def RUN(pixels):
    """the current pixel `pixels` times (1..8): the op's own pixel and pixels - 1 further ones"""
    assert 1 <= pixels <= 8
    return bytes([0xf0 | (pixels - 1)])


def RUN2(pixels):
    assert 1 <= pixels <= 1024
    return bytes([0xf8 | (pixels - 1) >> 8, (pixels - 1) & 255])


def GRAY(v): return bytes([0xfc, v])
def RGB(r, g, b): return bytes([0xfd, r, g, b])
def RGBA(r, g, b, a): return bytes([0xfe, r, g, b, a])
END = b"\xff"


def header(w, h, channels=3, colorspace=0, version=1, bitdepth=8, compression=0, par=1.0, dpi=96.0, magic=b"qoix"):
    par = par if isinstance(par, bytes) else struct.pack(">f", par)
    dpi = dpi if isinstance(dpi, bytes) else struct.pack(">f", dpi)
    return magic + struct.pack(">IIBBBBB", w, h, version, channels, bitdepth, colorspace, compression) + par + dpi


def stored(w, h, ops, channels=3, pad=PAD, **kw):
    """an uncompressed file: header, op bytes, closing bytes"""
    return header(w, h, channels, **kw) + bytes(ops) + pad


# ---- LZ4 blocks
def _length(n):
    """the extension bytes of a length field whose nibble is 15"""
    out = b""
    n -= 15
    while n >= 255:
        out += b"\xff"; n -= 255
    return out + bytes([n])


def lz4_block(seqs, last_literals):
    """seqs: [(literals, offset, match_len >= 4)], then a final run of literals.  Nothing is checked: a test may write what no encoder would."""
    out = bytearray()
    for lit, off, ml in seqs:
        lit = bytes(lit)
        m = ml - 4
        out.append(min(len(lit), 15) << 4 | min(m, 15))
        if len(lit) >= 15:
            out += _length(len(lit))
        out += lit + struct.pack("<H", off)
        if m >= 15:
            out += _length(m)
    last_literals = bytes(last_literals)
    out.append(min(len(last_literals), 15) << 4)
    if len(last_literals) >= 15:
        out += _length(len(last_literals))
    return bytes(out + last_literals)


def lz4_greedy(data):
    """-> (seqs, last_literals) for lz4_block: the longest-first-seen match by a 4-byte hash, within the format's end rules (the last
    match begins at least 12 bytes before the end, the last 5 bytes are literals)"""
    data = bytes(data)
    n, seen, seqs = len(data), {}, []
    i = anchor = 0
    while i + 12 <= n:
        key = data[i:i + 4]
        j = seen.get(key)
        seen[key] = i
        if j is None or i - j > 65535:
            i += 1
            continue
        k = 4
        while i + k < n - 5 and data[j + k] == data[i + k]:
            k += 1
        seqs.append((data[anchor:i], i - j, k))
        i += k
        anchor = i
    return seqs, data[anchor:]


def compressed(w, h, ops, channels=3, pad=PAD, block=None, orig=None, **kw):
    """an LZ4 file of the same op stream; block: the LZ4 bytes if not the greedy matcher's; orig: the claim if not the truth"""
    body = bytes(ops) + pad
    if block is None:
        block = lz4_block(*lz4_greedy(body))
    return header(w, h, channels, compression=1, **kw) + struct.pack(">I", len(body) if orig is None else orig) + bytes(block)


# ---- the encoder
def _loco(a, b, c):
    lo, hi = min(a, b), max(a, b)
    return hi if c <= lo else lo if c >= hi else a + b - c


def _s8(v):
    v &= 255
    return v - 256 if v >= 128 else v


def encode_ops(img):
    """(h, w, 3 or 4) uint8 -> op bytes: runs, INDEX hits, ADIFF for small alpha steps, the shortest LUMA form that fits, else GRAY / RGB / RGBA"""
    h, w, ch = img.shape
    rgba = np.full((h, w, 4), 255, np.uint8)
    rgba[..., :ch] = img
    flat = [tuple(int(v) for v in p) for p in rgba.reshape(-1, 4)]
    out = bytearray()
    px, fifo, nfifo, i, n = (0, 0, 0, 255), [(0, 0, 0, 0)] * 64, 0, 0, w * h
    while i < n:
        y, x = divmod(i, w)
        if y == 0:
            ref = px[:3]
        elif x == 0:
            ref = flat[i - w][:3]
        else:
            ref = tuple(_loco(flat[i - 1][k], flat[i - w][k], flat[i - w - 1][k]) for k in range(3))
        t = flat[i]
        if t == px:
            k = 1
            while i + k < n and flat[i + k] == px and k < 1024:
                k += 1
            out += RUN(k) if k <= 8 else RUN2(k)
            i += k
            continue
        if t in fifo:
            out += INDEX(fifo.index(t)); px = t; i += 1
            continue
        da = _s8(t[3] - px[3])
        if da and not -4 <= da <= 3:
            out += RGBA(*t)
        else:
            if da:
                out += ADIFF(da)
            vg = _s8(t[1] - ref[1])
            dr, db = _s8(t[0] - ref[0] - vg), _s8(t[2] - ref[2] - vg)
            bias = 1 if vg < 0 else 2
            if -4 <= vg <= 3 and -bias <= dr <= 3 - bias and -bias <= db <= 3 - bias:
                out += LUMA(vg, dr + bias, db + bias)
            elif -16 <= vg <= 15 and -8 <= dr <= 7 and -8 <= db <= 7:
                out += LUMA2(vg, dr + 8, db + 8)
            elif -64 <= vg <= 63 and -32 <= dr <= 31 and -32 <= db <= 31:
                out += LUMA3(vg, dr + 32, db + 32)
            elif t[0] == t[1] == t[2]:
                out += GRAY(t[0])
            else:
                out += RGB(*t[:3])
        fifo[nfifo & 63] = t; nfifo += 1
        px = t; i += 1
    return bytes(out)


def encode(img, lz4=False, **kw):
    h, w, ch = img.shape
    ops = encode_ops(img)
    return compressed(w, h, ops, ch, **kw) if lz4 else stored(w, h, ops, ch, **kw)


def photo_like(w, h, ch=3, seed=0):
    """smooth gradients plus noise: mostly LUMA ops"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 23.0 + k) * np.cos(yy / 17.0 - k) for k in range(ch)], -1)
    img = np.clip(base + rng.normal(0, 3, (h, w, ch)), 0, 255).astype(np.uint8)
    if ch == 4:
        img[..., 3] = np.clip(200 + 50 * np.sin(xx / 40.0), 0, 255).astype(np.uint8)
    return img


def flat_image(w, h, ch=3, seed=0):
    """a few flat rectangles: runs and INDEX hits, compresses well"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, ch), np.uint8)
    img[...] = rng.integers(0, 256, ch)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(1, h // 2 + 2)), x0:x0 + int(rng.integers(1, w // 2 + 2))] = rng.integers(0, 256, ch)
    return img
