"""A second, independent reading of the GIF writer (saveGIF over msf_gif: codecs/msf_gif.d) in numpy and plain Python, for the
"two readings" check against tests/c/gif_encode_ref.c.  It is organised differently on purpose: cooking is one vectorised expression,
the translation table is a sorted list, the LZW dictionary is a Python dict keyed by (prefix, colour), and the sub-block framing is
"chunk the packed code stream by 255" instead of the reference's rolling block buffer."""
import numpy as np

RBITS = (0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
GBITS = (0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6)
BBITS = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5)
# (short)((255.0f - ((1 << (8 - bits)) - 1)) / 255.0f * 257) for bits 0..6, checked against the float expression on import
MUL = (0, 129, 193, 225, 241, 249, 253)
for _bits, _m in enumerate(MUL):
    _f = (np.float32(255.0) - np.float32((1 << (8 - _bits)) - 1)) / np.float32(255.0) * np.float32(257)
    assert _f.dtype == np.float32 and int(_f) == _m, (_bits, _f)
DITHER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64) << 12


def bit_log(i):
    return max(1, int(i).bit_length())


def cook(frame, depth, alpha_threshold):
    """(h, w, 4) uint8 -> cooked values (h, w) int64; transparent pixels are 1 << depth"""
    rb, gb, bb = RBITS[depth], GBITS[depth], BBITS[depth]
    h, w = frame.shape[:2]
    k = np.tile(DITHER, ((h + 3) // 4, (w + 3) // 4))[:h, :w]
    p = frame.astype(np.int64)
    r = np.minimum(65535, p[..., 0] * MUL[rb] + (k >> rb)) >> (16 - rb)
    g = np.minimum(65535, p[..., 1] * MUL[gb] + (k >> gb)) >> (16 - gb)
    b = np.minimum(65535, p[..., 2] * MUL[bb] + (k >> bb)) >> (16 - bb)
    v = r | g << rb | b << (rb + gb)
    return np.where(p[..., 3] < alpha_threshold, 1 << depth, v)


def replicate(v, bits):
    if bits == 0:
        return 0
    v <<= 8 - bits
    return (v | v >> bits | v >> (2 * bits) | v >> (3 * bits)) & 255


def encode(frames, centiseconds=7, max_bit_depth=16, alpha_threshold=10):
    """frames: (n, h, w, 4) uint8 -> file bytes"""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    assert 1 <= w <= 65535 and 1 <= h <= 65535 and n >= 1
    max_bit_depth = max(1, min(16, max_bit_depth))
    out = bytearray(b"GIF89a" + w.to_bytes(2, "little") + h.to_bytes(2, "little") + b"\x70\0\0" + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\0\0\0")
    prev_depth, prev_count, prev_cooked, prev_block = 0, 0, None, None
    for f in range(n):
        depth = min(max_bit_depth, prev_depth + 160 // max(1, prev_count))
        while True:
            cooked = cook(frames[f], depth, alpha_threshold)
            values = np.unique(cooked)
            colours = [int(v) for v in values if v != 1 << depth]
            if len(colours) >= 256 and depth > 1:
                depth -= 1
                continue
            break
        has_transparent = bool((cooked == 1 << depth).any())
        rb, gb, bb = RBITS[depth], GBITS[depth], BBITS[depth]
        index_of = {v: i + 1 for i, v in enumerate(colours)}
        index_of[1 << depth] = 0
        table_bits = max(2, bit_log(len(colours)))
        table_size = 1 << table_bits
        palette = bytearray(3 * table_size)
        for v, i in index_of.items():
            if i:
                palette[3 * i:3 * i + 3] = bytes((replicate(v & ((1 << rb) - 1), rb), replicate(v >> rb & ((1 << gb) - 1), gb), replicate(v >> (rb + gb), bb)))
        compatible = f > 0 and depth == prev_depth and not has_transparent
        if has_transparent and f > 0:
            out[prev_block + 3] = 0x09
        prev_block = len(out)
        out += b"\x21\xF9\x04\x05" + (centiseconds & 0xFFFF).to_bytes(2, "little") + b"\0\0\x2C\0\0\0\0" + w.to_bytes(2, "little") + h.to_bytes(2, "little")
        out.append(0x80 | (table_bits - 1))
        out += palette
        out.append(table_bits)
        flat = cooked.reshape(-1)
        idx = np.array([index_of[int(v)] for v in values], np.int64)[np.searchsorted(values, flat)]
        if compatible:
            idx = np.where(flat == prev_cooked.reshape(-1), 0, idx)
        # greedy LZW into one big integer of bits
        acc, nbits = 0, 0

        def put(code, width):
            nonlocal acc, nbits
            acc |= code << nbits
            nbits += width

        table, length = {}, table_size + 2
        put(table_size, bit_log(length - 1))
        last = int(idx[0])
        for c in idx[1:].tolist():
            code = table.get((last, c))
            if code is not None:
                last = code
                continue
            width = bit_log(length - 1)
            put(last, width)
            if length > 4095:
                put(table_size, width)
                table, length = {}, table_size + 2
            else:
                table[(last, c)] = length
                length += 1
            last = c
        put(last, min(12, bit_log(length - 1)))
        put(table_size + 1, min(12, bit_log(length)))
        stream = acc.to_bytes((nbits + 7) // 8, "little")
        for at in range(0, len(stream), 255):
            chunk = stream[at:at + 255]
            out.append(len(chunk))
            out += chunk
        out.append(0)
        prev_depth, prev_count, prev_cooked = depth, len(colours), cooked
    out.append(0x3B)
    return bytes(out)
