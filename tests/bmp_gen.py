"""A small BMP writer for the tests: every variant the reference's loader (stbi__bmp_load, codecs/stbdec.d:2112-2512) distinguishes --
header sizes 12 / 40 / 56 / 108 / 124, depths 1 / 4 / 8 / 16 / 24 / 32, compression 0 / 3 with arbitrary masks, top-down and
bottom-up, palettes shorter than 2^bpp, a gap between palette and pixels, density fields.  Pixel bytes (row padding included) are
random unless given."""
import struct

import numpy as np

HEADER_SIZES = (12, 40, 56, 108, 124)
DEPTHS = (1, 4, 8, 16, 24, 32)


def row_stride(w, bpp):
    return ((w * bpp + 7) // 8 + 3) & ~3


def make(w, h, bpp, hsz=40, compression=0, masks=None, top_down=False, palette_entries=None, gap=0, ppm=(0, 0), seed=0, body=None,
         planes=1):
    """-> the file as bytes.  masks: (r, g, b[, a]) for compression 3.  palette_entries: how many entries are written (default 2^bpp).
    body: the pixel bytes (h * row_stride) in FILE row order, random when None."""
    rng = np.random.default_rng(seed)
    masks = tuple(masks or (0, 0, 0, 0)) + (0,) * (4 - len(masks or (0, 0, 0, 0)))
    extra = b""
    if hsz == 12:
        dib = struct.pack("<IHHHH", 12, w & 0xffff, h & 0xffff, planes, bpp)
    else:
        dib = struct.pack("<IiiHHIIiiII", hsz, w, -h if top_down else h, planes, bpp, compression & 0xffffffff, 0, ppm[0], ppm[1], 0, 0)
        if hsz == 56:
            dib += struct.pack("<4I", *masks)
        elif hsz in (108, 124):
            dib += struct.pack("<4I", *masks) + b"BGRs" + bytes(48)
            if hsz == 124:
                dib += bytes(16)
        if hsz in (40, 56) and compression == 3:
            extra = struct.pack("<3I", *masks[:3])
        dib = dib.ljust(hsz, b"\0")
    pal = b""
    if bpp <= 8:
        n = (1 << bpp) if palette_entries is None else palette_entries
        pal = rng.integers(0, 256, n * (3 if hsz == 12 else 4), dtype=np.uint8).tobytes()
    gapb = rng.integers(0, 256, gap, dtype=np.uint8).tobytes()
    offset = 14 + len(dib) + len(extra) + len(pal) + gap
    if body is None:
        body = rng.integers(0, 256, h * row_stride(w, bpp), dtype=np.uint8).tobytes()
    body = bytes(body)
    size = offset + len(body)
    return b"BM" + struct.pack("<IHHI", size, 0, 0, offset) + dib + extra + pal + gapb + body


MASK_SETS_16 = [(0x7c00, 0x03e0, 0x001f, 0), (0xf800, 0x07e0, 0x001f, 0), (0x0f00, 0x00f0, 0x000f, 0xf000), (0x7c00, 0x03e0, 0x001f, 0x8000),
                (0x00c0, 0x0038, 0x0007, 0xff00)]
MASK_SETS_32 = [(0x00ff0000, 0x0000ff00, 0x000000ff, 0xff000000), (0x000000ff, 0x0000ff00, 0x00ff0000, 0xff000000), (0x3ff00000 >> 2, 0x000ff000 >> 4, 0x000000ff, 0),
                (0xff000000, 0x00ff0000, 0x0000ff00, 0x000000ff), (0x00fc0000, 0x0003f000, 0x00000f80, 0x0000007f), (0x00ff0000, 0x0000ff00, 0x000000ff, 0)]


def variants(w, h, seed=0):
    """every kind of file the loader tells apart, at one geometry: list of (name, bytes)"""
    out = []
    k = seed * 1000
    for hsz in HEADER_SIZES:
        for bpp in (1, 4, 8):
            for td in (False, True):
                if hsz == 12 and td:
                    continue
                out.append((f"h{hsz}_p{bpp}_{'td' if td else 'bu'}", make(w, h, bpp, hsz, top_down=td, seed=k))); k += 1
        out.append((f"h{hsz}_p8_short", make(w, h, 8, hsz, palette_entries=37 if hsz != 12 else 41, seed=k))); k += 1
        out.append((f"h{hsz}_p4_gap", make(w, h, 4, hsz, gap=2, seed=k))); k += 1
        out.append((f"h{hsz}_24", make(w, h, 24, hsz, seed=k))); k += 1
        if hsz == 12:
            continue
        out.append((f"h{hsz}_24_td_ppm", make(w, h, 24, hsz, top_down=True, ppm=(3780, 2835), seed=k))); k += 1
        out.append((f"h{hsz}_24_gap", make(w, h, 24, hsz, gap=8, seed=k))); k += 1
        out.append((f"h{hsz}_16_rgb", make(w, h, 16, hsz, seed=k))); k += 1
        out.append((f"h{hsz}_32_rgb", make(w, h, 32, hsz, top_down=(k & 1) == 1, seed=k))); k += 1
        for i, m in enumerate(MASK_SETS_16):
            out.append((f"h{hsz}_16_bf{i}", make(w, h, 16, hsz, 3, m, top_down=(i & 1) == 1, seed=k))); k += 1
        for i, m in enumerate(MASK_SETS_32):
            out.append((f"h{hsz}_32_bf{i}", make(w, h, 32, hsz, 3, m, top_down=(i & 1) == 0, ppm=(0, 2835), seed=k))); k += 1
    return out


def random_file(rng):
    """one random small file over every parameter of make()"""
    hsz = int(rng.choice(HEADER_SIZES)); bpp = int(rng.choice(DEPTHS))
    w, h = int(rng.integers(1, 40)), int(rng.integers(1, 7))
    comp, masks = 0, None
    if hsz != 12 and bpp in (16, 32) and rng.random() < 0.6:
        comp = 3
        masks = (MASK_SETS_16 if bpp == 16 else MASK_SETS_32)[int(rng.integers(0, 5))]
        if rng.random() < 0.3:                                    # arbitrary masks: contiguous runs of 1..8 bits anywhere
            masks = tuple((((1 << int(rng.integers(1, 9))) - 1) << int(rng.integers(0, bpp - 8))) & ((1 << bpp) - 1) for _ in range(4))
    entries = None
    if bpp <= 8 and rng.random() < 0.4:
        entries = int(rng.integers(1, (1 << bpp) + 1))
    return make(w, h, bpp, hsz, comp, masks, top_down=hsz != 12 and rng.random() < 0.5, palette_entries=entries,
                gap=int(rng.integers(0, 9)) if rng.random() < 0.3 else 0,
                ppm=(int(rng.choice([0, 1, 2, 2835, 3780, -5])), int(rng.choice([0, 1, 2835, 3780]))), seed=int(rng.integers(0, 1 << 30)))
