"""TGA files for the tests: every variant TGADecoder reads (types 1 / 2 / 3 / 9 / 10 / 11, 8 / 15 / 16 / 24 / 32 bits, colour maps of
8 / 15 / 16 / 24 / 32-bit entries under 8- or 16-bit indices), with knobs for the ID length, the colour map's start and length, the
descriptor bits, the packet policy of the run-length forms and a seed.  The writer is the test suite's own; nothing is decoded here."""
import numpy as np

POLICIES = ("mixed", "max", "one", "raw", "run")


def source_bytes(image_type, bpp, cmap_size=0):
    """bytes per pixel as stored in the file"""
    if image_type in (1, 9):
        return bpp // 8
    return 2 if bpp in (15, 16) else bpp // 8


def packets(policy, npix, rng, overrun=False):
    """[(is_run, count)] covering npix pixels; with overrun the last packet is not trimmed to the pixel count"""
    out, done = [], 0
    while done < npix:
        if policy == "max":
            run, cnt = bool(len(out) & 1), 128
        elif policy == "one":
            run, cnt = bool(rng.integers(0, 2)), 1
        elif policy == "raw":
            run, cnt = False, int(rng.integers(1, 129))
        elif policy == "run":
            run, cnt = True, int(rng.integers(1, 129))
        else:
            run, cnt = bool(rng.integers(0, 2)), int(rng.choice([1, 2, 3, 7, 31, 64, 127, 128, int(rng.integers(1, 129))]))
        if not overrun:
            cnt = min(cnt, npix - done)
        out.append((run, cnt)); done += cnt
    return out


def rle_stream(pkts, bps, rng, pixel=None):
    """the packet bytes; pixel(rng) -> bps bytes of one source pixel"""
    pixel = pixel or (lambda r: r.integers(0, 256, bps, dtype=np.uint8).tobytes())
    parts = []
    for run, cnt in pkts:
        parts.append(bytes([(0x80 if run else 0) | (cnt - 1)]))
        parts.append(pixel(rng) if run else b"".join(pixel(rng) for _ in range(cnt)))
    return b"".join(parts)


def header(w, h, image_type, bpp, cmap_size=0, pal_start=0, pal_len=0, id_len=0, top_down=False, desc_extra=0, cmap_type=None):
    cmap_type = (1 if image_type in (1, 9) else 0) if cmap_type is None else cmap_type
    desc = (0x20 if top_down else 0) | desc_extra
    return (bytes([id_len, cmap_type, image_type]) + pal_start.to_bytes(2, "little") + pal_len.to_bytes(2, "little") + bytes([cmap_size]) +
            bytes(4) + w.to_bytes(2, "little") + h.to_bytes(2, "little") + bytes([bpp, desc]))


def make(w, h, image_type, bpp, cmap_size=0, pal_len=None, pal_start=0, id_len=0, top_down=False, desc_extra=0, policy="mixed", seed=0,
         overrun=False, bad_index=False, trailer=b"", pkts=None):
    """a whole file.  Indexed types: pal_len entries (default 256 for 8-bit indices, 300 for 16-bit ones) behind pal_start filler BYTES;
    indices below pal_len unless bad_index.  Run-length types: packets by `policy` (or the explicit list pkts), free to cross row ends."""
    rng = np.random.default_rng([seed, w, h, image_type, bpp, cmap_size])
    indexed = image_type in (1, 9)
    bps = source_bytes(image_type, bpp, cmap_size)
    if indexed and pal_len is None:
        pal_len = 256 if bpp == 8 else 300
    f = header(w, h, image_type, bpp, cmap_size, pal_start, pal_len or 0, id_len, top_down, desc_extra)
    f += rng.integers(0, 256, id_len, dtype=np.uint8).tobytes()
    if indexed:
        esz = 2 if cmap_size in (15, 16) else cmap_size // 8
        f += rng.integers(0, 256, pal_start, dtype=np.uint8).tobytes() + rng.integers(0, 256, pal_len * esz, dtype=np.uint8).tobytes()
        top = min(1 << bpp, pal_len + 40) if bad_index else min(1 << bpp, pal_len)
        pixel = lambda r: int(r.integers(0, top)).to_bytes(bps, "little")
    else:
        pixel = None
    npix = w * h
    if image_type >= 8:
        f += rle_stream(pkts if pkts is not None else packets(policy, npix, rng, overrun), bps, rng, pixel)
    elif pixel:
        f += b"".join(pixel(rng) for _ in range(npix))
    else:
        f += rng.integers(0, 256, npix * bps, dtype=np.uint8).tobytes()
    return f + trailer


def variants():
    """(name, image_type, bpp, cmap_size) of every pixel variant the decoder distinguishes, unpacked and run-length"""
    out = []
    for rle in (0, 8):
        for bpp in (8, 15, 16, 24, 32):
            out.append((f"t{2 + rle}_b{bpp}", 2 + rle, bpp, 0))
        for bpp in (8, 15, 16, 24):
            out.append((f"t{3 + rle}_b{bpp}", 3 + rle, bpp, 0))
        for cmap in (8, 15, 16, 24, 32):
            for idx in (8, 16):
                out.append((f"t{1 + rle}_i{idx}_c{cmap}", 1 + rle, idx, cmap))
    return out
