"""The corpus of tests/c/png_host_check.cpp: the PNG fixtures of tests/golden/ref_images as they are, and files from gen.write_png at 5x3 in every
colour type and depth -- with and without Adam7, with tRNS, with a palette -- each as written and re-chunked into 1-byte IDATs (the zlib header
then spans two chunks); the generated files are marked so that the check also runs every truncation of them.  Per file a little-endian u32 length,
a byte (1: truncate) and the bytes.

TEST INFRASTRUCTURE, used by test_png_host_cpu.py; by hand for the sanitizer build:    python tests/png_host_corpus.py corpus.bin"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIXTURES = ("issue65.png", "vst3-compatible.png", "issue76.png", "issue51cgbi.png", "issue51cgbi2.png")


def chunks(data):
    """(type, payload) of every chunk of a well-formed file"""
    at, out = 8, []
    while at < len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def idat_stream(data):
    return b"".join(d for t, d in chunks(data) if t == b"IDAT")


def with_idat(data, payloads):
    """the file with these IDAT chunks in the place of its own (none: the file has no IDAT)"""
    cs = chunks(data)
    first = next(i for i, (t, _) in enumerate(cs) if t == b"IDAT")
    return data[:8] + b"".join(_chunk(t, d) for t, d in cs[:first]) + b"".join(_chunk(b"IDAT", d) for d in payloads) + \
        b"".join(_chunk(t, d) for t, d in cs[first:] if t != b"IDAT")


def rechunk(data, size=1):
    """the same file with its IDAT payload cut into chunks of `size` bytes"""
    idat = idat_stream(data)
    return with_idat(data, [idat[i:i + size] for i in range(0, len(idat), size)])


def generated(w=5, h=3):
    import gen
    rng = np.random.default_rng(92)
    out = []
    for color, depths in [(0, (1, 2, 4, 8, 16)), (2, (8, 16)), (4, (8, 16)), (6, (8, 16)), (3, (1, 2, 4, 8))]:
        ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[color]
        for depth in depths:
            smp = rng.integers(0, 1 << depth, (h, w * ch))
            pal = rng.integers(0, 256, (1 << depth, 3)) if color == 3 else None
            for interlace in (0, 1):
                out.append(gen.write_png(smp, w, h, color, depth, interlace=interlace, palette=pal))
                if color in (0, 2):
                    key = [int(v) for v in smp[0, :ch]]
                    out.append(gen.write_png(smp, w, h, color, depth, interlace=interlace, trns=sum(([v >> 8, v & 255] for v in key), [])))
                if color == 3:
                    out.append(gen.write_png(smp, w, h, 3, depth, interlace=interlace, palette=pal, trns=list(rng.integers(0, 256, min(len(pal), 3)))))
                    out.append(gen.write_png(smp, w, h, 3, depth, interlace=interlace))          # no PLTE
    out.append(gen.write_png(rng.integers(0, 256, (h, w * 4)), w, h, 6, 8, iphone=True))
    out.append(gen.write_png(rng.integers(0, 256, (h, w * 4)), w, h, 6, 8, no_iend=True))
    return out


def corpus():
    """[(bytes, truncate)]"""
    files = [(open(os.path.join(HERE, "golden", "ref_images", n), "rb").read(), False) for n in FIXTURES]
    gen_files = generated()
    files += [(f, True) for f in gen_files] + [(rechunk(f), True) for f in gen_files]
    bad = bytearray(rechunk(gen_files[0]))                                                  # a zlib header that fails its check, across two chunks
    bad[bad.index(b"IDAT", bad.index(b"IDAT") + 4) + 4] = 0x79
    files += [(bytes(bad), False), (rechunk(gen_files[0], 0x7FFFFFFF)[:-12], False), (b"", False), (b"\x89PNG\r\n\x1a\n", False)]
    return files


def write(path):
    files = corpus()
    with open(path, "wb") as o:
        for f, truncate in files:
            o.write(struct.pack("<IB", len(f), int(truncate)) + f)
    return files


if __name__ == "__main__":
    print(len(write(sys.argv[1])), "files")
