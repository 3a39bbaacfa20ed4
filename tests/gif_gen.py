"""A GIF writer for the tests with every knob the decoder can see: screen and frame rectangles, interlace, lzw_cs, GCT / LCT sizes, the
GCE's fields or its absence, sub-block sizes, where clear codes go (deferred clear included), end code present or absent, raw code lists.

The LZW side is split in two: compress() turns symbols into a list of codes, pack() writes a list of codes with the code sizes the
DECODER will have when it reads them (it follows the decoder's `avail` and code-size rule, codecs/gif.d:685-754), so that any code
list -- a legal one or not -- can be written."""
import numpy as np

END = "end"
CLEAR = "clear"


class _DecoderState:
    """the part of parseImageData's state that decides how wide the next code is"""

    def __init__(self, cs):
        self.cs = cs
        self.clear = 1 << cs
        self.reset()

    def reset(self):
        self.codesize = self.cs + 1
        self.avail = self.clear + 2
        self.old = False

    def data(self):
        if self.old:
            self.avail += 1
        if (self.avail & ((1 << self.codesize) - 1)) == 0 and self.avail <= 0x0FFF:
            self.codesize += 1
        self.old = True


def pack(codes, cs):
    """codes: ints, CLEAR or END -> the bit stream as bytes"""
    st = _DecoderState(cs)
    acc = nbits = 0
    out = bytearray()
    for c in codes:
        v = st.clear if c == CLEAR else st.clear + 1 if c == END else int(c)
        acc |= (v & ((1 << st.codesize) - 1)) << nbits
        nbits += st.codesize
        while nbits >= 8:
            out.append(acc & 255); acc >>= 8; nbits -= 8
        if v == st.clear:
            st.reset()
        elif v != st.clear + 1:
            st.data()
    if nbits:
        out.append(acc & 255)
    return bytes(out)


def compress(symbols, cs, start_clears=1, end=True, clear_when="full", clears_at=None):
    """symbols (each < 1 << cs; the decoder emits symbol & 255) -> code list.
    clear_when: the decoder's `avail` at which a clear code is written ("full": 4096, or 8192 for lzw_cs 12; None: never -- deferred
    clear, the table stays as it is and `avail` keeps counting).  clears_at: {symbol position: number of clear codes written there}."""
    clears_at = clears_at or {}
    maxcode = 8191 if cs == 12 else 4095
    if clear_when == "full":
        clear_when = maxcode + 1
    st = _DecoderState(cs)
    table = {}
    codes = [CLEAR] * start_clears
    n, i = len(symbols), 0
    sym = [int(s) for s in symbols]
    while i < n:
        if i in clears_at:
            codes += [CLEAR] * clears_at[i]
            st.reset(); table.clear()
        w, j = sym[i], i + 1
        while j < n and j not in clears_at and table.get((w, sym[j]), 1 << 30) < (1 << st.codesize):   # (lzw_cs 0: the code size lags behind `avail`)
            w = table[(w, sym[j])]; j += 1
        codes.append(w)
        st.data()
        if j < n and j not in clears_at and st.avail <= maxcode:
            table[(w, sym[j])] = st.avail
        if clear_when is not None and st.avail >= clear_when and j < n:
            codes.append(CLEAR)
            st.reset(); table.clear()
        i = j
    if end:
        codes.append(END)
    return codes


def subblocks(data, size=255, terminator=True):
    out = bytearray()
    for p in range(0, len(data), size):
        chunk = data[p:p + size]
        out.append(len(chunk)); out += chunk
    if terminator:
        out.append(0)
    return bytes(out)


def table_bytes(colors):
    """colors: (n, 3) uint8, n a power of two from 2 to 256 -> (size field, bytes)"""
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    n = colors.shape[0]
    assert n in (2, 4, 8, 16, 32, 64, 128, 256)
    return n.bit_length() - 2, colors.tobytes()


def gce(disposal=0, transparent=None, delay=0, size=4, terminator=0, user_input=0):
    flag = (disposal & 7) << 2 | (user_input & 1) << 1 | (0 if transparent is None else 1)
    return bytes([0x21, 0xF9, size, flag]) + int(delay).to_bytes(2, "little") + bytes([0 if transparent is None else transparent, terminator])


def comment(text=b"hello"):
    return b"\x21\xFE" + subblocks(text)


def app_ext(loops=0):
    return b"\x21\xFF\x0bNETSCAPE2.0" + subblocks(b"\x01" + int(loops).to_bytes(2, "little"))


def plain_text():
    return b"\x21\x01\x0c" + bytes(12) + subblocks(b"text")


def frame(x, y, w, h, symbols=None, cs=8, interlace=False, lct=None, gce_bytes=b"", pre=b"", block=255, payload=None, codes=None,
          terminator=True, after_end=b"", **lzw):
    """one image: extensions in front (`pre`, then the GCE), descriptor, LCT, lzw_cs and the sub-block chain.
    payload: the packed LZW bytes given directly; codes: a code list for pack(); otherwise symbols for compress()."""
    if payload is None:
        if codes is None:
            codes = compress(symbols, cs, **lzw)
        payload = pack(codes, cs)
    flags = 0x40 if interlace else 0
    lct_b = b""
    if lct is not None:
        sz, lct_b = table_bytes(lct)
        flags |= 0x80 | sz
    desc = b"\x2C" + b"".join(int(v).to_bytes(2, "little") for v in (x, y, w, h)) + bytes([flags])
    return {"pre": pre, "gce": gce_bytes, "desc": desc, "lct": lct_b, "cs": bytes([cs]), "data": subblocks(payload + after_end, block, terminator)}


def build(sw, sh, frames, gct=None, version=b"GIF89a", bg=0, aspect=0, trailer=True, tail=b""):
    """-> (file bytes, spans): spans is a list of (kind, start, end) with kind in "gce", "desc", "data" """
    flags = 0x70
    gct_b = b""
    if gct is not None:
        sz, gct_b = table_bytes(gct)
        flags |= 0x80 | sz
    out = bytearray(version + int(sw).to_bytes(2, "little") + int(sh).to_bytes(2, "little") + bytes([flags, bg, aspect]) + gct_b)
    spans = []
    for f in frames:
        out += f["pre"]
        if f["gce"]:
            spans.append(("gce", len(out), len(out) + len(f["gce"])))
        out += f["gce"]
        spans.append(("desc", len(out), len(out) + len(f["desc"])))
        out += f["desc"] + f["lct"] + f["cs"]
        spans.append(("data", len(out), len(out) + len(f["data"])))
        out += f["data"]
    out += tail
    if trailer:
        out += b"\x3B"
    return bytes(out), spans


def make(sw, sh, frames, **kw):
    return build(sw, sh, frames, **kw)[0]


def palette(n, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (n, 3), dtype=np.uint8)


def noise(rng, n, levels=256):
    return rng.integers(0, levels, n)


def photo_like(rng, w, h, levels=256):
    """smooth gradients plus a little noise: short strings, a table that fills"""
    yy, xx = np.mgrid[0:h, 0:w]
    v = (np.sin(xx / 17.0) + np.cos(yy / 11.0) + 2) / 4 * (levels - 1) + rng.normal(0, 2.0, (h, w))
    return np.clip(v, 0, levels - 1).astype(np.int64).reshape(-1)


def flat(w, h, levels=4, band=16):
    """bands of one colour: long strings"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // band) + (xx // (band * 4))) % levels).astype(np.int64).reshape(-1)


def small_valid(rng):
    """a small valid file of 1-3 frames for the mutation tests -> (bytes, spans)"""
    sw, sh = int(rng.integers(4, 24)), int(rng.integers(4, 20))
    bits = int(rng.integers(1, 5))
    frames = []
    for k in range(int(rng.integers(1, 4))):
        fw, fh = int(rng.integers(1, sw + 1)), int(rng.integers(1, sh + 1))
        fx, fy = int(rng.integers(0, sw - fw + 1)), int(rng.integers(0, sh - fh + 1))
        sym = noise(rng, fw * fh, 1 << bits) if rng.random() < 0.6 else flat(fw, fh, 1 << min(bits, 2), 2)
        g = gce(int(rng.integers(0, 4)), int(rng.integers(0, 1 << bits)) if rng.random() < 0.4 else None, int(rng.integers(0, 12))) if rng.random() < 0.75 else b""
        lct = palette(1 << bits, k) if rng.random() < 0.3 else None
        frames.append(frame(fx, fy, fw, fh, sym, cs=max(bits, 2), interlace=rng.random() < 0.3, lct=lct, gce_bytes=g,
                            block=int(rng.choice([255, 7, 40]))))
    return build(sw, sh, frames, gct=palette(1 << bits, 99))


def mutate(data, spans, rng):
    """1-3 bytes changed inside one GCE, one descriptor or one LZW payload, by rules under which the reference alone accepts and
    refuses more than a tenth of the files each: most changes flip low bits (a frame moves or shrinks, a code changes), some set a
    whole byte (a bad separator, a block length that runs past the file, a frame that leaves the screen)."""
    kind, a, b = spans[int(rng.integers(0, len(spans)))]
    out = bytearray(data)
    for _ in range(int(rng.integers(1, 4))):
        p = int(rng.integers(a, b))
        if rng.random() < 0.5:
            out[p] ^= 1 << int(rng.integers(0, 3))
        else:
            out[p] = int(rng.integers(0, 256))
    return bytes(out)
