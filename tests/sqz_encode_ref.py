"""SQZ_encode read a second time, in Python, from the D text (source/gamut/codecs/sqz.d) and not from tests/c/sqz_ref.c.  The scan orders,
the schedule table, SQZ_mirror and SQZ_ilog2 are the ones tests/sqz_ref.py already read from the same text for the decoder.

  analyze(px, mode, levels)       (h, w[, 3]) uint8 -> planes * h * w sign-magnitude int16 (SQZ_color_process read = 1, SQZ_dwt, :1574-1582)
  dwt(planes, w, h, levels)       two's-complement int16 planes in raster order -> the same, without the colour stage
  encode(px, mode, levels, ...)   -> the file as bytes;  encode_coeffs(co, w, h, ...) the writer alone

numpy carries whole rows or columns where that changes nothing: the horizontal pass keeps the reference's loop over i and its running
cf0..cf3 (a vector over the ROWS of a level, every row sees exactly the reference's arithmetic, the scratch row with evens and odds
back to back included); the vertical walk keeps the reference's loop over row pairs and its pointer guards (a vector over the
columns).  The one liberty: the walk is made twice, first doing only the horizontal passes, then only the vertical steps.  That is the
same thing if no vertical step touches a row before the row's horizontal pass in the reference's order; the walk records the order
and asserts it for every height it is given."""
import math

import numpy as np

import sqz_ref as D                                                         # scans, schedule, mirror, ilog2: read from the D text

GREY, YCOCG, OKLAB, LOGL1 = range(4)
PLANES = (1, 3, 3, 3)


class Undefined(Exception):
    """the reference shifts 1u by 32 here"""


def clamp_levels(w, h, levels):
    """SQZ_validate_input, read_only = 0"""
    return min(levels, min(D.ilog2(min(w, h)) - 3, 8))


# ---- colour, :1153-1515 with read = 1 ----
def srgb_to_linear():
    t = [int(math.floor(65535.0 * ((i / 255.0) / 12.92 if i / 255.0 <= 0.04045 else ((i / 255.0 + 0.055) / 1.055) ** 2.4) + 0.5)) for i in range(256)]
    assert (t[0], t[1], t[12], t[128], t[254], t[255]) == (0x0000, 0x0014, 0x00F1, 0x3742, 0xFDB8, 0xFFFF)      # entries of :1251-1285
    return np.array(t, np.int64)


def cbrt_01(v):
    """SQZ_i32_cbrt_01 :1368-1385 on an int64 array; the clamps come first, the rest runs on harmless values there"""
    v = np.asarray(v, np.int64)
    w = np.clip(v, 1, 65534)
    root = ((w * (((w * (w - 144107)) >> 16) + 132114)) >> 16) + 14379
    for _ in range(2):
        n = root * root * root
        den = w + (n >> 31)
        num = root * (2 * w + (n >> 32))
        assert (num >= 0).all() and (den > 0).all()                        # so flooring is the reference's truncating division
        root = num // den
    root = root.astype(np.int32).astype(np.int64)                           # cast(int)
    return np.where(v <= 0, 0, np.where(v >= 65535, 65535, root))


def colour(px, mode):
    """-> (planes, h, w) int16"""
    px = np.asarray(px, np.uint8)
    s16 = lambda a: np.asarray(a, np.int64).astype(np.int16)
    if mode == GREY:
        return s16(px.astype(np.int64) - 128)[None]
    R, G, B = (px[..., c].astype(np.int64) for c in range(3))
    if mode == YCOCG:
        t = s16((R + B) >> 1).astype(np.int64)
        return np.stack([s16(((t + G) >> 1) - 128), s16(R - B), s16(G - t)])
    if mode == OKLAB:
        lut = srgb_to_linear()
        r, g, b = lut[R], lut[G], lut[B]
        i32 = lambda a: a.astype(np.int32).astype(np.int64)
        l = cbrt_01(i32((27015 * r + 35149 * g + 3372 * b) >> 16))
        m = cbrt_01(i32((13887 * r + 44610 * g + 7038 * b) >> 16))
        s = cbrt_01(i32((5787 * r + 18462 * g + 41286 * b) >> 16))
        return np.stack([s16(((862 * l + 3250 * m - 17 * s + 32767) >> 16) - 2048),
                         s16((8100 * l - 9945 * m + 1845 * s + 32767) >> 16),
                         s16((106 * l + 3205 * m - 3311 * s + 32767) >> 16)])
    i32 = lambda a: a.astype(np.int32).astype(np.int64)                     # LOG-L1 computes in int
    return np.stack([s16(i32((33779 * R + 41184 * G + 38182 * B) >> 16) - 221),
                     s16(i32(-52830 * R + 8188 * G + 37906 * B) >> 16),
                     s16(i32(19051 * R - 50317 * G + 37420 * B) >> 16)])


# ---- SQZ_dwt_5_3i_horizontal_pass :1597-1643, on the rows of `block` (rows, width) int16, in place ----
def horizontal_pass(block):
    rows, width = block.shape
    if width < 4:
        return
    s16 = lambda a: np.asarray(a, np.int64).astype(np.int16)
    half_w = width >> 1
    stride = half_w
    w = half_w - 1
    odd_w = width & 1
    if odd_w:
        stride += 1
    scratch = np.zeros((rows, width + 1), np.int16)                         # evens = scratch, odds = scratch + stride
    ev = lambda i: scratch[:, i].astype(np.int64)
    od = lambda i: scratch[:, stride + i].astype(np.int64)
    scratch[:, :half_w] = block[:, 0:2 * half_w:2]
    scratch[:, stride:stride + half_w] = block[:, 1:2 * half_w:2]
    if odd_w:
        scratch[:, half_w] = block[:, 2 * half_w]
    h_band = block[:, stride:]
    l_band = block
    cf0, cf2 = ev(0), ev(1)
    cf1 = s16(od(0) + ((-(cf0 + cf2)) >> 1)).astype(np.int64)               # h_band[0] = cf1 = cast(short)(...)
    h_band[:, 0] = s16(cf1)
    cf0 = cf0 + ((cf1 + 1) >> 1)
    l_band[:, 0] = s16(cf0)
    i = 1
    while i < w:
        cf3 = od(i)
        cf0 = ev(i + 1)
        cf3 = cf3 + ((-(cf2 + cf0)) >> 1)
        h_band[:, i] = s16(cf3)
        cf2 = cf2 + ((cf1 + cf3 + 2) >> 2)
        l_band[:, i] = s16(cf2)
        i += 1
        cf1 = od(i)
        cf2 = ev(i + 1)                                                     # (i = w on the last turn when w is even: evens[w + 1] is odds[0] for an even width)
        cf1 = cf1 + ((-(cf2 + cf0)) >> 1)
        h_band[:, i] = s16(cf1)
        cf0 = cf0 + ((cf1 + cf3 + 2) >> 2)
        l_band[:, i] = s16(cf0)
        i += 1
    cf3 = od(w) + (((-(ev(w) + ev(w + 1))) >> 1) if odd_w else -ev(w))
    h_band[:, w] = s16(cf3)
    l_band[:, w] = s16(ev(w) + ((h_band[:, w - 1].astype(np.int64) + cf3 + 2) >> 2))
    if odd_w:
        l_band[:, w + 1] = s16(ev(w + 1) + ((cf3 + 1) >> 1))


# ---- SQZ_dwt_5_3i :1645-1673 on `a` (height, width) int16, in place; row numbers stand for the reference's row pointers ----
def level_5_3(a):
    height, width = a.shape
    mx = height - 1
    passed = {}                                                             # row -> the step of the walk at which it was passed
    for do_vertical in (False, True):
        step = 0
        nnn, nn = D.mirror(-3, mx), D.mirror(-2, mx)
        i = -2
        while i < height:
            n, r = D.mirror(i + 1, mx), D.mirror(i + 2, mx)
            if nn <= r:
                step += 1
                if not do_vertical:
                    assert n not in passed
                    passed[n] = step
            if i + 2 < height:
                step += 1
                if not do_vertical:
                    assert r not in passed
                    passed[r] = step
            if nn <= r:
                step += 1
                if do_vertical:
                    assert max(passed[n], passed[nn], passed[r]) < step
                    a[n] = (a[n].astype(np.int64) - ((a[nn].astype(np.int64) + a[r].astype(np.int64)) >> 1)).astype(np.int16)
            if nnn <= n:
                step += 1
                if do_vertical:
                    assert max(passed[nn], passed[nnn], passed[n]) < step
                    a[nn] = (a[nn].astype(np.int64) + ((a[nnn].astype(np.int64) + a[n].astype(np.int64) + 2) >> 2)).astype(np.int16)
            nnn, nn = n, r
            i += 2
        if not do_vertical:
            assert sorted(passed) == list(range(height))
            horizontal_pass(a)


def dwt(planes, w, h, levels):
    """two's-complement planes (any shape holding planes * h * w int16) -> sign-magnitude coefficients, flat"""
    d = np.array(planes, np.int16).reshape(-1, h, w)
    for p in range(d.shape[0]):
        lw, lh = w, h
        for level in range(levels):                                         # SQZ_dwt :1686-1694: stride << level
            view = d[p, ::1 << level, :][:lh, :lw]
            level_5_3(view)
            lw, lh = (lw + 1) >> 1, (lh + 1) >> 1
    v = d.astype(np.int64)
    return np.where(v < 0, (-2 * v) | 1, 2 * v).astype(np.int16).reshape(-1)        # :1580


def analyze(px, mode, levels):
    px = np.asarray(px, np.uint8)
    h, w = px.shape[:2]
    return dwt(colour(px, mode), w, h, levels)


# ---- the bit buffer's write side :570-623: a bit list cut at the capacity ----
class Writer:
    def __init__(self, budget):
        self.cap, self.chunks, self.pos = budget * 8, [], 0

    def eob(self):
        return self.pos >= self.cap

    def bits(self, v, width):
        """SQZ_bit_buffer_write_bits: what fits is written, MSB first; 0 as soon as the buffer is found full at the top of the loop"""
        if self.eob():
            return 0
        take = min(width, self.cap - self.pos)
        if take:
            self.chunks.append(np.array([(v >> (width - 1 - k)) & 1 for k in range(take)], np.uint8))
        self.pos += take
        return int(take == width)

    def bit(self, b):
        return self.bits(b & 1, 1)

    def many(self, bits):
        """write_bit after write_bit until one fails"""
        take = min(len(bits), max(self.cap - self.pos, 0))
        self.chunks.append(np.asarray(bits[:take], np.uint8))
        self.pos += take

    def file(self):
        allbits = np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.uint8)
        return np.packbits(allbits).tobytes()[:(self.pos + 7) // 8]


def interleave(i):
    """SQZ_interleave_u16_to_u32 :548-556"""
    v = 0
    for k in range(16):
        v |= ((i >> k) & 1) << (2 * k)
    return v


def write_run(out, run):
    """SQZ_encode_write_wdr_run :1928-1939"""
    cost = D.ilog2(run) - 1
    if cost <= 16:
        return out.bits(interleave(run), cost * 2)
    return out.bits(interleave(run >> 16), (cost - 16) * 2) and out.bits(interleave(run), 32)


class Band:
    pass


def encode_coeffs(co, w, h, mode, levels, scan, subsampling, budget):
    """SQZ_encode :2208-2240 behind the DWT.  levels is clamped here.  None when the header does not fit (SQZ_BUFFER_TOO_SMALL)."""
    levels = clamp_levels(w, h, levels)
    planes = PLANES[mode]
    data = np.asarray(co, np.int16).reshape(-1)
    assert data.size == planes * w * h
    out = Writer(budget)
    for v, n in ((0xA5, 8), (w - 1, 16), (h - 1, 16), (mode, 2), (levels - 1, 3), (scan, 2)):     # SQZ_encode_header :1901-1911
        out.bits(v, n)
    out.bit(int(bool(subsampling)))
    if out.eob():
        return None
    bands = {}
    for p in range(planes):                                                 # SQZ_common_init_context :1805-1827
        bw, bh = w, h
        for level in range(levels - 1, -1, -1):
            for o in range(1 if level > 0 else 0, 4):
                b = Band()
                b.base = p * w * h
                b.w, b.h = (bw + (0 if o & 1 else 1)) >> 1, (bh + (0 if o > 1 else 1)) >> 1
                b.round = D.schedule(mode, p, level, o) + (int(bool(subsampling)) & int(p > 0))
                b.stride = w << (levels - level)
                if o & 1:
                    b.base += (bw + 1) >> 1
                if o > 1:
                    b.base += b.stride >> 1
                b.bitplane = b.max_bitplane = 0
                bands[p, level, o] = b
            bw, bh = (bw + 1) >> 1, (bh + 1) >> 1
    idle = Band()
    idle.round = idle.bitplane = 0

    def task(b, first):
        if first:                                                           # SQZ_encode_init_subband :1866-1876
            xy = np.array(D.SCANS[scan](b.w, b.h), np.int64)
            b.lip = b.base + xy[:, 1] * b.stride + xy[:, 0]
            b.lsp = np.zeros(0, np.int64)
            mx = int(data[b.lip].max())                                     # SQZ_dwt_get_max compares shorts
            shifted = (mx >> 1) & 0xFFFFFFFF                                # the short's >> 1 is an int, SQZ_ilog2 takes a uint
            b.max_bitplane = b.bitplane = D.ilog2(shifted)
            out.bits(b.max_bitplane, 4)
        nsp = np.zeros(0, np.int64)
        if len(b.lip) and b.bitplane > 0:                                   # SQZ_encode_sorting_pass :1953-1986
            if b.bitplane >= 32:
                raise Undefined
            mask = np.int16(1 << b.bitplane)                                # a maximum that is not negative gives a bit plane of 14 at most
            v = data[b.lip]
            sig = (v & mask) != 0
            last, broke, taken = 0, False, 0
            for k in np.nonzero(sig)[0]:
                i = int(k) + 1
                if not out.bits(2 | (int(v[k]) & 1), 1 + int(last != 0)) or not write_run(out, i - last):
                    broke = True
                    break
                last = i
                taken += 1
            i = (int(np.nonzero(sig)[0][taken]) + 1) if broke else len(b.lip) + 1
            out.bits(3, 1 + int(taken > 0))
            write_run(out, i - last)
            out.bit(1)
            nsp = b.lip[sig]
            b.lip = b.lip[~sig]
            if out.eob():
                return False
        mask = np.int16(1 << b.bitplane)                                    # SQZ_encode_refinement_pass :2022-2037
        out.many(((data[b.lsp] & mask) != 0).astype(np.uint8))
        if out.eob():
            return False
        b.lsp = np.concatenate([b.lsp, nsp])                                # SQZ_list_merge
        b.bitplane -= b.bitplane > 0
        return not out.eob()

    state = plane = level = o = 0                                           # SQZ_schedule_task :2105-2168
    rnd, done, stop = 0, False, False
    while not done and not out.eob() and not stop:
        done = True
        while True:
            b = bands.get((plane, level, o), idle)
            if rnd < b.round or (rnd > b.round and b.bitplane == 0):
                done = done and rnd > b.round
            else:
                if not task(b, b.round == rnd):
                    stop = True
                    break
                done = done and b.bitplane == 0
            if not state:
                o += 1
                if o >= 4:
                    level += 1
                    o = int(level < levels)
                    if o == 0:
                        level = 0
                        state = plane = int(planes > 1)
                        if not state:
                            break
            else:
                plane += 1
                if plane >= planes:
                    plane = 1
                    o += 1
                    if o >= 4:
                        level += 1
                        o = int(level < levels)
                        if o == 0:
                            level = 0
                            state = plane = 0
                            break
        rnd += 1
    return out.file()


def encode(px, mode, levels, scan=1, subsampling=0, budget=None):
    px = np.asarray(px, np.uint8)
    h, w = px.shape[:2]
    levels = clamp_levels(w, h, levels)
    if budget is None:
        budget = 64 + px.size * 3
    return encode_coeffs(analyze(px, mode, levels), w, h, mode, levels, scan, subsampling, budget)
