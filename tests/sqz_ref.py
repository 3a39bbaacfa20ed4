"""SQZ_decode read a second time, in Python, from the D text (source/gamut/codecs/sqz.d) and not from tests/c/sqz_ref.c: plain lists where
the reference links nodes, a recursive generator for the Hilbert curve where it keeps a stack, arbitrary-precision integers wrapped by
hand where it computes in short / int / long.  Slow: for small frames only.  decode() -> None when the file is refused, else
(info dict, coefficients after SQZ_decode_round_coefficients as a list, pixels as bytes)."""
import math

PLANES = (1, 3, 3, 3)


def s16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def s32(v):
    v &= 0xFFFFFFFF
    return v - 0x100000000 if v & 0x80000000 else v


class Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data), 0                                   # pos counts bits

    def eob(self):
        return self.pos >> 3 >= len(self.d)

    def bit(self):
        if self.eob():
            return -1
        b = (self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, width):
        """SQZ_bit_buffer_read_bits: -1 as soon as a byte is missing, even with some bits already taken"""
        v = 0
        while True:
            if self.eob():
                return -1
            avail = 8 - (self.pos & 7)
            take = min(avail, width)
            v = (v << take) | ((self.d[self.pos >> 3] >> (avail - take)) & ((1 << take) - 1))
            self.pos += take
            width -= take
            if width == 0:
                return v


def ilog2(x):
    return x.bit_length()


def mirror(v, maximum):
    if maximum == 0:
        return 0
    while v < 0 or v > maximum:                                             # cast(uint)value > cast(uint)maximum
        v = -v
        if v < 0:
            v += 2 * maximum
    return v


# ---- scan orders ----
def scan_raster(w, h):
    return [(x, y) for y in range(h) for x in range(w)]


def scan_snake(width, height, tw=4, th=15):
    tw, th = min(tw, width), min(th, height)
    step = 1
    while True:
        grid_w = (width + tw - 1) // tw
        if grid_w & 1:
            break
        tw += step
        if tw > width or tw < 0:
            tw = width
        elif tw == 0:
            tw = 1
        step = -(abs(step) + 1) * ((step > 0) - (step < 0))
    cols_rem = width % tw or tw
    step = 2
    while True:
        rows_rem = height % th
        if rows_rem > 0 and not rows_rem & 1:
            th += step
            if th > height or th < 0:
                th = height
            elif th == 0:
                th = 1
            step = -(abs(step) + 2) * ((step > 0) - (step < 0))
        else:
            rows_rem = rows_rem or th
            break
    grid_h = (height + th - 1) // th
    # the state of SQZ_scan_snake, stepped as the reference steps it
    s = dict(tx=0, ty=0, tw=tw, th=th, r2l=0, gx=0, gy=0, ci=0, codd=0, rodd=0, ox=0, oy=0)
    out = [(0, 0)]
    while True:
        s["tx"] += 1
        where = "columns"
        if s["tx"] >= s["tw"]:
            s["tx"] = 0
            s["ty"] += 1
            where = "rows"
            if s["ty"] >= s["th"]:
                s["ty"] = 0
                s["ci"] += 1
                where = "grid"
                if s["ci"] >= grid_w:
                    s["ci"] = 0
                    s["gy"] += 1
                    if s["gy"] >= grid_h:
                        return out
                    s["rodd"] = s["gy"] & 1
                    s["th"] = th if s["gy"] < grid_h - 1 else rows_rem
                    s["oy"] = s["gy"] * th
        if where == "grid":
            last = grid_w - 1
            s["gx"] = last - s["ci"] if s["rodd"] else s["ci"]
            s["codd"] = s["gx"] & 1
            s["tw"] = tw if s["gx"] < last else cols_rem
            s["ox"] = s["gx"] * tw
            where = "rows"
        if where == "rows":
            row = s["th"] - 1 - s["ty"] if s["codd"] else s["ty"]
            s["r2l"] = (s["gy"] ^ row) & 1
        x = (s["tw"] - 1 - s["tx"] if s["r2l"] else s["tx"]) + s["ox"]
        y = (s["th"] - 1 - s["ty"] if s["codd"] else s["ty"]) + s["oy"]
        out.append((x, y))


def _even_bits(i):
    v = 0
    for k in range(16):
        v |= ((i >> (2 * k)) & 1) << k
    return v


def scan_morton(w, h):
    rng = ilog2(min(w, h) - 1)
    mask = (1 << (2 * rng)) - 1
    length = 1 << (rng + ilog2(max(w, h) - 1))
    out, index = [(0, 0)], 0
    while True:
        found = False
        while True:
            index += 1
            x, y = _even_bits(index & mask), _even_bits((index >> 1) & mask)
            m = (index & ~mask) >> rng
            if w > h:
                x |= m
            else:
                y |= m
            if x < w and y < h:
                found = True
                break
            if not index < length:
                break
        if not found:
            return out
        out.append((x, y))


def _tdiv(a):
    return int(a / 2)                                                       # D's integer division truncates towards zero


def _gilbert(x, y, ax, ay, bx, by):
    w, h = abs(ax + ay), abs(bx + by)
    sg = lambda v: (v > 0) - (v < 0)
    dax, day, dbx, dby = sg(ax), sg(ay), sg(bx), sg(by)
    if h == 1:
        for _ in range(w):
            yield x, y
            x, y = x + dax, y + day
        return
    if w == 1:
        for _ in range(h):
            yield x, y
            x, y = x + dbx, y + dby
        return
    ax2, ay2, bx2, by2 = _tdiv(ax), _tdiv(ay), _tdiv(bx), _tdiv(by)
    w2, h2 = abs(ax2 + ay2), abs(bx2 + by2)
    if 2 * w > 3 * h:
        if w2 % 2 and w > 2:
            ax2, ay2 = ax2 + dax, ay2 + day
        yield from _gilbert(x, y, ax2, ay2, bx, by)
        yield from _gilbert(x + ax2, y + ay2, ax - ax2, ay - ay2, bx, by)
    else:
        if h2 % 2 and h > 2:
            bx2, by2 = bx2 + dbx, by2 + dby
        yield from _gilbert(x, y, bx2, by2, ax2, ay2)
        yield from _gilbert(x + bx2, y + by2, ax, ay, bx - bx2, by - by2)
        yield from _gilbert(x + (ax - dax) + (bx2 - dbx), y + (ay - day) + (by2 - dby), -bx2, -by2, -(ax - ax2), -(ay - ay2))


def scan_hilbert(w, h):
    return list(_gilbert(0, 0, w, 0, 0, h) if w >= h else _gilbert(0, 0, 0, h, w, 0))


SCANS = (scan_raster, scan_snake, scan_morton, scan_hilbert)


def schedule(mode, plane, level, o):
    """SQZ_schedule[mode][plane][level][o], read off the table"""
    luma = [[0, l + 1, l + 1, l + 2] for l in range(8)]
    chroma = [[1, 2, 2, 3]] + [[0, l + 2, l + 2, l + 3] for l in range(1, 8)]
    if plane == 0:
        return luma[level][o]
    return 0 if mode == 0 else chroma[level][o]


class Band:
    def __init__(self):
        self.lip, self.lsp, self.nsp = [], [], []
        self.max_bitplane = self.bitplane = self.round = 0
        self.base = self.w = self.h = self.stride = 0


def parse_header(data):
    b = Bits(data)
    if b.bits(8) != 0xA5:
        return None
    w, h, mode, lv, scan, ss = b.bits(16) + 1, b.bits(16) + 1, b.bits(2), b.bits(3) + 1, b.bits(2), b.bit()
    if b.eob():
        return None
    if not (8 <= w <= 65535 and 8 <= h <= 65535):
        return None
    if lv > min(ilog2(min(w, h)) - 3, 8):
        return None
    return dict(width=w, height=h, planes=PLANES[mode], color_mode=mode, levels=lv, scan_order=scan, subsampling=int(bool(ss)),
                pixel_type=0 if mode == 0 else 9, detected=1), b


def decode_coeffs(data):
    hd = parse_header(data)
    if hd is None:
        return None
    info, b = hd
    W, H, L, mode, planes = info["width"], info["height"], info["levels"], info["color_mode"], info["planes"]
    data16 = [0] * (W * H * planes)
    bands = {}
    for p in range(planes):
        w, h = W, H
        for level in range(L - 1, -1, -1):
            for o in range(1 if level > 0 else 0, 4):
                bd = Band()
                bd.base = p * W * H
                bd.w, bd.h = (w + (0 if o & 1 else 1)) >> 1, (h + (0 if o > 1 else 1)) >> 1
                bd.round = schedule(mode, p, level, o) + (info["subsampling"] & int(p > 0))
                bd.stride = W << (L - level)
                if o & 1:
                    bd.base += (w + 1) >> 1
                if o > 1:
                    bd.base += bd.stride >> 1
                bands[p, level, o] = bd
            w, h = (w + 1) >> 1, (h + 1) >> 1
    idle = Band()

    def at(bd, xy):
        return bd.base + xy[1] * bd.stride + xy[0]

    def read_run():
        run = 1
        while b.bit() == 0:
            v = b.bit()
            if v < 0:
                return None
            run = (run + run + v) & 0xFFFFFFFF
        return run

    def sorting(bd):
        if not bd.lip or bd.bitplane <= 0:
            return True
        mask = 1 << bd.bitplane
        k = 0                                                               # index into the LIP: the reference's `pixel`
        while True:
            sign = b.bit()
            if sign < 0:
                break
            run = read_run()
            if run is None:
                break
            while True:
                run = (run - 1) & 0xFFFFFFFF
                if not (run > 0 and k < len(bd.lip)):
                    break
                k += 1
            if k >= len(bd.lip):
                break
            i = at(bd, bd.lip[k])
            data16[i] = s16(data16[i] | mask | sign)
            bd.nsp.append(bd.lip.pop(k))                                    # exchange: out of the LIP, to the NSP's tail; k is now the next entry
        return not b.eob()

    def refinement(bd):
        mask = 1 << (bd.bitplane & 31)
        for xy in bd.lsp:
            v = b.bit()
            if v > 0:
                i = at(bd, xy)
                data16[i] = s16(data16[i] | mask)
            elif v < 0:
                break
        return not b.eob()

    def task(bd, first):
        if first:
            bd.lip = list(SCANS[info["scan_order"]](bd.w, bd.h))
            bd.max_bitplane = bd.bitplane = b.bits(4)
        if not sorting(bd) or not refinement(bd):
            return False
        bd.lsp += bd.nsp
        bd.nsp = []
        bd.bitplane -= bd.bitplane > 0
        return not b.eob()

    state = plane = level = o = 0
    rnd, done, stop = 0, False, False
    while not done and not b.eob() and not stop:
        done = True
        while True:
            bd = bands.get((plane, level, o), idle)
            if rnd < bd.round or (rnd > bd.round and bd.bitplane == 0):
                done = done and rnd > bd.round
            else:
                if not task(bd, bd.round == rnd):
                    stop = True
                    break
                done = done and bd.bitplane == 0
            if not state:
                o += 1
                if o >= 4:
                    level += 1
                    o = int(level < L)
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
                        o = int(level < L)
                        if o == 0:
                            level = 0
                            state = plane = 0
                            break
        rnd += 1
    for bd in bands.values():                                               # SQZ_decode_round_coefficients
        if bd.max_bitplane == 0 or bd.bitplane < 2:
            continue
        rm = ((1 << bd.bitplane) - 1) ^ 1
        for xy in bd.lsp:
            i = at(bd, xy)
            data16[i] = s16(data16[i] | rm)
    return info, data16


# ---- pixels ----
def idwt_row(d, base, width):
    if width < 4:
        return
    half = width >> 1
    odd = width & 1
    stride = half + odd
    w = half - 1
    L = lambda i: d[base + i]
    Hb = lambda i: d[base + stride + i]
    evens, odds = [0] * (half + 1), [0] * half
    cf1 = Hb(0)
    cf0 = L(0) - ((cf1 + 1) >> 1)
    evens[0] = s16(cf0)
    i = 1
    cf2 = cf3 = 0
    while i < w:
        cf2, cf3 = L(i), Hb(i)
        cf2 -= (cf1 + cf3 + 2) >> 2
        evens[i] = s16(cf2)
        odds[i - 1] = s16(cf1 - ((-(cf0 + cf2)) >> 1))
        i += 1
        cf0, cf1 = L(i), Hb(i)
        cf0 -= (cf1 + cf3 + 2) >> 2
        evens[i] = s16(cf0)
        odds[i - 1] = s16(cf3 - ((-(cf0 + cf2)) >> 1))
        i += 1
    evens[w] = s16(L(w) - ((Hb(w - 1) + Hb(w) + 2) >> 2))
    odds[w - 1] = s16(Hb(w - 1) - ((-(evens[w - 1] + evens[w])) >> 1))
    if odd:
        evens[w + 1] = s16(L(w + 1) - ((Hb(w) + 1) >> 1))
    odds[w] = s16(Hb(w) - (((-(evens[w] + evens[w + 1])) >> 1) if odd else -evens[w]))
    for i in range(half):
        d[base + 2 * i], d[base + 2 * i + 1] = evens[i], odds[i]
    if odd:
        d[base + 2 * half] = evens[half]


def idwt_level(d, base, width, height, stride):
    mx = height - 1
    nn, n = mirror(-2, mx), mirror(-1, mx)                                  # row numbers stand for the reference's row pointers
    i = -1
    while i <= height:
        r, s = mirror(i + 1, mx), mirror(i + 2, mx)
        if n <= s:
            for k in range(width):
                d[base + r * stride + k] = s16(d[base + r * stride + k] - ((d[base + n * stride + k] + d[base + s * stride + k] + 2) >> 2))
        if nn <= r:
            for k in range(width):
                d[base + n * stride + k] = s16(d[base + n * stride + k] + ((d[base + nn * stride + k] + d[base + r * stride + k]) >> 1))
        if i - 1 >= 0:
            idwt_row(d, base + nn * stride, width)
        if nn <= r:
            idwt_row(d, base + n * stride, width)
        nn, n = r, s
        i += 2


def srgb_table():
    return [int(math.floor(255.0 * (12.92 * (i / 511.0) if i / 511.0 <= 0.0031308 else 1.055 * (i / 511.0) ** (1.0 / 2.4) - 0.055) + 0.5)) for i in range(512)]


def clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def pixels(info, coeffs):
    W, H, L, mode, planes = info["width"], info["height"], info["levels"], info["color_mode"], info["planes"]
    d = [-(v >> 1) if v & 1 else v >> 1 for v in coeffs]
    for p in range(planes):
        for level in range(L - 1, -1, -1):
            w, h = W, H
            for _ in range(level):
                w, h = (w + 1) >> 1, (h + 1) >> 1
            idwt_level(d, p * W * H, w, h, W << level)
    n = W * H
    t = srgb_table()

    def lin(v):
        v = s32(v)
        if v <= 0:
            return 0
        if v >= 65535:
            return 255
        vm = v * 511
        off, frac = vm >> 16, vm & 65535
        return (t[off] + ((frac * (t[off + 1] - t[off])) >> 16)) & 0xFF

    out = bytearray(n * planes)
    for i in range(n):
        if mode == 0:
            out[i] = clip(s16(d[i] + 128))
        elif mode == 1:
            Y, Co, Cg = s16(d[i] + 128), d[n + i], d[2 * n + i]
            B = s16(Y + ((1 - Cg) >> 1) - (Co >> 1))
            G = s16(Y - ((-Cg) >> 1))
            R = s16(Co + B)
            out[3 * i:3 * i + 3] = bytes((clip(R), clip(G), clip(B)))
        elif mode == 2:
            Lv, a, b = s16(d[i] + 2048), d[n + i], d[2 * n + i]
            l_ = Lv * 16 + ((25974 * a + 14143 * b) >> 12)
            m_ = Lv * 16 + ((-6918 * a - 4185 * b) >> 12)
            s_ = Lv * 16 + ((-5864 * a - 84638 * b) >> 12)
            l, m, s = (l_ ** 3) >> 32, (m_ ** 3) >> 32, (s_ ** 3) >> 32
            out[3 * i:3 * i + 3] = bytes((lin((267169 * l - 216771 * m + 15137 * s) >> 16), lin((-83127 * l + 171030 * m - 22368 * s) >> 16),
                                          lin((-275 * l - 46099 * m + 111909 * s) >> 16)))
        else:
            Y, c0, c1 = s16(d[i] + 221), d[n + i], d[2 * n + i]
            R = s16((33779 * Y - 52830 * c0 + 19051 * c1) >> 16)
            G = s16((41184 * Y + 8188 * c0 - 50317 * c1) >> 16)
            B = s16((38182 * Y + 37906 * c0 + 37420 * c1) >> 16)
            out[3 * i:3 * i + 3] = bytes((clip(R), clip(G), clip(B)))
    return bytes(out)


def decode(data):
    r = decode_coeffs(data)
    if r is None:
        return None
    info, co = r
    return info, co, pixels(info, co)
