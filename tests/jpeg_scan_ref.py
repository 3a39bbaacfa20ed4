"""A plain baseline JPEG decoder (ITU T.81, SOF0) for tests: marker walk, bit-by-bit Huffman code search with no look-up table (Annex F.2.2.3,
DECODE: one bit at a time against the canonical first code of every length), EXTEND, DC prediction, restart intervals, any sampling, one or
more scans.  It is the independent reading the hand-built scans of tests/jpeg_scan_cases.py are checked against, and it keeps a CENSUS of what
a stream contains, so that a case can prove what its name claims:

    lengths[(tc, th)]    code lengths used, per table               symbols[...]        symbols by kind (see Census)
    stuffed              FF 00 pairs in the scan                    stuffed_at          their offsets from the first scan byte
    segments             unstuffed length of every restart interval marker_at           offsets of the RSTn markers' first 0xFF
    sub_need(bits)       second-level entries a table needs under the rule of to_dev_huff_build
    phase_lock(...)      per lane boundary: does a decoder entered there in state (block 0, index 0) ever stand in the true state at a later one

Coefficients leave de-quantised, int16 (the product wraps), natural order, blocks in MCU order -- the dense form of the library.  Only streams
that T.81 defines are decoded: an unassigned bit pattern, a run past 63 or a DC category above 15 raise Undefined."""
import collections

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50,
          43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Undefined(Exception):
    pass


class Huff:
    """canonical code of a DHT table: mincode / count / first value index per length"""

    def __init__(self, bits, vals):
        self.bits = [0] + list(bits)                       # bits[1..16]
        self.vals = list(vals)
        self.mincode, self.first = [0] * 17, [0] * 17
        code = k = 0
        for ln in range(1, 17):
            self.mincode[ln], self.first[ln] = code, k
            code += self.bits[ln]; k += self.bits[ln]
            code <<= 1

    def codes(self):
        """[(code, length, symbol)] in table order"""
        out = []
        for ln in range(1, 17):
            for i in range(self.bits[ln]):
                out.append((self.mincode[ln] + i, ln, self.vals[self.first[ln] + i]))
        return out


def sub_need(bits):
    """entries of the second level a table with these counts (bits[0] = codes of length 1) needs: for every 9-bit prefix that only codes of more
    than 9 bits begin with, 2 ** (the longest such code's length - 9)"""
    longest = {}
    code = 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            if ln > 9:
                p = code >> (ln - 9)
                longest[p] = max(longest.get(p, 0), ln)
            code += 1
        code <<= 1
    return sum(1 << (ln - 9) for ln in longest.values())


def sub_fit(bits, capacity):
    """(prefixes that get a second level, prefixes left to the canonical search) when the levels are handed out in prefix order into `capacity` entries"""
    longest = {}
    code = 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            if ln > 9:
                p = code >> (ln - 9)
                longest[p] = max(longest.get(p, 0), ln)
            code += 1
        code <<= 1
    used, fit, left = 0, [], []
    for p in sorted(longest):
        n = 1 << (longest[p] - 9)
        if used + n > capacity:
            left.append(p)
        else:
            fit.append(p); used += n
    return fit, left


class Census:
    def __init__(self):
        self.lengths = collections.defaultdict(collections.Counter)      # (tc, th) -> {code length: count}
        self.prefixes = collections.defaultdict(collections.Counter)     # (tc, th) -> {9-bit prefix of a code longer than 9 bits: count}
        self.symbols = collections.Counter()                               # ("dc", cat) / ("ac", size) / "eob" / "zrl" / ("r0", run) / "full" (a block that ends at 63 without EOB)
        self.stuffed = 0
        self.stuffed_at = []
        self.marker_at = []
        self.fill = []                                                      # 0xFF fill bytes in front of every RSTn
        self.rst = []                                                       # the RSTn numbers met
        self.segments = []                                                  # unstuffed bytes per restart interval (every scan)
        self.dc_wraps = 0                                                   # times a DC predictor left the int16 range between two blocks
        self.zero_products = 0                                              # non-zero values whose de-quantised product is 0 in int16
        self.tables_defined = collections.Counter()                         # (tc, th) -> definitions met
        self.tables_used = set()
        self.dht_segments = []                                              # tables per DHT segment
        self.dqt_precision = {}
        self.scans = []                                                     # component indices per scan
        self.trace = []                                                     # per segment: (unstuffed bytes, {bit position: (block of the MCU, zig-zag index)}, nb, tables)


class Decoded:
    pass


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _i16(x):
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def decode(data, trace=False):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    cen = Census()
    quant, huff = {}, {}
    p = 2
    frame = None
    ri = 0
    out = Decoded(); out.census = cen
    coeffs = None
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        if m == 0xD9:
            break
        n = (data[p + 2] << 8) | data[p + 3]
        pl = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xDB:
            q = 0
            while q < len(pl):
                pq, tq = pl[q] >> 4, pl[q] & 15
                q += 1
                if pq:
                    quant[tq] = [(pl[q + 2 * i] << 8) | pl[q + 2 * i + 1] for i in range(64)]; q += 128
                else:
                    quant[tq] = list(pl[q:q + 64]); q += 64
                cen.dqt_precision[tq] = pq
        elif m == 0xC4:
            q = 0; here = 0
            while q < len(pl):
                tc, th = pl[q] >> 4, pl[q] & 15
                bits = list(pl[q + 1:q + 17]); nv = sum(bits)
                huff[(tc, th)] = Huff(bits, pl[q + 17:q + 17 + nv]); q += 17 + nv
                cen.tables_defined[(tc, th)] += 1; here += 1
            cen.dht_segments.append(here)
        elif m == 0xDD:
            ri = (pl[0] << 8) | pl[1]
        elif m == 0xC0:
            assert pl[0] == 8
            h, w, nc = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4], pl[5]
            comp = [dict(id=pl[6 + 3 * c], h=pl[7 + 3 * c] >> 4, v=pl[7 + 3 * c] & 15, tq=pl[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comp[0]["h"] = comp[0]["v"] = 1                                  # one component: never interleaved (A.2.2)
            hmax, vmax = max(c["h"] for c in comp), max(c["v"] for c in comp)
            mpr, mpc = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            off, nb = [], 0
            for c in comp:
                off.append(nb); nb += c["h"] * c["v"]
            frame = dict(w=w, h=h, comp=comp, hmax=hmax, vmax=vmax, mpr=mpr, mpc=mpc, nb=nb, off=off)
            coeffs = np.zeros((mpr * mpc * nb, 64), np.int16)
        elif m == 0xDA:
            ns = pl[0]
            sel = []
            for k in range(ns):
                cid, t = pl[1 + 2 * k], pl[2 + 2 * k]
                ci = [c["id"] for c in frame["comp"]].index(cid)
                sel.append((ci, t >> 4, t & 15))
            assert pl[1 + 2 * ns:1 + 2 * ns + 3] == bytes([0, 63, 0])
            cen.scans.append([s[0] for s in sel])
            p = _scan(data, p, frame, sel, quant, huff, ri, coeffs, cen, trace)
    out.width, out.height = frame["w"], frame["h"]
    out.frame = frame
    out.coeffs = coeffs
    out.huff, out.quant = huff, quant
    return out


def _scan(data, p, fr, sel, quant, huff, ri, coeffs, cen, trace):
    """the entropy-coded data from data[p] on; -> position of the marker that ends it"""
    comp = fr["comp"]
    if len(sel) == 1:                                                       # non-interleaved: the component's own blocks, raster order
        ci = sel[0][0]; c = comp[ci]
        nbx = -(-(-(-fr["w"] * c["h"] // fr["hmax"])) // 8); nby = -(-(-(-fr["h"] * c["v"] // fr["vmax"])) // 8)
        units = nbx * nby

        def blocks_of(u):
            by, bx = divmod(u, nbx)
            mcu = (by // c["v"]) * fr["mpr"] + bx // c["h"]
            return [(0, mcu * fr["nb"] + fr["off"][ci] + (by % c["v"]) * c["h"] + bx % c["h"])]
    else:
        units = fr["mpr"] * fr["mpc"]
        order = [(slot, fr["off"][ci] + b) for slot, (ci, _, _) in enumerate(sel) for b in range(comp[ci]["h"] * comp[ci]["v"])]

        def blocks_of(u):
            return [(slot, u * fr["nb"] + o) for slot, o in order]
    nb_scan = len(blocks_of(0))
    # cut at the markers, unstuff
    start = p
    segs, seg = [], bytearray()
    while True:
        b = data[p]
        if b != 0xFF:
            seg.append(b); p += 1; continue
        if data[p + 1] == 0x00:
            seg.append(0xFF); cen.stuffed += 1; cen.stuffed_at.append(p - start); p += 2; continue
        q = p + 1
        while data[q] == 0xFF:
            q += 1
        if 0xD0 <= data[q] <= 0xD7:
            cen.marker_at.append(p - start); cen.fill.append(q - p - 1); cen.rst.append(data[q] - 0xD0)
            segs.append(bytes(seg)); seg = bytearray(); p = q + 1; continue
        p = q - 1
        break
    segs.append(bytes(seg))
    n_int = -(-units // ri) if ri else 1
    assert len(segs) == n_int, (len(segs), n_int)
    assert cen.rst[len(cen.rst) - (n_int - 1):] == [k & 7 for k in range(n_int - 1)]
    qz = [quant[comp[ci]["tq"]] for ci, _, _ in sel]
    tabs = [(huff[(0, td)], huff[(1, ta)], td, ta) for _, td, ta in sel]
    for _, td, ta in sel:
        cen.tables_used.add((0, td)); cen.tables_used.add((1, ta))
    u = 0
    for si, sg in enumerate(segs):
        cen.segments.append(len(sg))
        nbits = len(sg) * 8
        pos = 0
        states = {} if trace else None

        def bit():
            nonlocal pos
            if pos >= nbits:
                raise Undefined("the segment ends inside a symbol")
            v = (sg[pos >> 3] >> (7 - (pos & 7))) & 1
            pos += 1
            return v

        def sym(h, key):
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | bit()
                k = code - h.mincode[ln]
                if 0 <= k < h.bits[ln]:
                    cen.lengths[key][ln] += 1
                    if ln > 9:
                        cen.prefixes[key][code >> (ln - 9)] += 1
                    return h.vals[h.first[ln] + k]
            raise Undefined("no code word")

        def value(s):
            v = 0
            for _ in range(s):
                v = (v << 1) | bit()
            return _extend(v, s)

        pred = [0] * len(sel)
        last = min(units, u + ri) if ri else units
        while u < last:
            for bi, (slot, blk) in enumerate(blocks_of(u)):
                hd, ha, td, ta = tabs[slot]
                if trace:
                    states[pos] = (bi, 0)
                s = sym(hd, (0, td))
                if s > 15:
                    raise Undefined("DC category above 15")
                cen.symbols[("dc", s)] += 1
                before = pred[slot]
                pred[slot] += value(s)
                if ((before + 0x8000) >> 16) != ((pred[slot] + 0x8000) >> 16):
                    cen.dc_wraps += 1
                prod = _i16(pred[slot] * qz[slot][0])
                if pred[slot] and not prod:
                    cen.zero_products += 1
                coeffs[blk, 0] = prod
                k = 1
                while k < 64:
                    if trace:
                        states[pos] = (bi, k)
                    rs = sym(ha, (1, ta))
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r == 15:
                            if k + 16 > 64:
                                raise Undefined("ZRL past the block")
                            cen.symbols["zrl"] += 1
                            k += 16; continue
                        if r:
                            raise Undefined("r/0")
                        cen.symbols["eob"] += 1
                        break
                    k += r
                    if k > 63:
                        raise Undefined("run past 63")
                    cen.symbols[("ac", s)] += 1
                    v = value(s)
                    prod = _i16(v * qz[slot][k])
                    if not prod:
                        cen.zero_products += 1
                    coeffs[blk, ZIGZAG[k]] = prod
                    k += 1
                else:
                    cen.symbols["full"] += 1
            u += 1
        if trace:
            states[pos] = (0, 0)
            cen.trace.append((sg, states, nb_scan, [(t[0], t[1]) for t in tabs], [b[0] for b in blocks_of(0)]))
    return p


def header(data):
    """the marker walk alone, up to the first SOS: -> ({(class, id): Huff}, raw bytes from the first scan byte to the end of the file) -- for files
    whose scan decode() does not read"""
    huff, p = {}, 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        pl = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xC4:
            q = 0
            while q < len(pl):
                bits = list(pl[q + 1:q + 17]); nv = sum(bits)
                huff[(pl[q] >> 4, pl[q] & 15)] = Huff(bits, pl[q + 17:q + 17 + nv]); q += 17 + nv
        if m == 0xDA:
            return huff, len(data) - p


def phase_lock(trace_entry, lane_bytes):
    """for every lane boundary t * lane_bytes (t >= 1) inside the segment: True when a decoder entered at that bit in state (block 0, index 0)
    stands, at some LATER lane boundary, exactly where the true decoder stands (same bit, block of the MCU and zig-zag index when it is the
    first to reach or pass the boundary) -- from there on the two are one.  A stream error on the way counts as never.  -> {t: bool}"""
    sg, states, nb, tabs, slots = trace_entry
    nbits = len(sg) * 8
    step = lane_bytes * 8
    padded = sg + b"\xff" * 8
    # the true decoder's crossing state of every boundary
    order = sorted(states)
    truth = {}
    j = 0
    for t in range(1, (nbits + step - 1) // step):
        while order[j] < t * step:
            j += 1
        truth[t] = (order[j],) + states[order[j]]
    memo = {}

    def one(pos, c, z):
        """one symbol -> (pos, c, z) or None"""
        hd, ha = tabs[slots[c]]
        h = hd if z == 0 else ha
        w = int.from_bytes(padded[pos >> 3:(pos >> 3) + 5], "big") >> (24 - (pos & 7)) & 0xFFFF
        for ln in range(1, 17):
            code = w >> (16 - ln)
            k = code - h.mincode[ln]
            if 0 <= k < h.bits[ln]:
                s = h.vals[h.first[ln] + k]
                break
        else:
            return None
        if z == 0:
            if s > 15:
                return None
            return pos + ln + s, c, 1
        r, s = s >> 4, s & 15
        if s == 0:
            if r == 15:
                return (pos + ln, c, z + 16) if z + 16 < 64 else ((pos + ln, (c + 1) % nb, 0) if z + 16 == 64 else None)
            return pos + ln, (c + 1) % nb, 0
        if z + r > 63:
            return None
        z += r + 1
        return (pos + ln + s, c, z) if z < 64 else (pos + ln + s, (c + 1) % nb, 0)

    res = {}
    for t in sorted(truth):
        st = (t * step, 0, 0)
        path = []
        verdict = None
        nxt = t + 1
        while verdict is None:
            if st in memo:
                verdict = memo[st]; break
            path.append(st)
            new = one(*st)
            if new is None or new[0] >= nbits:
                verdict = False; break
            while nxt in truth and new[0] >= nxt * step:
                if truth[nxt] == new:
                    verdict = True
                nxt += 1
            st = new
        for s in path:
            memo[s] = verdict
        res[t] = verdict
    return res
