"""A plain progressive JPEG decoder (ITU T.81 Annex G, SOF2) for tests, the counterpart of tests/jpeg_scan_ref.py: marker walk (DHT / DQT / DRI
anywhere between the scans), bit-by-bit Huffman code search (jpeg_scan_ref.Huff, no look-up table), Python ints, the four scan kinds as G.1.2 /
G.2 state them -- DC first, DC refinement, AC first with EOB runs, AC refinement with correction bits -- restart intervals, any of the five
sampling modes, interleaved DC scans and non-interleaved scans of any component.  It is the independent reading the hand-built scans of
tests/jpeg_prog_cases.py are checked against, and it keeps a CENSUS per scan so that a case can prove what its name claims (ScanCensus).

Where T.81 defines no result it raises Undefined: a code word no table holds, a DC category above 15, a run or ZRL that leaves the band, a
refinement symbol of size 2 and more, a run that finds fewer positions without history than it asks for, an EOB run that reaches past its
restart interval or scan, a correction bit for a coefficient whose bit plane is already set, a segment that ends inside a symbol.
decode(data, habits=True) does what the REFERENCE does in those places instead (jpegload.d:3296-3518: a run may end anywhere up to 63, a
refinement run that runs out sets position Se + 1, an EOB run is dropped at RSTn and at the end of the scan, a set bit plane is left alone,
ones follow the data) and notes each in ScanCensus.habits -- the census of the cases that rest on a habit.  What the reference refuses (a run
past 63, size >= 2) is Undefined either way.

Coefficients are kept the way the reference keeps them: int16, a stored value wraps (value << Al; the predictor is not clipped).  They leave
de-quantised (int16 products), natural order, blocks in MCU order -- the dense form of the library -- with max_zag = the last zig-zag position
that is not 0, plus one."""
import collections

import numpy as np

from jpeg_scan_ref import ZIGZAG, Huff, Undefined

DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE = range(4)
KIND = ["dc_first", "dc_refine", "ac_first", "ac_refine"]


class ScanCensus:
    def __init__(self, kind, comps, ss, se, ah, al, ri, units):
        self.kind, self.comps, self.ss, self.se, self.ah, self.al, self.ri, self.units = kind, comps, ss, se, ah, al, ri, units
        self.symbols = collections.Counter()      # ("dc", cat) / ("ac", size) / "zrl" / ("eob", n) / ("new", run)
        self.lengths = collections.Counter()      # code length -> count
        self.max_eobrun = 0                       # blocks the longest EOB run covers (the block of the symbol included)
        self.eob_starts = []                      # (unit the EOBn symbol was read in, n, extra bits, blocks covered)
        self.eob_units = set()                    # units decoded while an EOB run is in force (the symbol's own block included)
        self.free_skips = set()                   # ... of an AC refinement scan without history in the band: not a bit of the stream
        self.corr_only = set()                    # ... with history: correction bits only
        self.corr_bits = []                       # (unit, symbol, correction bits behind it); symbol None: the bits of a block inside an EOB run
        self.history = {}                         # unit -> zig-zag positions of the band that were not 0 when the scan reached the block (AC refinement)
        self.starved = []                         # (unit, symbol, position the walk stopped at): no position without history was left
        self.sign_at, self.corr_at = [], []       # (segment, bit position in the unstuffed segment)
        self.code_at = []                         # (segment, bit position, code length, symbol)
        self.block_span = {}                      # unit -> (segment, first bit, bit behind the last)
        self.left_int16 = 0                       # values that did not fit int16 when stored
        self.plane_set = 0                        # correction bits 1 for a coefficient whose bit `Al` was set already
        self.past_band = []                       # (unit, position): a coefficient stored behind Se
        self.habits = []                          # what the reference made of a place T.81 does not define
        self.segments, self.seg_bits = [], []     # unstuffed bytes / bits used, per restart interval
        self.stuffed = []                         # per segment: unstuffed offsets of the 0xFF bytes that carried a 0x00
        self.fill, self.surplus = [], []          # 0xFF fill bytes in front of each RSTn; whole bytes between an interval's last bit and its marker
        self.past_end = 0                         # bits read behind the data


class Decoded:
    pass


def _i16(x):
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def header_blocks(data):
    """8 x 8 blocks of the frame's largest component, from the SOF2 alone"""
    at = bytes(data).index(b"\xff\xc2")
    return -(-((data[at + 5] << 8) | data[at + 6]) // 8) * -(-((data[at + 7] << 8) | data[at + 8]) // 8)


def decode(data, habits=False):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    quant, huff = {}, {}
    ri, p, frame, zz = 0, 2, None, None
    out = Decoded(); out.scans = []; out.dht_between = 0; out.dqt_between = 0; out.dri_values = []
    while True:
        if p + 1 >= len(data):
            raise Undefined("the file ends without EOI")
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
            out.dqt_between += bool(out.scans)
        elif m == 0xC4:
            q = 0
            while q < len(pl):
                bits = list(pl[q + 1:q + 17]); nv = sum(bits)
                huff[(pl[q] >> 4, pl[q] & 15)] = Huff(bits, pl[q + 17:q + 17 + nv]); q += 17 + nv
            out.dht_between += bool(out.scans)
        elif m == 0xDD:
            ri = (pl[0] << 8) | pl[1]
            out.dri_values.append(ri)
        elif m == 0xC2:
            assert pl[0] == 8
            h, w, nc = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4], pl[5]
            comp = [dict(id=pl[6 + 3 * c], h=pl[7 + 3 * c] >> 4, v=pl[7 + 3 * c] & 15, tq=pl[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comp[0]["h"] = comp[0]["v"] = 1
            hmax, vmax = max(c["h"] for c in comp), max(c["v"] for c in comp)
            mpr, mpc = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            off, nb = [], 0
            for c in comp:
                off.append(nb); nb += c["h"] * c["v"]
            frame = dict(w=w, h=h, comp=comp, hmax=hmax, vmax=vmax, mpr=mpr, mpc=mpc, nb=nb, off=off)
            zz = np.zeros((mpr * mpc * nb, 64), np.int16)                       # zig-zag order, not de-quantised
        elif m == 0xDA:
            ns = pl[0]
            sel = []
            for k in range(ns):
                ci = [c["id"] for c in frame["comp"]].index(pl[1 + 2 * k])
                sel.append((ci, pl[2 + 2 * k] >> 4, pl[2 + 2 * k] & 15))
            ss, se, ah, al = pl[1 + 2 * ns], pl[2 + 2 * ns], pl[3 + 2 * ns] >> 4, pl[3 + 2 * ns] & 15
            p = _scan(data, p, frame, sel, ss, se, ah, al, huff, ri, zz, out, habits)
    out.width, out.height, out.frame = frame["w"], frame["h"], frame
    co = np.zeros_like(zz)
    per = [frame["comp"][c]["tq"] for c in range(len(frame["comp"])) for _ in range(frame["comp"][c]["h"] * frame["comp"][c]["v"])]
    for b in range(frame["nb"]):
        q = np.array(quant[per[b]], np.int64)
        co[b::frame["nb"], ZIGZAG] = (zz[b::frame["nb"]].astype(np.int64) * q).astype(np.int16)      # the product wraps
    out.coeffs = co
    last = np.zeros(len(zz), int)
    for z in range(63, 0, -1):
        hit = (zz[:, z] != 0) & (last == 0)
        last[hit] = z
    out.max_zag = (last + 1).astype(np.uint8)
    out.quantised = zz
    return out


def _scan(data, p, fr, sel, ss, se, ah, al, huff, ri, zz, out, habits):
    comp = fr["comp"]
    assert ss <= se <= 63 and (ss or not se) and (ss == 0 or len(sel) == 1) and (not ah or al == ah - 1)
    kind = (DC_REFINE if ah else DC_FIRST) if ss == 0 else (AC_REFINE if ah else AC_FIRST)
    if len(sel) == 1:
        ci = sel[0][0]; c = comp[ci]
        nbx = -(-(-(-fr["w"] * c["h"] // fr["hmax"])) // 8); nby = -(-(-(-fr["h"] * c["v"] // fr["vmax"])) // 8)
        units = nbx * nby

        def blocks_of(u):
            by, bx = divmod(u, nbx)
            return [(0, ((by // c["v"]) * fr["mpr"] + bx // c["h"]) * fr["nb"] + fr["off"][ci] + (by % c["v"]) * c["h"] + bx % c["h"])]
    else:
        units = fr["mpr"] * fr["mpc"]
        order = [(slot, fr["off"][ci] + b) for slot, (ci, _, _) in enumerate(sel) for b in range(comp[ci]["h"] * comp[ci]["v"])]

        def blocks_of(u):
            return [(slot, u * fr["nb"] + o) for slot, o in order]
    cen = ScanCensus(kind, [s[0] for s in sel], ss, se, ah, al, ri, units)
    out.scans.append(cen)
    # cut at the markers, unstuff
    segs, seg, stuffed, rst = [], bytearray(), [], []
    while True:
        if p >= len(data):
            raise Undefined("the file ends inside a scan")
        b = data[p]
        if b != 0xFF:
            seg.append(b); p += 1; continue
        if p + 1 >= len(data):
            raise Undefined("the file ends inside a scan")
        if data[p + 1] == 0x00:
            stuffed.append(len(seg)); seg.append(0xFF); p += 2; continue
        q = p + 1
        while q < len(data) and data[q] == 0xFF:
            q += 1
        if q < len(data) and 0xD0 <= data[q] <= 0xD7:
            cen.fill.append(q - p - 1); rst.append(data[q] - 0xD0)
            segs.append(bytes(seg)); cen.stuffed.append(stuffed); seg, stuffed = bytearray(), []; p = q + 1; continue
        p = q - 1
        break
    segs.append(bytes(seg)); cen.stuffed.append(stuffed)
    n_int = -(-units // ri) if ri else 1
    if len(segs) != n_int or rst != [k & 7 for k in range(n_int - 1)]:
        raise Undefined("the restart markers do not fit the scan")
    p1, m1 = 1 << al, -1 << al
    u = 0
    for si, sg in enumerate(segs):
        nbits, pos = len(sg) * 8, 0

        def bit():
            nonlocal pos
            if pos >= nbits:
                if not habits:
                    raise Undefined("the segment ends inside a symbol")
                cen.past_end += 1; pos += 1
                return 1
            v = (sg[pos >> 3] >> (7 - (pos & 7))) & 1
            pos += 1
            return v

        def bits(n):
            v = 0
            for _ in range(n):
                v = (v << 1) | bit()
            return v

        def sym(h):
            at, code = pos, 0
            for ln in range(1, 17):
                code = (code << 1) | bit()
                k = code - h.mincode[ln]
                if 0 <= k < h.bits[ln]:
                    s = h.vals[h.first[ln] + k]
                    cen.lengths[ln] += 1; cen.code_at.append((si, at, ln, s))
                    return s
            raise Undefined("no code word")

        def store(row, k, v):
            if not -32768 <= v <= 32767:
                cen.left_int16 += 1
            row[k] = _i16(v)

        def correct(row, k):
            cen.corr_at.append((si, pos))
            if bit():
                v = int(row[k])
                if v & p1:
                    if not habits:
                        raise Undefined("the bit plane is already set")
                    cen.plane_set += 1
                else:
                    store(row, k, v + (p1 if v >= 0 else m1))

        pred = [0] * len(sel)
        eobrun = 0
        last = min(units, u + ri) if ri else units
        while u < last:
            first_bit = pos
            for slot, blk in blocks_of(u):
                row = zz[blk]
                if kind == DC_FIRST:
                    s = sym(huff[(0, sel[slot][1])])
                    if s > 15:
                        raise Undefined("DC category above 15")
                    cen.symbols[("dc", s)] += 1
                    if s:
                        cen.sign_at.append((si, pos))
                    pred[slot] += _extend(bits(s), s)
                    store(row, 0, pred[slot] << al)
                elif kind == DC_REFINE:
                    cen.corr_at.append((si, pos))
                    if bit():
                        row[0] = _i16(int(row[0]) | p1)
                elif kind == AC_FIRST:
                    if eobrun:
                        eobrun -= 1; cen.eob_units.add(u); continue
                    h = huff[(1, sel[slot][2])]
                    k = ss
                    while k <= se:
                        rs = sym(h)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise Undefined("run past 63")
                            if k > se:
                                if not habits:
                                    raise Undefined("run past Se")
                                cen.habits.append(("run past Se", u, k)); cen.past_band.append((u, k))
                            cen.symbols[("ac", s)] += 1
                            cen.sign_at.append((si, pos))
                            store(row, k, _extend(bits(s), s) << al)
                            k += 1
                        elif r == 15:
                            k += 15
                            if k > 63:
                                raise Undefined("ZRL past the block")
                            if k > se:
                                if not habits:
                                    raise Undefined("ZRL past Se")
                                cen.habits.append(("ZRL past Se", u, k))
                            cen.symbols["zrl"] += 1
                            k += 1
                        else:
                            extra = bits(r)
                            eobrun = (1 << r) + extra
                            cen.symbols[("eob", r)] += 1; cen.eob_starts.append((u, r, extra, eobrun))
                            cen.max_eobrun = max(cen.max_eobrun, eobrun)
                            eobrun -= 1; cen.eob_units.add(u)
                            break
                else:
                    h = huff[(1, sel[slot][2])]
                    hist = [k for k in range(ss, se + 1) if row[k]]
                    cen.history[u] = hist
                    k = ss
                    if eobrun == 0:
                        while k <= se:
                            rs = sym(h)
                            r, s = rs >> 4, rs & 15
                            val = 0
                            if s:
                                if s != 1:
                                    raise Undefined("size >= 2 in a refinement scan")
                                cen.sign_at.append((si, pos))
                                val = p1 if bit() else m1
                                cen.symbols[("new", r)] += 1
                            elif r != 15:
                                extra = bits(r)
                                eobrun = (1 << r) + extra
                                cen.symbols[("eob", r)] += 1; cen.eob_starts.append((u, r, extra, eobrun))
                                cen.max_eobrun = max(cen.max_eobrun, eobrun)
                                break
                            else:
                                cen.symbols["zrl"] += 1
                            passed = 0
                            while k <= se:
                                if row[k]:
                                    correct(row, k); passed += 1
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            cen.corr_bits.append((u, rs, passed))
                            if k > se:                                         # no position without history left for the run
                                if not habits:
                                    raise Undefined("the run finds no position without history")
                                cen.starved.append((u, rs, k)); cen.habits.append(("starved run", u, k))
                                if val and k < 64:
                                    row[k] = val; cen.past_band.append((u, k))
                            elif val:
                                row[k] = val
                            k += 1
                    if eobrun > 0:
                        passed = 0
                        for k in range(k, se + 1):
                            if row[k]:
                                correct(row, k); passed += 1
                        cen.eob_units.add(u)
                        (cen.corr_only if hist else cen.free_skips).add(u)
                        if passed:
                            cen.corr_bits.append((u, None, passed))
                        eobrun -= 1
            cen.block_span[u] = (si, first_bit, pos)
            u += 1
        if eobrun:
            if not habits:
                raise Undefined("the EOB run reaches past its interval")
            cen.habits.append(("EOB run dropped", u, eobrun))
        cen.segments.append(len(sg)); cen.seg_bits.append(pos)
        cen.surplus.append(max(0, len(sg) - -(-pos // 8)))
        if cen.surplus[-1]:
            if not habits:
                raise Undefined("octets between the interval's last bit and the marker")
            # process_restart (jpegload.d:2335-2402) looks for the marker from where the reference's input stands -- its bit reader fetches two octets
            # at a time, four at a (re)start --, through at most 1536 octets up to a 0xFF, which has to be the marker's (a stuffed one is not)
            rest = sg[4 + 2 * (pos // 16):]
            if si < len(segs) - 1 and (0xFF in rest or len(rest) + cen.fill[si] > 1535):
                raise Undefined("the restart marker is not where the reference looks for it")
            cen.habits.append(("octets skipped", u, cen.surplus[-1]))
    return p
