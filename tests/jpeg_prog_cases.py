"""Hand-built progressive (SOF2) JPEG files for k_prog_scan (gamut_amd/csrc/jpeg_prog.hpp): a writer that takes the SYMBOLS of every scan, and
the named cases built with it -- the progressive counterpart of tests/jpeg_scan_cases.py, whose tables, bit writer and case plumbing it uses.

Every progressive stream the kernel had seen came from libjpeg, from tests/jpeg_scripts.py (natural coefficients, one grammar) or from random
damage.  The cases here stand on what those never produce: EOB runs of every size up to 32767, runs that start in step with the kernel's three
prefetch slots and across its 64-unit hand-offs, refinement symbols that pass dozens of coefficients with history, blocks whose whole band has
history, runs that find no position without history, code words of every length in front of 14 extra bits, sign and correction bits in stuffed
bytes and on both sides of the wave's 256-byte window, restart intervals that change between a scan and its refinement.

A file is a Frame (SOF2, one of the five sampling modes) and a list of Scan.  A scan lists its units (MCUs of an interleaved scan, blocks of a
single-component one), a unit its blocks, a block its items:
    DC first        (category, difference)
    DC refinement   ("bit", b)
    AC first        (rs, value)   (0xF0,)   ("eob", n, extra)            n << 4, then n extra bits
    AC refinement   (r << 4 | 1, sign bit, [correction bits])   (0xF0, [correction bits])   ("eob", n, extra, [correction bits])
                    ("corr", [correction bits])                           a block inside an EOB run: nothing but its correction bits
                    (rs, raw value, [..]) with size >= 2: what a refinement scan must not carry
    everywhere      ("cw", k, ...)  code word number k of the table, the rest as for its symbol;   ("raw", bits, n)
Only the ORDER of the items of a restart interval matters to the bytes; canonical() (the symbols an encoder writes for given coefficients, by
jpeg_scripts._scan_symbols) puts an interval's items into its first unit.

write() also says what T.81 makes of the symbols (a decoder of the symbol stream, not of the bits): the expected coefficients, or None where
the standard defines none.  cases() -> [(name, bytes, verdict)], corpus() -> the Case objects, as in jpeg_scan_cases.py."""
import os
import re

import numpy as np

import jpeg_prog_ref as P
import jpeg_scan_cases as S
import jpeg_scripts as J

Table, by_length, Bits, Case = S.Table, S.by_length, S.Bits, S.Case
ZIGZAG = S.ZIGZAG
DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE = P.DC_FIRST, P.DC_REFINE, P.AC_FIRST, P.AC_REFINE
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------------ geometry of the kernel
def geometry():
    """the numbers of gamut_amd/csrc/jpeg_prog.hpp the cases are built around"""
    src = open(os.path.join(os.path.dirname(HERE), "gamut_amd", "csrc", "jpeg_prog.hpp")).read()

    def one(pattern, what):
        m = re.search(pattern, src)
        assert m, "jpeg_prog.hpp: %s not found" % what
        return int(m.group(1))

    slots = re.findall(r"fetch\(p(\d), c\1, nu > \1\)", src)
    assert slots == [str(i) for i in range(len(slots))] and slots, "jpeg_prog.hpp: the prefetch slots not found"
    g = dict(batch=one(r"constexpr int kProgBatch = (\d+);", "kProgBatch"),
             dc_chunk=one(r"constexpr int kChunk = (\d+);", "kChunk"),
             slots=len(slots),
             t6_bits=one(r"t6 = \(e >> 8\) <= (\d+) && e \?", "the t6 look-ahead"),
             wavehuff_bits=one(r"return \(e >> 8\) <= (\d+) \? e : 0u;", "the WaveHuff look-ahead"),
             window_dwords=one(r"if \(__builtin_expect\(li >= (\d+)u, 0\)\) \{ chunk = pos >> 5;", "the WaveBits window"),
             padding=one(r"memset\(dst \+ w, 0xFF, (\d+)\); w \+= \1;", "the padding behind a segment"),
             deps=one(r"int32_t dep\[(\d+)\], dep_pipe, ctr, ctr_need;", "ProgItem::dep"))
    assert all(v > 0 for v in g.values())
    return g


# ------------------------------------------------------------------------------------------------------------------ frame and scans
class Frame:
    def __init__(self, mode, w, h):
        self.mode, self.w, self.h, self.comps = mode, w, h, S.MODES[mode]
        nc = len(self.comps)
        self.hs = [1 if nc == 1 else c[1] for c in self.comps]; self.vs = [1 if nc == 1 else c[2] for c in self.comps]
        self.hmax, self.vmax = max(self.hs), max(self.vs)
        self.mpr, self.mpc = -(-w // (8 * self.hmax)), -(-h // (8 * self.vmax))
        self.off, self.nb = [], 0
        for c in range(nc):
            self.off.append(self.nb); self.nb += self.hs[c] * self.vs[c]
        self.blocks = self.mpr * self.mpc * self.nb

    def nbx(self, c):
        return -(-(-(-self.w * self.hs[c] // self.hmax)) // 8)

    def nby(self, c):
        return -(-(-(-self.h * self.vs[c] // self.vmax)) // 8)

    def scan_geometry(self, sel):
        """-> (units, blocks_of(u) -> [(slot, dense block index)])"""
        hs, vs, off, nb, mpr = self.hs, self.vs, self.off, self.nb, self.mpr
        if len(sel) == 1:
            c = sel[0]; nbx = self.nbx(c)
            return nbx * self.nby(c), lambda u: [(0, ((u // nbx // vs[c]) * mpr + (u % nbx) // hs[c]) * nb + off[c] + ((u // nbx) % vs[c]) * hs[c] + (u % nbx) % hs[c])]
        order = [(slot, off[c] + b) for slot, c in enumerate(sel) for b in range(hs[c] * vs[c])]
        return self.mpr * self.mpc, lambda u: [(slot, u * nb + o) for slot, o in order]


def grey(nbx, nby=1):
    return Frame(0, 8 * nbx, 8 * nby)


class Scan:
    """comps: component indices; units: see the module text; dht: [(class, id, Table)] written in front of the SOS; tabs: [(Td, Ta)] per component
    of the scan (default (0, 0)); dri: a DRI segment in front of the SOS (None: none -- the interval in force stays); dqt: {id: 64 values} written in
    front of the SOS; fill: {interval: 0xFF bytes in front of the RSTn that ends it}; surplus: {interval: octets between its last byte and
    that}; trim: bytes taken off the end of the scan's data"""

    def __init__(self, comps, ss, se, ah, al, units, dht=(), tabs=None, dri=None, dqt=None, fill=None, surplus=None, pad_ones=True, trim=0):
        self.comps, self.ss, self.se, self.ah, self.al, self.units = list(comps), ss, se, ah, al, units
        self.dht, self.tabs, self.dri, self.dqt = list(dht), tabs or [(0, 0)] * len(self.comps), dri, dqt or {}
        self.fill, self.surplus, self.pad_ones, self.trim = fill or {}, surplus or {}, pad_ones, trim
        self.kind = (DC_REFINE if ah else DC_FIRST) if ss == 0 else (AC_REFINE if ah else AC_FIRST)


class _Undef(Exception):
    pass


def _resolve(it, t):
    """-> (symbol, code, length, what follows the symbol in the item)"""
    if it[0] == "cw":
        code, ln, s = t.codes[it[1]]
        return s, code, ln, it[2:]
    if it[0] == "eob":
        code, ln = t.enc[it[1] << 4]
        return it[1] << 4, code, ln, it[2:]
    code, ln = t.enc[it[0]]
    return it[0], code, ln, it[1:]


def _corr_of(kind, s, rest):
    """the correction bits an AC refinement item carries"""
    if kind != AC_REFINE:
        return []
    at = 0 if s == 0xF0 else 1
    return list(rest[at]) if len(rest) > at else []


def _put(bw, kind, it, t):
    if it[0] == "raw":
        bw.put(it[1], it[2]); return
    if it[0] == "bit":
        bw.put(it[1], 1); return
    if it[0] == "corr":
        for b in it[1]:
            bw.put(b, 1)
        return
    s, code, ln, rest = _resolve(it, t)
    bw.put(code, ln)
    r, n = s >> 4, s & 15
    if kind == DC_FIRST:
        if s:
            assert s > 15 or abs(int(rest[0])).bit_length() == s, (it, "the difference does not have the category's size")
            bw.put(S._value_bits(int(rest[0]), n) if s <= 15 else int(rest[0]), n)
    elif n:
        if kind == AC_FIRST:
            assert abs(int(rest[0])).bit_length() == n, (it, "the value does not have the size the symbol says")
            bw.put(S._value_bits(int(rest[0]), n), n)
        else:
            bw.put(int(rest[0]), n)                             # the sign bit (size 1), or the raw bits of a size no refinement scan may carry
    elif r != 15:
        assert 0 <= rest[0] < 1 << r, it
        bw.put(rest[0], r)
    for b in _corr_of(kind, s, rest):
        bw.put(b, 1)


class _Stream:
    """the items of a restart interval in order, and the correction bits the last symbol brought"""

    def __init__(self, items):
        self.items, self.i, self.corr = items, 0, []

    def next(self):
        if self.corr or self.i >= len(self.items) or self.items[self.i][0] in ("raw", "corr"):
            raise _Undef
        self.i += 1
        return self.items[self.i - 1]

    def corr_bit(self):
        if not self.corr and self.i < len(self.items) and self.items[self.i][0] == "corr":
            self.corr = list(self.items[self.i][1]); self.i += 1
        if not self.corr:
            raise _Undef
        return self.corr.pop(0)

    def done(self):
        return self.i == len(self.items) and not self.corr


def _model(fr, sc, tab, zz, dri):
    """what T.81 makes of the scan's symbols, applied to zz (blocks x 64, zig-zag order, int16 as the reference stores them); _Undef where it defines nothing"""
    units, blocks_of = fr.scan_geometry(sc.comps)
    kind, ss, se, al = sc.kind, sc.ss, sc.se, sc.al
    p1, m1 = 1 << al, -1 << al
    step = dri or units
    for u0 in range(0, units, step):
        st = _Stream([it for unit in sc.units[u0:u0 + step] for blk in unit for it in blk])

        def correct(row, k):
            if st.corr_bit():
                v = int(row[k])
                if v & p1:
                    raise _Undef
                row[k] = S._i16(v + (p1 if v >= 0 else m1))

        pred, eobrun = [0] * len(sc.comps), 0
        for u in range(u0, min(units, u0 + step)):
            for slot, blk in blocks_of(u):
                row, t = zz[blk], tab[slot]
                if kind == DC_REFINE:
                    it = st.next()
                    if it[0] != "bit":
                        raise _Undef
                    if it[1]:
                        row[0] = S._i16(int(row[0]) | p1)
                    continue
                if kind == AC_FIRST and eobrun:
                    eobrun -= 1; continue
                if kind == DC_FIRST:
                    it = st.next()
                    if it[0] == "bit":
                        raise _Undef
                    s, _, _, rest = _resolve(it, t)
                    if s > 15:
                        raise _Undef
                    pred[slot] += int(rest[0]) if s else 0
                    row[0] = S._i16(pred[slot] << al)
                    continue
                k = ss
                while k <= se and not (kind == AC_REFINE and eobrun):
                    it = st.next()
                    if it[0] == "bit":
                        raise _Undef
                    s, _, _, rest = _resolve(it, t)
                    r, n = s >> 4, s & 15
                    if kind == AC_FIRST:
                        if n:
                            k += r
                            if k > se:
                                raise _Undef
                            row[k] = S._i16(int(rest[0]) << al); k += 1
                        elif r == 15:
                            k += 16
                            if k > se + 1:
                                raise _Undef
                        else:
                            eobrun = (1 << r) + rest[0] - 1
                            break
                        continue
                    val = 0
                    st.corr = _corr_of(kind, s, rest)
                    if n:
                        if n != 1:
                            raise _Undef
                        val = p1 if rest[0] else m1
                    elif r != 15:
                        eobrun = (1 << r) + rest[0]
                        break
                    while k <= se:
                        if row[k]:
                            correct(row, k)
                        else:
                            r -= 1
                            if r < 0:
                                break
                        k += 1
                    if k > se or st.corr:
                        raise _Undef
                    if val:
                        row[k] = val
                    k += 1
                if kind == AC_REFINE and eobrun:
                    for k in range(k, se + 1):
                        if row[k]:
                            correct(row, k)
                    eobrun -= 1
        if eobrun or not st.done():
            raise _Undef


def _dqt_segment(dqt):
    out = bytearray()
    for tq in sorted(dqt):
        wide = max(dqt[tq]) > 255
        body = b"".join(int(v).to_bytes(2, "big") for v in dqt[tq]) if wide else bytes(dqt[tq])
        out += b"\xff\xdb" + (3 + len(body)).to_bytes(2, "big") + bytes([(16 if wide else 0) | tq]) + body
    return out


def write(fr, dqt, scans, cut=None):
    """-> (bytes, expect, max_zag): expect = the de-quantised int16 coefficients (blocks in MCU order, natural order), max_zag per block; both None
    where T.81 does not define them.  cut: keep that many bytes of the last scan's data"""
    out = bytearray(b"\xff\xd8") + _dqt_segment(dqt)
    comps = fr.comps
    out += b"\xff\xc2" + (8 + 3 * len(comps)).to_bytes(2, "big") + bytes([8]) + fr.h.to_bytes(2, "big") + fr.w.to_bytes(2, "big") + bytes([len(comps)])
    for cid, h, v, tq, _, _ in comps:
        out += bytes([cid, h << 4 | v, tq])
    dqt = dict(dqt)
    tab, dri = {}, 0
    zz = np.zeros((fr.blocks, 64), np.int16)
    defined = True
    for n_scan, sc in enumerate(scans):
        out += _dqt_segment(sc.dqt); dqt.update(sc.dqt)
        for tc, th, t in sc.dht:
            body = t.payload(tc, th)
            out += b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body
            tab[(tc, th)] = t
        if sc.dri is not None:
            out += b"\xff\xdd\x00\x04" + int(sc.dri).to_bytes(2, "big"); dri = sc.dri
        out += b"\xff\xda" + (6 + 2 * len(sc.comps)).to_bytes(2, "big") + bytes([len(sc.comps)])
        for c, (td, ta) in zip(sc.comps, sc.tabs):
            out += bytes([comps[c][0], td << 4 | ta])
        out += bytes([sc.ss, sc.se, sc.ah << 4 | sc.al])
        scan_at = len(out)
        units, _ = fr.scan_geometry(sc.comps)
        assert len(sc.units) == units, (n_scan, len(sc.units), units)
        mine = [tab.get((0, td) if sc.ss == 0 else (1, ta)) for td, ta in sc.tabs]
        nbs = [fr.hs[c] * fr.vs[c] if len(sc.comps) > 1 else 1 for c in sc.comps]
        slot_of = [slot for slot, n in enumerate(nbs) for _ in range(n)]
        step = dri or units
        for interval, u0 in enumerate(range(0, units, step)):
            if interval:
                out += bytes(sc.surplus.get(interval - 1, b"")) + b"\xff" * sc.fill.get(interval - 1, 0) + bytes([0xFF, 0xD0 + ((interval - 1) & 7)])
            bw = Bits()
            for unit in sc.units[u0:u0 + step]:
                for b, blk in enumerate(unit):
                    for it in blk:
                        _put(bw, sc.kind, it, mine[slot_of[b % len(slot_of)]])
            bw.flush(sc.pad_ones)
            out += bw.out
        if sc.trim:
            del out[-sc.trim:]
            defined = False
        if sc.surplus or any(it[0] == "raw" for unit in sc.units for blk in unit for it in blk):
            defined = False
        if defined:
            try:
                _model(fr, sc, mine, zz, dri)
            except _Undef:
                defined = False
    if cut is not None:
        del out[scan_at + cut:]
        defined = False
    out += b"\xff\xd9"
    if not defined:
        return bytes(out), None, None
    expect = np.zeros_like(zz)
    per = [comps[c][3] for c in range(len(comps)) for _ in range(fr.hs[c] * fr.vs[c])]
    for b in range(fr.nb):
        q = np.array(dqt[per[b]], np.int64)
        expect[b::fr.nb, ZIGZAG] = (zz[b::fr.nb].astype(np.int64) * q).astype(np.int16)
    last = np.zeros(len(zz), int)
    for z in range(63, 0, -1):
        hit = (zz[:, z] != 0) & (last == 0)
        last[hit] = z
    return bytes(out), expect, (last + 1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ symbols from coefficients
def canonical(fr, planes, comps, ss, se, ah, al, dri=0):
    """the units of the scan an encoder writes for the quantised coefficients `planes` (blocks x 64, natural order, MCU order): the symbols of
    jpeg_scripts._scan_symbols, every restart interval's items in its first unit"""
    units, blocks_of = fr.scan_geometry(comps)
    segs = J._scan_symbols(lambda u: [(slot, planes[b]) for slot, b in blocks_of(u)], comps, ss, se, ah, al, units, dri)
    kind = (DC_REFINE if ah else DC_FIRST) if ss == 0 else (AC_REFINE if ah else AC_FIRST)
    out = [[] for _ in range(units)]
    for i, ev in enumerate(segs):
        items, j = [], 0
        while j < len(ev):
            e = ev[j]; j += 1
            if e[0] == "b":
                assert kind == DC_REFINE and e[2] == 1
                items.append(("bit", e[1])); continue
            s = e[1]
            r, n = s >> 4, s & 15
            it = [s]
            if kind == DC_FIRST:
                n = s
            if n or (kind != DC_FIRST and r != 15 and r):
                v = ev[j][1]; j += 1
                if n and kind != AC_REFINE:
                    v = v if v >= 0 else v + 1
                it.append(v)
            elif kind != DC_FIRST and r != 15:
                it.append(0)
            if kind == DC_FIRST and not s:
                it.append(0)
            if kind == AC_REFINE:
                corr = []
                while j < len(ev) and ev[j][0] == "b":
                    corr.append(ev[j][1]); j += 1
                it.append(corr)
            if kind != DC_FIRST and not n and r != 15:
                it = ["eob", r] + it[1:]
            items.append(tuple(it))
        u0 = i * (dri or units)
        if ss:
            out[u0] = [items]
            continue
        at = 0                                                 # a DC scan: one item per block, and the blocks of an MCU have tables of their own
        for u in range(u0, min(units, u0 + (dri or units))):
            nblk = len(blocks_of(u))
            out[u] = [[it] for it in items[at:at + nblk]]; at += nblk
        assert at == len(items)
    return out


def refine_block(hist, ops, ss=1, se=63, bit=lambda i: i & 1):
    """the items of one AC refinement block over the positions `hist` that have history.  ops: (run, sign bit) -- a new coefficient behind `run`
    positions without history --, "zrl", or ("eob", n, extra), which ends the block; the correction bits of every symbol are counted by walking
    the band as a decoder does (a run that finds too few positions takes the correction bits of all that is left), their values are bit(i)"""
    hist = set(hist)
    its, k, i = [], ss, 0
    for op in ops:
        if op[0] == "eob":
            c = len([z for z in range(k, se + 1) if z in hist])
            its.append(("eob", op[1], op[2], [bit(i + j) for j in range(c)]))
            return its
        r = 15 if op == "zrl" else op[0]
        c = 0
        while k <= se:
            if k in hist:
                c += 1
            else:
                r -= 1
                if r < 0:
                    break
            k += 1
        corr = [bit(i + j) for j in range(c)]; i += c
        its.append((0xF0, corr) if op == "zrl" else (op[0] << 4 | 1, op[1], corr))
        k += 1
    return its


def items_of(units):
    return [it for unit in units for blk in unit for it in blk]


def table_for(units, length=None, lengths=None, extra=()):
    """a table that holds the symbols the units use (and `extra`): every code `length` bits (default: the shortest that leaves the all-ones word
    free), or the listed lengths handed out in the order the symbols first appear"""
    syms = []
    for it in items_of(units):
        if it[0] in ("raw", "bit", "corr", "cw"):
            continue
        s = it[1] << 4 if it[0] == "eob" else it[0]
        if s not in syms:
            syms.append(s)
    for s in extra:
        if s not in syms:
            syms.append(s)
    syms = syms or [0]
    if lengths is not None:
        assert len(lengths) >= len(syms), (len(lengths), len(syms))
        return by_length(list(zip(lengths, syms)))
    if length is None:
        length = max(1, len(syms).bit_length())
    return by_length([(length, s) for s in syms])


def first_block(coeffs, ss=1, se=63, eob=True):
    """AC first items of one block: {zig-zag position: value (already shifted down by Al)}, closed by EOB0 unless the band is full"""
    out, k = [], ss
    for z in sorted(coeffs):
        v = int(coeffs[z])
        r = z - k
        while r > 15:
            out.append((0xF0,)); r -= 16
        out.append((r << 4 | abs(v).bit_length(), v)); k = z + 1
    if k <= se and eob:
        out.append(("eob", 0, 0))
    return out


def dc_units(values):
    """DC first units of a single-component scan: the values (already shifted down by Al) as differences"""
    out, pred = [], 0
    for v in values:
        d = int(v) - pred; pred = int(v)
        out.append([[(abs(d).bit_length(), d)]])
    return out


def cover(n):
    """EOB symbols (n, extra) that cover n blocks, the largest first"""
    out = []
    while n:
        e = min(14, n.bit_length() - 1)
        extra = min(n - (1 << e), (1 << e) - 1)
        out.append((e, extra)); n -= (1 << e) + extra
    return out


def runs_plan(plan, new=lambda u: [(0x01, 1)]):
    """units of an AC first scan over a band of ONE position from a plan of 'c' (a coefficient: the block is full) and integers (an EOB run of
    that many blocks)"""
    units = []
    for p in plan:
        if p == "c":
            units.append([new(len(units))])
        else:
            (e, extra), = cover(p)
            units.append([[("eob", e, extra)]])
            units += [[[]] for _ in range(p - 1)]
    return units


DC_1BIT = by_length([(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6), (8, 7), (9, 8), (10, 9), (11, 10), (12, 11)])      # category 0: one bit
Q1 = S.Q1
q_ramp = S.q_ramp
_made = None


def corpus():
    global _made
    if _made is None:
        _made = _build()
    return _made


def cases():
    return [(c.name, c.data, c.verdict) for c in corpus()]


FAMILIES = ("eobrun", "ac_first", "ac_refine", "dc", "script")


def _build():
    g = geometry()
    BATCH, CHUNK, SLOTS, DEPS = (g[k] for k in ("batch", "dc_chunk", "slots", "deps"))        # (the look-aheads, the window and the padding: the tests' claims)
    out, names = [], set()

    def add(name, family, made, verdict="image", wellformed=True, **claims):
        data, expect, max_zag = made
        assert name not in names and family in FAMILIES
        names.add(name)
        if wellformed:
            assert expect is not None, (name, "T.81 does not define what the writer was given")
        c = Case(name, family, data, verdict, expect if wellformed else None, wellformed, claims)
        c.max_zag = max_zag if wellformed else None
        out.append(c)

    def dc0(fr, comps=(0,), table=S.FLAT_DC, al=0, value=lambda b: (b * 37) % 200 - 100):
        """a DC first scan: a value per block of the scan"""
        units, blocks_of = fr.scan_geometry(list(comps))
        us, pred = [], [0] * len(comps)
        for u in range(units):
            blks = []
            for slot, b in blocks_of(u):
                v = value(b); d = v - pred[slot]; pred[slot] = v
                blks.append([(abs(d).bit_length(), d)])
            us.append(blks)
        return Scan(comps, 0, 0, 0, al, us, dht=[(0, 0, table)])

    def ac(ss, se, ah, al, units, length=None, lengths=None, extra=(), table=None, **kw):
        """an AC scan of component 0 with a table made for its symbols"""
        t = table or table_for(units, length, lengths, extra)
        return Scan([0], ss, se, ah, al, units, dht=[(1, 0, t)], **kw)

    def blocks(n, f):
        return [[f(u)] for u in range(n)]

    # ================================================================================================================ EOB runs in AC first scans
    # large case one: 182 x 181 grey blocks, every AC coefficient 0, the DC scan a 1-bit code per block: a run of 32767 (EOB14, extra bits all one), 16384
    # (all zero), and with them every EOBn from 0 to 14 with both kinds of extra bits, each run as long as the scan allows
    fr = grey(182, 181)
    n = fr.blocks

    def eob_scan(band, head):
        """runs as listed, then whatever covers the rest of the scan"""
        runs = list(head) + cover(n - sum((1 << e) + x for e, x in head))
        us = []
        for e, x in runs:
            us.append([[("eob", e, x)]]); us += [[[]] for _ in range((1 << e) + x - 1)]
        assert len(us) == n
        return ac(band, band, 0, 0, us, lengths=list(range(1, 17))), [e for e, _ in runs]

    s1, e1 = eob_scan(1, [(14, (1 << 14) - 1)])
    s2, e2 = eob_scan(2, [(13, 0), (12, 0), (11, (1 << 11) - 1), (10, 0), (9, (1 << 9) - 1), (8, 0), (6, 63), (4, 0), (2, 3), (0, 0)])
    s3, e3 = eob_scan(3, [(14, 0), (12, (1 << 12) - 1), (11, 0), (10, (1 << 10) - 1), (9, 0), (8, 255), (7, 0), (7, 127), (6, 0), (5, 31), (5, 0), (4, 15), (3, 7), (3, 0), (2, 0), (1, 1), (1, 0)])
    s4, e4 = eob_scan(4, [(13, (1 << 13) - 1), (12, (1 << 12) - 1)])
    assert set(e1 + e2 + e3 + e4) == set(range(15))
    zero_dc = Scan([0], 0, 0, 0, 0, [[[(0, 0)]] for _ in range(n)], dht=[(0, 0, DC_1BIT)])
    add("eob14_all_ones_run_of_32767_blocks_and_every_eobn_0_to_14_182x181_blocks", "eobrun", write(fr, {0: Q1}, [zero_dc, s1, s2, s3, s4]),
        max_eobrun=32767, eob_sizes=range(15), extra_all_ones=[14, 13, 12], extra_all_zero=[14, 13, 12], file_below=8192)

    # runs of 1 .. 5 blocks that start at a unit = 0, 1, 2 (mod the prefetch slots), then runs that start at units BATCH - 2, - 1, + 0 of the next batches:
    # a first scan over position 1 (Al = 1), and the refinement of the same band, whose blocks without history are the free skip
    plan, starts = [], {}
    for length in range(1, 6):
        for res in range(SLOTS):
            at = sum(1 if p == "c" else p for p in plan)
            while at % SLOTS != res:
                plan.append("c"); at += 1
            starts[(length, res)] = at
            plan += [length, "c"]
    at = sum(1 if p == "c" else p for p in plan)
    assert at < 2 * BATCH - 2
    edge = []
    for k, d in enumerate((-2, -1, 0)):                        # (three runs cannot start at 62, 63 and 64 of ONE batch: the edges of three batches)
        want = (k + 2) * BATCH + d
        plan += ["c"] * (want - at) + [4]; edge.append(want); at = want + 4
    total = 6 * BATCH - 8
    plan += ["c"] * (total - at - 3) + [3]                      # ... and a run that ends exactly on the scan's last block
    fr = grey(total // 8, 8)
    assert fr.blocks == total
    first = runs_plan(plan, lambda u: [(0x01, 1 if u % 3 else -1)])
    # the refinement: every block with history carries one correction bit; blocks in a run of the first scan have no history: a run of the same length
    ref, u = [], 0
    for p in plan:
        if p == "c":
            ref.append([[("eob", 0, 0, [u & 1])]]); u += 1
        else:
            (e, x), = cover(p)
            ref.append([[("eob", e, x, [])]]); ref += [[[]] for _ in range(p - 1)]; u += p
    add("eob_runs_of_1_to_5_at_every_prefetch_slot_and_at_units_62_63_64_of_a_batch", "eobrun",
        write(fr, {0: q_ramp(1)}, [dc0(fr), ac(1, 1, 0, 1, first, length=3), ac(1, 1, 1, 0, ref, length=3)]),
        run_starts=sorted(starts.values()) + edge + [total - 3], run_start_residues=SLOTS, ends_on_last_block=True, band_of_one=True)

    # every EOBn a small scan has room for, extra bits all zero and all one, through the three look-aheads: code lengths 1 .. 16
    fr = grey(20, 10)
    scans = [dc0(fr)]
    for band, (e, x) in enumerate([(0, 0), (1, 0), (1, 1), (2, 0), (2, 3), (3, 0), (3, 7), (4, 0), (4, 15), (5, 0), (5, 31), (6, 0), (6, 63), (7, 0), (7, 71)], 1):
        run = (1 << e) + x                                     # coefficients, the run, one more coefficient; code lengths band and band + 1
        us = [[[(0x01, 1)]] for _ in range(200 - run - 1)] + [[[("eob", e, x)]]] + [[[]] for _ in range(run - 1)] + [[[(0x01, -1)]]]
        scans.append(ac(band, band, 0, 0, us, lengths=[band, band + 1]))
    add("eob0_to_eob7_extra_bits_all_zero_and_all_one_20x10_blocks", "eobrun", write(fr, {0: q_ramp(1)}, scans), eob_sizes=range(8), hand_offs=3,
        code_lengths=range(1, 17))

    fr = grey(9, 8)                                            # 72 blocks: one hand-off
    us = [[[(0x01, 1)]] for _ in range(4)] + [[[("eob", 5, 0)]]] + [[[]] for _ in range(31)] + [[[(0x01, -1)]] for _ in range(35)] + [[[("eob", 0, 0)]]]
    add("eob_run_ends_in_front_of_rst_dri_36", "eobrun", write(fr, {0: Q1}, [dc0(fr), ac(1, 1, 0, 0, us, dri=36)]), run_ends_at_interval_end=36)
    us = [[[(0x01, 1)]] for _ in range(30)] + [[[("eob", 3, 0)]]] + [[[]] for _ in range(5)] + [[[(0x01, -1)]] for _ in range(36)]
    add("eob_run_longer_than_its_restart_interval_dropped_at_rst_habit", "eobrun",
        write(fr, {0: Q1}, [dc0(fr), ac(1, 1, 0, 0, us, dri=36)]), wellformed=False, habit="EOB run dropped")
    us = [[[(0x01, 1)]] for _ in range(70)] + [[[("eob", 9, 100)]]] + [[[]]]
    add("eob_run_longer_than_its_scan_dropped_at_the_end_habit", "eobrun", write(fr, {0: Q1}, [dc0(fr), ac(1, 1, 0, 0, us)]), wellformed=False, habit="EOB run dropped")
    for e in range(8, 15):                                     # ... of every size a small scan has no room for
        us = [[[("eob", e, (1 << e) - 1 if e % 2 else 0)]]] + [[[]] for _ in range(71)]
        scans_ = [dc0(fr), ac(1, 5, 0, 0, us, lengths=[16]), ac(6, 63, 0, 0, blocks(72, lambda u: first_block({6 + u % 58: 1 + u % 3}, 6)), length=8)]
        add("eob%d_in_a_scan_of_72_blocks_dropped_at_the_end_habit" % e, "eobrun", write(fr, {0: q_ramp(1)}, scans_), wellformed=False, habit="EOB run dropped")

    # ================================================================================================================ AC first grammar
    rng = np.random.default_rng(1)

    def natural(k_lo=1, k_hi=63, n=6, top=30):
        return {int(z): int(rng.integers(1, top)) * (1 if rng.integers(2) else -1) for z in rng.choice(np.arange(k_lo, k_hi + 1), min(n, k_hi - k_lo + 1), replace=False)}

    def around(special, ss=1, se=63, n=8):
        us = blocks(n, lambda u: first_block(natural(ss, se), ss, se))
        us[n // 2] = [special]
        return us

    fr8 = grey(4, 2)
    base = [dc0(fr8)]
    add("run_lands_exactly_on_se_20", "ac_first", write(fr8, {0: q_ramp(1)}, base + [ac(1, 20, 0, 0, around([(0x01, 1), (0xF0,), (0x22, -3)], 1, 20), length=8)]), lands_on_se=1)
    late = ac(11, 63, 0, 0, blocks(8, lambda u: first_block({12: 2 + u, 40: -1}, 11)), length=8)
    add("run_lands_past_se_10_on_12_inside_the_band_of_a_later_scan_habit", "ac_first",
        write(fr8, {0: q_ramp(1)}, base + [ac(1, 10, 0, 0, around([(0x01, 1), (0xA3, 5)], 1, 10), length=8), late]), wellformed=False, habit="run past Se")
    add("run_lands_past_se_10_on_12_an_earlier_scan_wrote_habit", "ac_first",
        write(fr8, {0: q_ramp(1)}, base + [late, ac(1, 10, 0, 0, around([(0x01, 1), (0xA3, 5)], 1, 10), length=8)]), wellformed=False, habit="run past Se")
    add("run_lands_past_63", "ac_first", write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, around([(0x01, 1), (0xF0,), (0xF0,), (0xF0,), (0xF2, -3)]), length=8)]),
        "null", wellformed=False)
    add("zrl_x3_then_a_coefficient_at_63", "ac_first", write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, around([(0xF0,), (0xF0,), (0xF0,), (0xE4, 9)]), length=8)]),
        symbols={"zrl": 3}, lands_on_se=1)
    add("zrl_reaches_64", "ac_first", write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, around([(0x01, 1)] * 15 + [(0xF0,)] * 3), length=8)]), symbols={"zrl": 3})
    add("zrl_past_64", "ac_first", write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, around([(0x01, 1)] * 16 + [(0xF0,)] * 3), length=8)]), "null", wellformed=False)
    add("ac_sizes_11_to_15", "ac_first",
        write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, around([(s, ((1 << s) - 1 - s) * (-1) ** s) for s in range(11, 16)] + [(0x2B, 1024), ("eob", 0, 0)]), length=8)]),
        symbols={("ac", 11): 2, ("ac", 15): 1})
    for al in range(0, 14):
        size = min(16 - al, 15)                                # the value's top bit lands on bit 15: the stored value wraps (Al = 0: size 15 is the largest there is, it fits)
        us = around([(size, (1 << (size - 1)) | 1), (0x11, -1), (size, -((1 << size) - 1)), ("eob", 0, 0)])
        add("value_shifted_by_al_%d_%s" % (al, "leaves_int16" if al else "largest_size_fits"), "ac_first",
            write(fr8, {0: q_ramp(1)}, [dc0(fr8), ac(1, 63, 0, al, us, length=8)]), left_int16=2 if al else 0, al=al)
    add("bands_1_1_and_63_63_and_2_62", "ac_first",
        write(fr8, {0: q_ramp(2)}, base + [ac(63, 63, 0, 0, blocks(8, lambda u: [(0x03, 4 + u % 4)] if u % 3 else [("eob", 0, 0)]), length=2),
                                           ac(1, 1, 0, 0, blocks(8, lambda u: [(0x02, -2 - u % 2)] if u % 2 else [("eob", 0, 0)]), length=2),
                                           ac(2, 62, 0, 0, blocks(8, lambda u: first_block(natural(2, 62), 2, 62)), length=8)]), bands=[(63, 63), (1, 1), (2, 62)])
    add("band_1_63_every_coefficient_coded", "ac_first",
        write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, blocks(8, lambda u: [(z % 7 + 1, (1 << (z % 7)) * (-1) ** (z + u)) for z in range(1, 64)]), length=4)]), bands=[(1, 63)])
    one = blocks(8, lambda u: first_block({1 + u: 5, 20: -7, 33: 2}))
    two = blocks(8, lambda u: first_block({2 + u: 3, 33: -1, 50: 1}))
    add("two_first_scans_over_one_band_the_second_leaves_what_it_does_not_code", "ac_first",
        write(fr8, {0: q_ramp(1)}, base + [ac(1, 63, 0, 0, one, length=8), ac(1, 63, 0, 0, two, length=8)]), scans_of_kind={AC_FIRST: 2})

    # ================================================================================================================ AC refinement
    def hist_scan(hists, al=1, ss=1, se=63, value=lambda u, z: 1 if (u + z) % 3 else -1):
        """the first scan under a refinement: {position: value} per block from the positions listed"""
        return ac(ss, se, 0, al, blocks(len(hists), lambda u: first_block({z: value(u, z) for z in hists[u]}, ss, se)), length=8, extra=[0])

    def refine(units, ss=1, se=63, al=0, **kw):
        return ac(ss, se, al + 1, al, units, **kw)

    full = list(range(1, 64))
    add("no_history_63_new_coefficients", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [refine(blocks(8, lambda u: [(0x01, (z + u) & 1, []) for z in range(1, 64)]), length=1)]), new_per_block=63, no_first_scan=True)
    for name, bits in (("all_0", [0] * 63), ("all_1", [1] * 63), ("alternating", [z & 1 for z in range(63)])):
        us = []
        for pair in range(4):
            us += [[[("eob", 1, 0, bits)]], [[("corr", bits[::-1] if pair % 2 else bits)]]]
        add("whole_band_has_history_eob1_and_63_correction_bits_%s_both_signs" % name, "ac_refine",
            write(fr8, {0: q_ramp(1)}, base + [hist_scan([full] * 8), refine(us, length=2)]), history_is=63, corr_after_eob=63, both_signs=True)
    us = blocks(8, lambda u: refine_block(range(1, 41 + u % 3), [(15, u & 1), ("eob", 0, 0)], bit=lambda i: (i + u) & 1))
    add("one_symbol_of_run_15_passes_40_and_more_coefficients_with_history", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([list(range(1, 41 + u % 3)) for u in range(8)]), refine(us, length=2)]), corr_behind_symbol=(0xF1, 40))
    hz = [z for z in range(1, 64) if z % 3 == 0]               # history at every third position: a ZRL passes 16 without and 7 or 8 with
    us = blocks(8, lambda u: refine_block(hz, ["zrl", "zrl", (4, 1), ("eob", 0, 0)], bit=lambda i: (i * 3 + u) & 1))
    add("zrl_with_history_in_between", "ac_refine", write(fr8, {0: q_ramp(1)}, base + [hist_scan([hz] * 8), refine(us, length=3)]), symbols={"zrl": 16}, corr_behind_symbol=(0xF0, 7))
    # runs that find fewer positions without history than they ask for (the reference sets position Se + 1, if there is one, and goes on)
    few = [z for z in range(1, 64) if z not in (5, 17, 29, 41, 60)]
    us = blocks(8, lambda u: refine_block(few, [(7, 1)] if u % 2 else ["zrl"], bit=lambda i: (i + u) & 1))
    add("run_and_zrl_with_fewer_positions_without_history_than_they_ask_for_se_63_habit", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([few] * 8), refine(us, length=2)]), wellformed=False, habit="starved run", starved=8)
    few20 = [z for z in range(1, 21) if z not in (5, 17)]
    us = blocks(8, lambda u: refine_block(few20, [(7, (u >> 1) & 1)] if u % 2 else ["zrl"], se=20, bit=lambda i: (i + u) & 1))
    tail = ac(21, 63, 0, 1, blocks(8, lambda u: first_block({21: 3, 30 + u: -1}, 21)), length=8)
    add("run_with_fewer_positions_than_it_asks_for_se_20_sets_21_of_a_later_scan_habit", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([few20] * 8, se=20), refine(us, se=20, length=2), tail]), wellformed=False, habit="starved run", starved=8, past_band=21)
    add("run_with_fewer_positions_than_it_asks_for_se_20_sets_21_an_earlier_scan_wrote_habit", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [tail, hist_scan([few20] * 8, se=20), refine(us, se=20, length=2)]), wellformed=False, habit="starved run", starved=8, past_band=21)
    add("new_coefficient_lands_on_se_20_exactly_a_later_scan_owns_21", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([[z for z in range(1, 20) if z != 5]] * 8, se=20),
                                           refine(blocks(8, lambda u: refine_block([z for z in range(1, 20) if z != 5], [(0, 1), (0, u & 1)], se=20)), se=20, length=2), tail]),
        lands_on_se=8)
    add("correction_bit_for_a_bit_plane_that_is_already_set_habit", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([[1, 2, 3, 9]] * 8, al=0, value=lambda u, z: (3, -3, 2, -2)[(u + z) % 4]),
                                           Scan([0], 1, 63, 1, 0, blocks(8, lambda u: [("eob", 0, 0, [1, 1, u & 1, 1])]), dht=[(1, 0, by_length([(1, 0)]))])]),
        wellformed=False, habit_plane_set=True)
    add("size_2_symbol_in_a_refinement_scan", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([[1, 2]] * 8), refine(blocks(8, lambda u: [(0x02, 3, [1, 1]), ("eob", 0, 0, [])] if u == 4 else [("eob", 0, 0, [1, 0])]), length=2)]),
        "null", wellformed=False)

    # EOBn over alternating blocks with and without history, across the hand-offs at 63 / 64 and 127 / 128 and across a restart
    fr200 = grey(20, 10)
    hists = [[] if u % 2 else [1 + u % 60, 2 + u % 60] for u in range(200)]
    for u in (62, 63, 64, 65, 126, 127, 128, 129):
        hists[u] = [3, 7, 11] if u % 2 == 0 else []
    hists[63] = [5]; hists[128] = []
    us = [[[]] for _ in range(200)]
    at = 0
    for e, x in [(5, 28), (2, 1), (6, 40), (0, 0), (5, 0), (4, 2)]:          # 60, 5, 104, 1, 32 ... blocks: runs that straddle 63 / 64 and 127 / 128
        run = (1 << e) + x
        if at >= 200:
            break
        if at + run > 200:
            run = 200 - at; (e, x), = cover(run)
        bits = lambda u: [(u + i) & 1 for i in range(len(hists[u]))]
        us[at] = [[("eob", e, x, bits(at))]]
        for u in range(at + 1, at + run):
            if hists[u]:
                us[u] = [[("corr", bits(u))]]
        at += run
    assert at == 200
    add("eobn_over_blocks_with_and_without_history_across_the_hand_offs", "ac_refine",
        write(fr200, {0: q_ramp(1)}, [dc0(fr200), hist_scan(hists), refine(us, length=3)]), free_skips_and_corr_only=(63, 64, 127, 128), hand_offs=3)
    us_r = [[[]] for _ in range(200)]
    for at in range(0, 200, 50):
        bits = lambda u: [(u + i) & 1 for i in range(len(hists[u]))]
        us_r[at] = [[("eob", 5, 18, bits(at))]]
        for u in range(at + 1, at + 50):
            if hists[u]:
                us_r[u] = [[("corr", bits(u))]]
    add("eobn_over_blocks_with_and_without_history_across_restarts_dri_50", "ac_refine",
        write(fr200, {0: q_ramp(1)}, [dc0(fr200), ac(1, 63, 0, 1, blocks(200, lambda u: first_block({z: 1 if (u + z) % 3 else -1 for z in hists[u]})), length=8, extra=[0], dri=50),
                                      refine(us_r, length=3)]), free_skips_and_corr_only=(49, 50, 99, 100), intervals=4)
    # EOB14 in a refinement scan (longer than the scan: the reference drops what is left), behind a 16-bit code word
    us = [[[("eob", 14, 0x2AAA, [1, 0])]]] + [[[("corr", [u & 1, 1])]] for u in range(1, 8)]
    add("eob14_behind_a_16_bit_code_word_in_a_refinement_scan_dropped_at_the_end_habit", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan([[2, 9]] * 8), refine(us, lengths=[16])]), wellformed=False, habit="EOB run dropped", code_in_front_of_extra=(16, 14))

    # code words of every length 1 .. 16 in a refinement scan: new coefficients of run 0 .. 14, ZRL and EOB0 -- one table per length class, and the comb
    hist16 = [[20, 40, 60]] * 8
    syms = [(r << 4) | 1 for r in range(14)] + [0xF0, 0x00]
    T6, WH = g["t6_bits"], g["wavehuff_bits"]
    assert (T6, WH) == (6, 8), "the labels below say 6 and 8"
    for lens, label in ((list(range(1, 17)), "comb_1_to_16"), ([T6 + 1] * 8 + [WH] * 8, "7_and_8_wavehuff"), ([min(16, WH + 1 + i // 2) for i in range(16)], "9_to_16_canonical_search"),
                        ([3 + i * (T6 - 3) // 7 for i in range(8)] + [WH + 1] * 8, "3_to_6_look_ahead_word")):
        for rot in (0, 7):
            order = syms[rot:] + syms[:rot]                     # which symbol gets which length
            t = by_length(list(zip(lens, order)))

            def blk(u):
                """block u: the new coefficients of run 2u and 2u + 1 (the last block: a ZRL and run 0), then EOB0 -- every symbol of the table in eight blocks"""
                ops = [(2 * u, u & 1), (2 * u + 1, 1)] if u < 7 else ["zrl", (0, 0)]
                return refine_block(hist16[u], ops + [("eob", 0, 0)], bit=lambda i: (i + u) & 1)
            add("refinement_code_lengths_%s_rotated_%d" % (label, rot), "ac_refine",
                write(fr8, {0: q_ramp(1)}, base + [hist_scan(hist16), refine(blocks(8, blk), table=t)]), code_lengths=sorted(set(lens)))

    # sign and correction bits inside stuffed bytes: a complete code whose all-ones word (one bit) is the new coefficient of run 0, every sign and
    # correction bit a one
    hist_w = [full[::2]] * 4 + [full] * 4
    us = blocks(8, lambda u: refine_block(hist_w[u], [(0, 1)] * 31 + [("eob", 0, 0)] if u < 4 else [("eob", 0, 0)], bit=lambda i: 1))
    add("sign_and_correction_bits_inside_stuffed_ff_bytes", "ac_refine",
        write(fr8, {0: q_ramp(1)}, base + [hist_scan(hist_w), refine(us, table=by_length([(1, 0x00), (1, 0x01)]))]), stuffed_with_bits=True)
    # blocks of some 125 bits: symbols, sign and correction bits on both sides of every reload of the wave's window
    frw = grey(8, 4)
    hw = [[z for z in range(1, 64) if (z + u) % 2] for u in range(32)]

    def wblk(u):
        ops = [(0, (u + j) & 1) for j in range(63 - len(hw[u]))]
        return refine_block(hw[u], ops + ([("eob", 0, 0)] if 63 in hw[u] else []), bit=lambda i: (i * 5 + u) & 1)
    add("blocks_on_both_sides_of_the_window_reload", "ac_refine",
        write(frw, {0: q_ramp(1)}, [dc0(frw), hist_scan(hw), refine(blocks(32, wblk), length=2)]), straddles_reload=True)
    # the last bit of the segment is a sign bit (7 x 5 + 9 + 4 = 48 bits); and a segment of 57 bits whose last byte -- that sign bit and the padding, a
    # stuffed 0xFF -- is gone: ones from behind the data answer
    t_last = by_length([(2, 0x01), (2, 0x00), (3, 0xF0), (3, 0xE1), (3, 0xB1)])
    us = blocks(8, lambda u: [(0x01, 1, []), ("eob", 0, 0, [])] if u < 7 else [(0xF0, []), (0xF0, []), (0xF0, []), (0xE1, 1, [])])
    add("sign_bit_is_the_last_bit_of_its_segment", "ac_refine", write(fr8, {0: q_ramp(1)}, base + [refine(us, table=t_last)]), sign_is_last_bit=True)
    us = blocks(8, lambda u: [(0x01, 1, []), ("eob", 0, 0, [])] if u < 7 else [(0x01, 1, [])] * 3 + [(0xF0, []), (0xF0, []), (0xF0, []), (0xB1, 1, [])])
    add("segment_one_bit_short_the_padding_answers_habit", "ac_refine", write(fr8, {0: q_ramp(1)}, base + [refine(us, table=t_last, trim=2)]), wellformed=False, past_end=1)
    for al in range(0, 14):                                    # (Al = 13 stands on a first scan with Al = 14: beyond T.81, the reference's nibble)
        us = blocks(8, lambda u: refine_block([1, 4, 5, 30, 44], [(1, u & 1), (0, 1), ("eob", 0, 0)], bit=lambda i: (i + u) & 1))
        add("refinement_al_%d_negative_history" % al, "ac_refine",
            write(fr8, {0: q_ramp(1)}, base + [hist_scan([[1, 4, 5, 30, 44]] * 8, al=al + 1, value=lambda u, z: -1 if (u + z) % 4 else 1), refine(us, al=al, length=2)]),
            al=al, negative_history=True)

    # ================================================================================================================ DC
    for al in range(0, 14):
        top = (1 << (15 - al)) - 1 if al else 2047
        add("dc_first_al_%d" % al, "dc", write(fr8, {0: q_ramp(1)}, [dc0(fr8, al=al, value=lambda b: ((b * 977) % (2 * top + 1)) - top)]), al=al)
    vals, v = [], 0
    for b in range(72):
        v += 2047 if (b // 24) % 2 == 0 else -2047
        vals.append(v)
    fr72 = grey(9, 8)
    add("dc_predictor_driven_out_of_int16_by_differences_of_2047", "dc", write(fr72, {0: q_ramp(1)}, [Scan([0], 0, 0, 0, 0, dc_units(vals), dht=[(0, 0, S.COMB_DC)])]), left_int16=10)
    add("dc_categories_12_to_15", "dc",
        write(fr8, {0: q_ramp(1)}, [Scan([0], 0, 0, 0, 0, blocks(8, lambda u: [(12 + u % 4, ((1 << (12 + u % 4)) - 1 - u) * (-1) ** (u // 4))]), dht=[(0, 0, S.COMB_DC)])]),
        symbols={("dc", 12): 2, ("dc", 15): 2})
    dc17 = by_length([(5, s) for s in range(16)] + [(6, 17)])
    add("dc_category_above_15_routed_to_the_host", "dc",
        write(fr8, {0: q_ramp(1)}, [Scan([0], 0, 0, 0, 0, blocks(8, lambda u: [(17, 1)] if u == 4 else [(3, 5)]), dht=[(0, 0, dc17)])]), "undefined", wellformed=False)
    for mode, (w, h) in ((1, (20, 12)), (2, (40, 12)), (3, (12, 40)), (4, (40, 24))):
        fr = Frame(mode, w, h)
        planes = np.zeros((fr.blocks, 64), np.int32)
        r = np.random.default_rng(40 + mode)
        planes[:, 0] = r.integers(-900, 900, fr.blocks)
        for z in (1, 2, 9, 63):
            planes[:, z] = r.integers(-3, 4, fr.blocks)
        dht = [(0, 0, S.FLAT_DC), (0, 1, S.COMB_DC)]
        scans = [Scan([0, 1, 2], 0, 0, 0, 1, canonical(fr, planes, [0, 1, 2], 0, 0, 0, 1), dht=dht, tabs=[(0, 0), (1, 0), (1, 0)])]
        for c in range(3):
            us = canonical(fr, planes, [c], 1, 63, 0, 0)
            scans.append(Scan([c], 1, 63, 0, 0, us, dht=[(1, 0, table_for(us, 8))]))
        scans.append(Scan([0, 1, 2], 0, 0, 1, 0, canonical(fr, planes, [0, 1, 2], 0, 0, 1, 0)))
        add("interleaved_dc_first_and_refinement_partial_mcus_scan_type_%d" % mode, "dc", write(fr, {0: q_ramp(1), 1: q_ramp(2)}, scans), scan_type=mode, blocks_per_unit=fr.nb)
        # non-interleaved DC scans of every component: the blocks outside the component's own nbx x nby stay 0
        scans = []
        for c in range(3):
            scans.append(Scan([c], 0, 0, 0, 1, canonical(fr, planes, [c], 0, 0, 0, 1), dht=[(0, 0, S.COMB_DC)]))
        for c in range(3):
            scans.append(Scan([c], 0, 0, 1, 0, canonical(fr, planes, [c], 0, 0, 1, 0)))
        if fr.nbx(0) < fr.mpr * fr.hs[0] or fr.nby(0) < fr.mpc * fr.vs[0]:
            add("non_interleaved_dc_scans_blocks_outside_nbx_stay_0_scan_type_%d" % mode, "dc", write(fr, {0: q_ramp(1), 1: q_ramp(2)}, scans), scan_type=mode, outside_stay_zero=True)
    # large case two: DC refinement over more units than the lane-per-bit loop takes between two looks at the first scan's progress, negative values
    frc = grey(33, 32)
    assert frc.blocks > CHUNK
    vals = [((b * 131) % 1001) - 500 for b in range(frc.blocks)]
    add("dc_refinement_over_33x32_blocks_more_than_kchunk_negative_values", "dc",
        write(frc, {0: q_ramp(1)}, [Scan([0], 0, 0, 0, 1, dc_units([v >> 1 for v in vals]), dht=[(0, 0, S.FLAT_DC)]),
                                    Scan([0], 0, 0, 1, 0, [[[("bit", v & 1)]] for v in vals])]), units_over=CHUNK, negative_values=True)
    vals = [((b * 71) % 301) - 150 for b in range(72)]
    add("dc_refinement_segment_shorter_than_its_bits_ones_from_behind_the_data_habit", "dc",
        write(fr72, {0: q_ramp(1)}, [Scan([0], 0, 0, 0, 1, dc_units([v >> 1 for v in vals]), dht=[(0, 0, S.FLAT_DC)]),
                                     Scan([0], 0, 0, 1, 0, [[[("bit", (u * 5 // 3) & 1)]] for u in range(72)], trim=2)]), wellformed=False, past_end=True)

    # ================================================================================================================ scripts and restart
    fr = Frame(4, 72, 40)                                      # 4:2:0, 5 x 3 MCUs, partial ones on both edges
    planes = np.zeros((fr.blocks, 64), np.int32)
    r = np.random.default_rng(50)
    planes[:, 0] = r.integers(-500, 500, fr.blocks)
    for z in range(1, 64):
        planes[:, ZIGZAG[z]] = r.integers(-6, 7, fr.blocks) * (r.integers(0, 64 + z, fr.blocks) < 24)
    Q = {0: q_ramp(1), 1: q_ramp(3)}
    DCT = [(0, 0, S.FLAT_DC)]

    def scripted(script, dris, **kw):
        """script: [(comps, ss, se, ah, al)]; dris: {scan number: DRI written in front of it}"""
        scans, dri = [], 0
        for i, (comps, ss, se, ah, al) in enumerate(script):
            dri = dris.get(i, dri)
            us = canonical(fr, planes, list(comps), ss, se, ah, al, dri)
            dht = list(DCT) if i == 0 else []
            if not (ss == 0 and ah):
                dht = dht + ([(1, 0, table_for(us, 8))] if ss else [])
            scans.append(Scan(list(comps), ss, se, ah, al, us, dht=dht, dri=dris.get(i), **(kw if i == len(script) - 1 else {})))
        return scans

    Y_FULL = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 63, 0, 1), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0, 1, 2), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    add("dri_changes_between_a_first_scan_and_its_refinement", "script", write(fr, Q, scripted(Y_FULL, {0: 4, 4: 7, 5: 5})), lined_up=False, dri_values=[4, 7, 5])
    add("dri_1_under_every_scan_kind", "script", write(fr, Q, scripted(Y_FULL, {0: 1})), dri_values=[1], kinds_with_intervals=4)
    add("dri_that_does_not_divide_the_unit_counts", "script", write(fr, Q, scripted(Y_FULL, {0: 7})), dri_values=[7])
    for i, kind in ((0, "dc_first"), (1, "ac_first"), (4, "dc_refinement"), (5, "ac_refinement")):
        scans = scripted(Y_FULL, {0: 5})
        scans[i].fill = {0: 3, 1: 1}
        add("fill_bytes_in_front_of_rst_%s" % kind, "script", write(fr, Q, scans), fill=(i, [3, 1]))
        scans = scripted(Y_FULL, {0: 5})
        scans[i].surplus = {0: b"\x55\xaa", 1: b"\x00"}
        add("surplus_octets_in_front_of_rst_%s_skipped_habit" % kind, "script", write(fr, Q, scans), wellformed=False, surplus=i)
    add("the_same_scans_twice", "script", write(fr, Q, scripted(Y_FULL[:2] + Y_FULL[:2] + Y_FULL[2:], {})), scans=8)
    add("a_component_no_scan_mentions", "script", write(fr, Q, scripted([((0, 1), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)], {})), unmentioned=2)
    FIVE = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 2, 0, 1), ((0,), 3, 5, 0, 1), ((0,), 6, 20, 0, 1), ((0,), 21, 40, 0, 1), ((0,), 41, 63, 0, 1), ((0,), 1, 63, 1, 0)]
    add("more_dependencies_than_an_item_has_slots", "script", write(fr, Q, scripted(FIVE, {})), deps_over=DEPS)
    scans = scripted(Y_FULL, {})
    scans[1].dht = scans[1].dht + [(0, 0, S.COMB_DC)]          # the DC table is defined again between the DC first scan and its refinement; DQT again too
    scans[2].dqt = {1: q_ramp(3)}
    add("dht_and_dqt_defined_again_between_the_scans", "script", write(fr, Q, scans), dht_between=True)
    for i, kind in ((1, "ac_first"), (5, "ac_refinement")):     # a stuffed 0xFF among the octets: "FF, then not RSTn" for the reference
        scans = scripted(Y_FULL, {0: 5})
        scans[i].surplus = {1: b"\x12\x34\x56\x78\x9a\xbc\xde\xff\x00\x21"}
        add("surplus_stuffed_ff_in_front_of_rst_%s_refused" % kind, "script", write(fr, Q, scans), "null", wellformed=False)
    # the last scan, a DC refinement of 90 bits, cut behind its first byte: ones follow (the EOI is no data)
    add("the_last_scan_cut_ones_follow_habit", "script", write(fr, Q, scripted(Y_FULL[:4] + [Y_FULL[5], Y_FULL[4]], {}), cut=1), wellformed=False, past_end=82)
    return out
