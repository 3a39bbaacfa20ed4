"""Hand-built baseline JPEG scans for the device entropy decoder (k_jpeg_unstuff, k_jpeg_entropy, k_jpeg_entropy_sync): a writer that takes
the SYMBOLS of every block, arbitrary DHT / DQT contents, sampling factors and a restart interval, and the named cases built with it.

Every stream the decoder had seen came from libjpeg: one family of Huffman tables and one symbol grammar.  The cases here stand on what
libjpeg never writes -- a code of every length 1 .. 16, second levels that do not fit the kernel's sub[] array, complete codes, unassigned bit
patterns, r/0 symbols, ZRL in front of EOB, DC predictors far outside int16, 0xFF in every data byte, segment lengths on the thresholds
between the kernels, streams a self-synchronising decoder never falls into step with.  cases() -> [(name, bytes, verdict)]:

    image       the reference decodes the file (T.81 defines it, or the reference has a habit the name says)
    null        the reference refuses it
    undefined   the reference has no defined result (the oracle returns -2, the library must not return OK)

corpus() returns the same with what a test needs to prove a name: the family, whether T.81 defines the stream (`wellformed`: the plain decoder
of tests/jpeg_scan_ref.py then gives the coefficients the writer put in), the coefficients the writer put in (`expect`) and the `claims` the
census has to confirm.  The kernels' geometry is read from the source (geometry()), so no case carries a literal of its own.

A block is a list of symbols; the first goes through the component's DC table, the rest through its AC table:
    (symbol, value)          the table's code word for `symbol`, then `symbol & 15` bits of `value` (T.81 F.1.2: negative values one less)
    ("cw", k, value)         code word number k of the table (table order) -- a symbol value two code words carry
    ("raw", bits, n)         n raw bits: a bit pattern no code word begins
"""
import os
import re

import numpy as np

import jpeg_scan_ref as R

ZIGZAG = R.ZIGZAG
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------------ geometry of the kernels
def geometry():
    """the numbers of gamut_amd/csrc/jpeg_entropy_kernels.hpp the cases are built around"""
    src = open(os.path.join(os.path.dirname(HERE), "gamut_amd", "csrc", "jpeg_entropy_kernels.hpp")).read()

    def one(pattern, what):
        m = re.search(pattern, src)
        assert m, "jpeg_entropy_kernels.hpp: %s not found" % what
        return m

    fast = int(one(r"uint16_t\s+fast\[(\d+)\];\s*// 9-bit lookahead", "the fast table").group(1))
    assert fast & (fast - 1) == 0
    threads = int(one(r"#define JPEG_SYNC_THREADS (\d+)", "JPEG_SYNC_THREADS").group(1))
    m = one(r"kLdsHuff = JPEG_SYNC_THREADS >= (\d+) \? (\d+) : (\d+)", "kLdsHuff")
    ut = one(r"kUnstuffThreads = (\d+), kUnstuffTile = kUnstuffThreads \* (\d+)", "kUnstuffTile")
    g = dict(fast_bits=fast.bit_length() - 1,
             sub_entries=int(one(r"#define JPEG_HUFF_SUB_ENTRIES (\d+)", "JPEG_HUFF_SUB_ENTRIES").group(1)),
             sync_min_bytes=int(one(r"kSyncMinBytes = (\d+);", "kSyncMinBytes").group(1)),
             sync_threads=threads,
             lane_min_bytes=int(one(r"const uint32_t sub = max\((\d+)u, \(\(len \+ kSyncThreads - 1\) / kSyncThreads \+ 3\) & ~3u\);", "the bytes per lane").group(1)),
             lds_huff=int(m.group(2)) if threads >= int(m.group(1)) else int(m.group(3)),
             unstuff_tile=int(ut.group(1)) * int(ut.group(2)))
    assert all(v > 0 for v in g.values())
    return g


def lane_bytes(length, g):
    """bytes per lane of k_jpeg_entropy_sync for a segment of `length` unstuffed bytes, and the lanes that work"""
    sub = max(g["lane_min_bytes"], (-(-length // g["sync_threads"]) + 3) & ~3)
    return sub, -(-length // sub)


# ------------------------------------------------------------------------------------------------------------------ tables
class Table:
    def __init__(self, bits, vals):
        assert len(bits) == 16 and sum(bits) == len(vals) <= 256
        self.bits, self.vals = list(bits), list(vals)
        self.h = R.Huff(bits, vals)
        self.codes = self.h.codes()
        self.enc = {}
        for code, ln, s in self.codes:
            self.enc.setdefault(s, (code, ln))
        self.kraft = sum(n << (16 - ln) for ln, n in enumerate(bits, 1))       # 65536: complete
        assert self.kraft <= 65536

    def payload(self, tc, th):
        return bytes([tc << 4 | th]) + bytes(self.bits) + bytes(self.vals)


def by_length(pairs):
    """[(length, symbol)] -> Table (canonical order: by length, then as listed)"""
    bits = [0] * 16
    pairs = sorted(pairs, key=lambda p: p[0])
    for ln, _ in pairs:
        bits[ln - 1] += 1
    return Table(bits, [s for _, s in pairs])


COMB_DC_SYMS = [2, 1, 3, 0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]                                     # length 1 .. 16
COMB_AC_SYMS = [0x01, 0x00, 0x02, 0x11, 0x03, 0xF0, 0x21, 0x04, 0x31, 0x05, 0x12, 0x41, 0x06, 0x51, 0x07, 0xE1]
COMB_DC = by_length(list(enumerate(COMB_DC_SYMS, 1)))         # one code of every length 1 .. 16; lengths 10 .. 16 share the prefix of nine 1-bits: x = 7
COMB_AC = by_length(list(enumerate(COMB_AC_SYMS, 1)))
FLAT_DC = by_length([(5, s) for s in range(16)])              # every category a 5-bit code
FLAT_AC = by_length([(8, s) for s in range(255)])             # every symbol 0x00 .. 0xFE an 8-bit code
# every symbol + value one byte: the symbol of size s has a code of 8 - s bits (s = 1 .. 7); FE and FF are the two 8-bit codes
BYTE_DC = by_length([(8 - s, s) for s in range(1, 8)] + [(8, 0), (8, 8)])
BYTE_AC = by_length([(8 - s, s) for s in range(1, 8)] + [(8, 0x00), (8, 0xF0)])      # complete: FE = EOB, FF = ZRL
# the phase-locked streams: DC and AC table identical, all-ones unassigned
PHASE = by_length([(8 - s, s) for s in range(0, 8)])

Q1 = [1] * 64


def q_ramp(a, b=1):
    return [a + b * i for i in range(64)]


# ------------------------------------------------------------------------------------------------------------------ the writer
class Bits:
    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0; self.total = 0

    def put(self, value, nbits):
        if not nbits:
            return
        self.total += nbits
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1)); self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self, ones=True):
        if self.n:
            k = 8 - self.n
            self.put((1 << k) - 1 if ones else 0, k)
            self.total -= k


def _value_bits(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def _put_block(bw, block, dc, ac):
    for i, item in enumerate(block):
        t = dc if i == 0 else ac
        if item[0] == "raw":
            bw.put(item[1], item[2]); continue
        if item[0] == "cw":
            code, ln, s = t.codes[item[1]]; v = item[2]
        else:
            s, v = item; code, ln = t.enc[s]
        bw.put(code, ln)
        if s & 15:
            assert abs(int(v)).bit_length() == s & 15, (item, "the value does not have the size the symbol says")
            bw.put(_value_bits(int(v), s & 15), s & 15)


def block_bits(block, dc, ac):
    bw = Bits(); _put_block(bw, block, dc, ac)
    return bw.total


def _i16(x):
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def _model_block(block, dc, ac, pred, q, out):
    """what T.81 makes of the symbols: -> (new predictor, True) or (.., False) when the standard does not define the block"""
    def sym_of(item, t):
        return t.codes[item[1]][2] if item[0] == "cw" else item[0]
    if any(it[0] == "raw" for it in block):
        return pred, False
    s = sym_of(block[0], dc)
    if s > 15:
        return pred, False
    pred += int(block[0][-1]) if s else 0
    out[0] = _i16(pred * q[0])
    k = 1
    ended = False
    for it in block[1:]:
        if ended or k > 63:
            return pred, False
        rs = sym_of(it, ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                if k + 16 > 64:
                    return pred, False
                k += 16; continue
            if r:
                return pred, False
            ended = True; continue
        k += r
        if k > 63:
            return pred, False
        out[ZIGZAG[k]] = _i16(int(it[-1]) * q[k]); k += 1
    return pred, ended or k == 64


def write(width, height, comps, dqt, dht, mcus=None, dri=0, pad_ones=True, fill=None, scans=None, one_dht_segment=False, dqt16=(), cut=None,
          sof_size=None):
    """comps: [(id, h, v, tq, td, ta)]; dqt: {id: 64 values, zig-zag order}; dht: [(class, id, Table)] in the order they are written (a table
    written twice: the last one counts); mcus: the units of the one interleaved scan, each a list of blocks; scans: [(component indices, units)]
    instead, for more than one scan; fill: {interval: 0xFF bytes in front of the RSTn that ends it}; cut: keep that many bytes of the (last)
    scan; sof_size: the (width, height) SOF0 declares when it is not the size the blocks were made for.
    -> (bytes, expect): expect = the de-quantised int16 coefficients (blocks in MCU order, natural order) or None where T.81 does not define them"""
    fill = fill or {}
    out = bytearray(b"\xff\xd8")
    for tq in sorted(dqt):
        wide = tq in dqt16 or max(dqt[tq]) > 255
        body = b"".join(int(v).to_bytes(2, "big") for v in dqt[tq]) if wide else bytes(dqt[tq])
        out += b"\xff\xdb" + (3 + len(body)).to_bytes(2, "big") + bytes([(16 if wide else 0) | tq]) + body
    sw, sh = sof_size or (width, height)
    out += b"\xff\xc0" + (8 + 3 * len(comps)).to_bytes(2, "big") + bytes([8]) + sh.to_bytes(2, "big") + sw.to_bytes(2, "big") + bytes([len(comps)])
    for cid, h, v, tq, td, ta in comps:
        out += bytes([cid, h << 4 | v, tq])
    if one_dht_segment:
        body = b"".join(t.payload(tc, th) for tc, th, t in dht)
        out += b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body
    else:
        for tc, th, t in dht:
            body = t.payload(tc, th)
            out += b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body
    if dri:
        out += b"\xff\xdd\x00\x04" + int(dri).to_bytes(2, "big")
    tab = {}
    for tc, th, t in dht:
        tab[(tc, th)] = t
    nc = len(comps)
    hs = [1 if nc == 1 else c[1] for c in comps]; vs = [1 if nc == 1 else c[2] for c in comps]
    hmax, vmax = max(hs), max(vs)
    mpr, mpc = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    off, nb = [], 0
    for c in range(nc):
        off.append(nb); nb += hs[c] * vs[c]
    expect = np.zeros((mpr * mpc * nb, 64), np.int16)
    defined = True
    if scans is None:
        scans = [(list(range(nc)), mcus)]
    for sel, units in scans:
        if len(sel) == 1:
            c = sel[0]
            nbx = -(-(-(-width * hs[c] // hmax)) // 8); nby = -(-(-(-height * vs[c] // vmax)) // 8)
            assert len(units) == nbx * nby

            def blocks_of(u, c=c, nbx=nbx):
                by, bx = divmod(u, nbx)
                return [(c, ((by // vs[c]) * mpr + bx // hs[c]) * nb + off[c] + (by % vs[c]) * hs[c] + bx % hs[c])]
        else:
            assert len(units) == mpr * mpc, (len(units), mpr * mpc)
            order = [(c, off[c] + b) for c in sel for b in range(hs[c] * vs[c])]

            def blocks_of(u, order=order):
                return [(c, u * nb + o) for c, o in order]
        out += b"\xff\xda" + (6 + 2 * len(sel)).to_bytes(2, "big") + bytes([len(sel)])
        for c in sel:
            out += bytes([comps[c][0], comps[c][4] << 4 | comps[c][5]])
        out += bytes([0, 63, 0])
        scan_at = len(out)
        bw = Bits()
        pred = {c: 0 for c in sel}
        interval = 0
        for u, unit in enumerate(units):
            if dri and u and u % dri == 0:
                bw.flush(pad_ones)
                out += bw.out + b"\xff" * fill.get(interval, 0) + bytes([0xFF, 0xD0 + (interval & 7)])
                bw = Bits(); pred = {c: 0 for c in sel}; interval += 1
            where = blocks_of(u)
            assert len(unit) == len(where), (u, len(unit), len(where))
            for block, (c, at) in zip(unit, where):
                dc, ac = tab[(0, comps[c][4])], tab[(1, comps[c][5])]
                _put_block(bw, block, dc, ac)
                pred[c], ok = _model_block(block, dc, ac, pred[c], dqt[comps[c][3]], expect[at])
                defined = defined and ok
        bw.flush(pad_ones)
        out += bw.out
        if cut is not None:
            del out[scan_at + cut:]
            defined = False
    out += b"\xff\xd9"
    return bytes(out), (expect if defined else None)


def coded(dc_diff, ac=None, eob=True):
    """the symbols an encoder writes for a block: DC difference, {zig-zag index: value}"""
    ac = ac or {}
    out = [(abs(int(dc_diff)).bit_length(), int(dc_diff))]
    k = 1
    for z in sorted(ac):
        v = int(ac[z])
        if not v:
            continue
        r = z - k
        while r > 15:
            out.append((0xF0, 0)); r -= 16
        out.append((r << 4 | abs(v).bit_length(), v)); k = z + 1
    if k < 64 and eob:
        out.append((0x00, 0))
    return out


# ------------------------------------------------------------------------------------------------------------------ case plumbing
class Case:
    def __init__(self, name, family, data, verdict, expect, wellformed, claims):
        self.name, self.family, self.data, self.verdict, self.expect, self.wellformed, self.claims = name, family, data, verdict, expect, wellformed, claims


GREY = [(1, 1, 1, 0, 0, 0)]
MODES = {0: GREY,
         1: [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)],
         2: [(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)],
         3: [(1, 1, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)],
         4: [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]}
NB = {0: 1, 1: 3, 2: 4, 3: 4, 4: 6}
MCU_W = {0: 8, 1: 8, 2: 16, 3: 8, 4: 16}
MCU_H = {0: 8, 1: 8, 2: 8, 3: 16, 4: 16}


def n_mcus(mode, w, h):
    return -(-w // MCU_W[mode]) * -(-h // MCU_H[mode])


def comb_block(rng, dense=False):
    """a block over the comb tables that uses whatever symbols fit: DC category 0 .. 11 (12 .. 15 only where a case asks), AC symbols at random"""
    cat = int(rng.integers(0, 12))
    d = 0 if not cat else int(rng.integers(1 << (cat - 1), 1 << cat)) * (1 if rng.integers(2) else -1)
    blk = [(cat, d)]
    k = 1
    n = int(rng.integers(20, 40)) if dense else int(rng.integers(0, 12))
    for _ in range(n):
        rs = COMB_AC_SYMS[int(rng.integers(0, 16))]
        r, s = rs >> 4, rs & 15
        if rs == 0x00:
            continue
        if rs == 0xF0:
            if k + 16 > 63:
                continue
            blk.append((rs, 0)); k += 16; continue
        if k + r > 63:
            continue
        v = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.integers(2) else -1)
        blk.append((rs, v)); k += r + 1
        if k > 63:
            break
    if k < 64:
        blk.append((0x00, 0))
    return blk


def all_comb_symbols_block():
    """every AC symbol of the comb once (so every code length 1 .. 16), then EOB"""
    blk = [(0, 0)]                                             # the DC symbol: the caller's
    for rs in COMB_AC_SYMS:
        if rs in (0x00,):
            continue
        s = rs & 15
        blk.append((rs, (1 << s) - 1 if s else 0))
    blk.append((0x00, 0))
    k = 1
    for rs, _ in blk[1:-1]:
        k += 16 if rs == 0xF0 else (rs >> 4) + 1
    assert k <= 64
    return blk


def fit_segment(dc, ac, n_blocks, target, rng, first_blocks=None):
    """n_blocks grey blocks over (dc, ac) -- tables that hold (0, s) symbols for s = 1 .. 10 and EOB -- whose scan is EXACTLY `target` unstuffed
    bytes: coefficients are added block by block, and the last block is adjusted until the length is hit"""
    blocks = [list(b) for b in (first_blocks or [])]
    while len(blocks) < n_blocks:
        blocks.append(None)
    top = 8 * target                                           # the scan's bits have to end in [top - 7, top]: the padding fills the byte
    used = sum(block_bits(b, dc, ac) for b in blocks if b is not None)
    todo = [i for i, b in enumerate(blocks) if b is None]
    cost = {s: block_bits([(1, 1), (s, 1 << (s - 1))], dc, ac) - block_bits([(1, 1)], dc, ac) for s in range(1, 11)}
    for n, i in enumerate(todo):
        left = len(todo) - n
        blk = [(1, 1 if rng.integers(2) else -1)]
        bits = block_bits(blk + [(0x00, 0)], dc, ac)
        share = (top - used) // left
        k = 1
        while k < 63:
            if left > 1:
                s = int(rng.integers(1, 11))
                if bits + cost[s] > share:
                    break
            else:                                              # the last block: land on the target
                rest = top - used - bits
                if rest <= 7:
                    break
                ends = [t for t in cost if 0 <= rest - cost[t] <= 7]
                goes = [t for t in cost if rest - cost[t] >= min(cost.values()) + 8]
                assert ends or goes, rest
                s = int(rng.choice(ends if ends else goes))
            v = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.integers(2) else -1)
            blk.append((s, v)); bits += cost[s]; k += 1
        if k < 64:
            blk.append((0x00, 0))
        blocks[i] = blk
        used += block_bits(blk, dc, ac)
    assert -(-used // 8) == target, (used, target)
    return blocks


def grey_dims(n):
    """(width, height) of a grey image of exactly n blocks"""
    for rows in range(int(n ** 0.5), 0, -1):
        if n % rows == 0:
            return 8 * (n // rows), 8 * rows


STD_DHT = [(0, 0, FLAT_DC), (1, 0, FLAT_AC)]
COMB_DHT = [(0, 0, COMB_DC), (1, 0, COMB_AC), (0, 1, COMB_DC), (1, 1, COMB_AC)]
_made = None


def corpus():
    global _made
    if _made is None:
        _made = _build()
    return _made


def cases():
    return [(c.name, c.data, c.verdict) for c in corpus()]


def _build():
    g = geometry()
    FB, SUB, SMIN, LANES, LMIN, TILE = g["fast_bits"], g["sub_entries"], g["sync_min_bytes"], g["sync_threads"], g["lane_min_bytes"], g["unstuff_tile"]
    out = []
    names = set()

    def add(name, family, made, verdict="image", wellformed=True, **claims):
        data, expect = made
        assert name not in names
        names.add(name)
        if wellformed:
            assert expect is not None, name
        out.append(Case(name, family, data, verdict, expect if wellformed else None, wellformed, claims))

    def grey(blocks, dht=STD_DHT, q=Q1, **kw):
        w, h = grey_dims(len(blocks))
        return write(w, h, GREY, {0: q}, dht, [[b] for b in blocks], **kw)

    # ---- table shapes -------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1)
    blocks = []
    for cat in range(16):                                      # every DC length (categories 12 .. 15 included) and every AC length in the scan
        b = all_comb_symbols_block()
        d = 0 if not cat else (1 << cat) - 1 - (cat if cat > 3 else 0)
        b[0] = (cat, d if cat % 2 else -d)
        blocks.append(b)
    add("comb_every_length_1_to_16_dc_and_ac", "tables", grey(blocks, COMB_DHT[:2], q_ramp(1)), lengths={(0, 0): range(1, 17), (1, 0): range(1, 17)},
        deepest_level=(1, 0))

    deep = Table([0] * 7 + [100] + [0] * 7 + [100], list(range(1, 11)) + list(range(0x11, 0x6B)) + list(range(0x6B, 0xCF)))
    assert deep.enc[0x01][1] == 8 and all(ln == 16 for _, ln, s in deep.codes[100:])
    longs = [s for _, ln, s in deep.codes if ln == 16 and 1 <= (s & 15) <= 10]
    blocks = []
    for i in range(16):
        blk = [(3, 5 - i % 2)]
        k = 1
        for j in range(6):
            rs = longs[(7 * i + j) % len(longs)]
            if k + (rs >> 4) > 63:
                break
            blk.append((rs, (1 << ((rs & 15) - 1)) | (j & ((1 << ((rs & 15) - 1)) - 1)))); k += (rs >> 4) + 1
        # (no EOB in this table: every block runs to coefficient 63)
        while k < 64:
            blk.append((0x01, 1 if k % 2 else -1)); k += 1
        blocks.append(blk)
    add("one_prefix_hundred_16_bit_codes_second_level_x7", "tables", grey(blocks, [(0, 0, FLAT_DC), (1, 0, deep)], q_ramp(2)),
        lengths={(1, 0): [8, 16]}, sub_need_is={(1, 0): 1 << (16 - FB)})

    # eight 9-bit prefixes behind the short codes, the codes below them 10, 11, ... 15, 16 and 16 bits long (a DHT assigns code words in order of
    # length, so each prefix is filled by ONE length): 2 + 4 + ... + 64 + 128 + 128 second-level entries, more than sub[] holds -- the last prefix
    # is left to the canonical search.  The reference cannot take that table: make_huff_table's bit tree has 512 slots and this code needs 516
    # (it writes behind the array: no defined result), and it refuses a DHT of more than 255 code words -- so the case as first described
    # is `undefined`, and its neighbour with 15-bit codes under the seventh prefix (2 + 4 + ... + 64 + 64 + 128 = 318 entries, 388 slots) is the image.
    def prefixes_table(counts):
        vals, pool = [], [v for v in range(256) if v not in (0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x11, 0x12, 0x21, 0x22, 0x31, 0xF0)]
        plan = {10: [0x00, 0x01], 11: [0x02, 0x11], 12: [0x03, 0x12], 13: [0x04, 0x21], 14: [0x05, 0x22], 15: [0x06, 0x31, 0xF0], 16: []}
        for ln in range(10, 17):                              # useful symbols among every length, EOB among the 10-bit codes
            n = counts[ln - 1]
            vals += plan[ln][:n] + [pool.pop() for _ in range(n - len(plan[ln][:n]))]
        vals[-1] = 0x07                                       # the last code word, alone under the eighth prefix
        t = Table(counts, vals)
        fit, left = R.sub_fit(t.bits, SUB)
        assert len(fit) == 7 and len(left) == 1
        in_last = [sym for code, ln, sym in t.codes if (code >> (ln - FB)) == left[0]]
        assert len(in_last) == 1 and in_last[0] & 15 and in_last[0] >> 4 == 0
        return t, in_last[0]

    for name, counts, verdict, n in (("eight_prefixes_lengths_10_to_15_15_16_second_levels_overflow_sub", [0] * 9 + [2, 4, 8, 16, 32, 128, 1], "image", 12),
                                     ("eight_prefixes_lengths_10_to_15_15_16_second_levels_overflow_sub_many_lanes", [0] * 9 + [2, 4, 8, 16, 32, 128, 1], "image", 192),
                                     ("eight_prefixes_lengths_10_to_16_16_no_defined_result_bit_tree_of_the_reference_overflows", [0] * 9 + [2, 4, 8, 16, 32, 64, 129], "undefined", 12)):
        eight, last_sym = prefixes_table(counts)
        blocks = []
        for i in range(n):
            blk = [(2, 2 + i % 2)]
            k = 1
            for rs in (0x01, 0x02, 0x11, 0x03, 0x12, 0x04, 0x21, 0x05, 0x22, 0x06, 0x31, 0xF0, last_sym, 0x01, last_sym):
                r, sz = rs >> 4, rs & 15
                if rs == 0xF0:
                    if rs in eight.enc:
                        blk.append((rs, 0)); k += 16
                    continue
                blk.append((rs, (1 << (sz - 1)) | (i & ((1 << (sz - 1)) - 1)))); k += r + 1
            blk.append((0x00, 0))
            blocks.append(blk)
        add(name, "tables", grey(blocks, [(0, 0, FLAT_DC), (1, 0, eight)], q_ramp(3)), verdict,
            lengths={(1, 0): [ln for ln in range(10, 17) if counts[ln - 1]]}, sub_need_over={(1, 0): SUB}, prefixes_fit_and_left=(1, 0),
            **({"segment_at_least": SMIN} if n > 100 else {}))

    one_dc, one_ac = Table([1] + [0] * 15, [3]), Table([1] + [0] * 15, [0x00])
    add("tables_of_a_single_code", "tables", grey([[(3, (-1) ** i * (4 + i % 4)), (0x00, 0)] for i in range(24)], [(0, 0, one_dc), (1, 0, one_ac)], q_ramp(5)),
        lengths={(0, 0): [1], (1, 0): [1]})
    only16_dc, only16_ac = Table([0] * 15 + [12], list(range(12))), Table([0] * 15 + [40], [0x00, 0xF0] + list(range(1, 11)) + list(range(0x11, 0x1B)) + list(range(0x21, 0x2B)) + list(range(0x31, 0x39)))
    rng = np.random.default_rng(2)
    blocks = []
    for i in range(16):
        blk = coded(int(rng.integers(-2000, 2000)))[:1]
        k = 1
        for _ in range(int(rng.integers(0, 14))):
            rs = only16_ac.vals[int(rng.integers(1, 40))]
            if rs == 0xF0:
                if k + 16 <= 63:
                    blk.append((rs, 0)); k += 16
                continue
            if k + (rs >> 4) > 63:
                break
            blk.append((rs, int(rng.integers(1 << ((rs & 15) - 1), 1 << (rs & 15))) * (-1) ** k)); k += (rs >> 4) + 1
        blocks.append(blk + ([(0x00, 0)] if k < 64 else []))
    add("tables_of_only_16_bit_codes", "tables", grey(blocks, [(0, 0, only16_dc), (1, 0, only16_ac)], q_ramp(1, 2)), lengths={(0, 0): [16], (1, 0): [16]})

    # complete codes: Kraft sum 1, the all-ones word assigned
    full_dc = by_length([(ln, s) for ln, s in zip(list(range(1, 15)) + [15, 15], [1, 2, 0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])])
    full_ac = by_length(list(enumerate(COMB_AC_SYMS, 1)) + [(16, 0x61)])
    assert full_dc.kraft == 65536 and full_ac.kraft == 65536 and full_ac.enc[0x61] == (0xFFFF, 16) and full_dc.enc[15] == (0x7FFF, 15)
    FULL_DHT = [(0, 0, full_dc), (1, 0, full_ac)]

    def full_blocks(n, seed, dense=False):
        r = np.random.default_rng(seed)
        res = []
        for i in range(n):
            b = comb_block(r, dense)
            if i % 3 == 0 and len(b) > 2:
                b.insert(1, (0x61, -1 if i % 2 else 1))                        # the all-ones code word
            if i % 5 == 0:
                b[0] = (15, -(1 << 14) - i)                     # the all-ones DC code word
            k = 1
            ok = []
            for it in b[1:]:
                rs = it[0]
                if rs == 0x00:
                    break
                step = 16 if rs == 0xF0 else (rs >> 4) + 1
                if k + step > 64 or (rs != 0xF0 and k + (rs >> 4) > 63):
                    continue
                ok.append(it); k += step
            res.append([b[0]] + ok + ([(0x00, 0)] if k < 64 else []))
        return res
    add("complete_code_whole_scan", "tables", grey(full_blocks(16, 3), FULL_DHT, q_ramp(1)), complete=[(0, 0), (1, 0)], all_ones_used=True)
    few = full_blocks(40, 4)
    w = write(40 * 8, 8, GREY, {0: q_ramp(1)}, FULL_DHT, [[b] for b in few], sof_size=(256, 256))
    add("complete_code_truncated_scan_under_256x256", "tables", w, wellformed=False, complete=[(0, 0), (1, 0)], scan_below=SMIN)
    n = 160
    while True:
        many = full_blocks(n, 5, dense=True)
        made = grey(many, FULL_DHT, q_ramp(1))
        if len(made[0]) - made[0].index(b"\xff\xda") - 10 - made[0].count(b"\xff\x00") >= SMIN + 64:
            break
        n += 16
    add("complete_code_long_scan_many_lanes", "tables", made, complete=[(0, 0), (1, 0)], all_ones_used=True, segment_at_least=SMIN)
    w = write(n * 8, 8, GREY, {0: q_ramp(1)}, FULL_DHT, [[b] for b in many], sof_size=(1024, 1024))
    add("complete_code_long_truncated_scan_under_1024x1024", "tables", w, wellformed=False, complete=[(0, 0), (1, 0)], scan_at_least=SMIN)

    # an incomplete code and windows no code word covers: (a) no code word shares the first 8 bits -- no bits taken, symbol 0: the AC table's
    # codes all begin with 0 or 10, the block simply stops and the next DC code (110...) is read from the same bits; (b) a subtree that runs
    # out: sixteen 1-bits under the comb, whose longest code is fifteen 1-bits and a 0 -- 16 bits taken, symbol 0
    short_ac = by_length([(2, 0x01), (2, 0x02), (3, 0x00), (3, 0x03)])          # 00, 01, 100, 101: 11x is unassigned, and no code word begins with it
    dc_11 = by_length([(2, 1), (2, 2), (2, 3), (3, 4)])                         # 00, 01, 10, 110: category 4 begins with the 11 that ends an AC run
    blocks = []
    for i in range(16):
        blk = [(4, 9 + i % 7 if i % 2 else -9 - i % 7), (0x01, 1), (0x03, -5), (0x02, 3)]
        if i % 4 == 3 or i == 15:
            blk.append((0x00, 0))                              # a real EOB now and then (and at the end: the padding is 1-bits as well)
        blocks.append(blk)                                     # otherwise the block ends where the next DC code, 110, begins
    add("unassigned_window_no_bits_taken_symbol_0", "tables", grey(blocks, [(0, 0, dc_11), (1, 0, short_ac)], q_ramp(2)), wellformed=False)
    blocks = []
    for i in range(16):
        blk = comb_block(np.random.default_rng(60 + i))
        if i % 2:
            blk = blk[:-1] if blk[-1][0] == 0x00 else blk
            k = 1
            for rs, _ in blk[1:]:
                k += 16 if rs == 0xF0 else (rs >> 4) + 1
            if k < 64:
                blk.append(("raw", 0xFFFF, 16))                # sixteen 1-bits: the subtree of the long codes runs out at 16 bits
        blocks.append(blk)
    add("unassigned_window_subtree_runs_out_16_bits_taken", "tables", grey(blocks, COMB_DHT[:2], q_ramp(2)), wellformed=False)

    twice = by_length([(2, 0x01), (3, 0x00), (4, 0x02), (4, 0x01), (5, 0x03), (11, 0x02), (12, 0xF0)])
    dup = {s: [i for i, c in enumerate(twice.codes) if c[2] == s] for s in (0x01, 0x02)}
    blocks = []
    for i in range(16):
        blk = [(3, 4 + i % 4)]
        for j in range(10):
            s = (0x01, 0x02)[(i + j) % 2]
            blk.append(("cw", dup[s][(i + j // 2) % 2], (1 << (s - 1)) * (1 if j % 3 else -1)))
        blk.append((0x00, 0))
        blocks.append(blk)
    add("symbol_value_carried_by_two_code_words", "tables", grey(blocks, [(0, 0, FLAT_DC), (1, 0, twice)], q_ramp(1)), lengths={(1, 0): [2, 4, 11]})

    rng = np.random.default_rng(6)
    ids_a = [(1, 1, 1, 0, 3, 1), (2, 1, 1, 1, 2, 2), (3, 1, 1, 2, 1, 3)]
    dht4 = [(0, 0, FLAT_DC), (0, 1, COMB_DC), (0, 2, full_dc), (0, 3, only16_dc), (1, 0, FLAT_AC), (1, 1, COMB_AC), (1, 2, full_ac), (1, 3, COMB_AC)]
    mcus = [[comb_block(rng), comb_block(rng), comb_block(rng)] for _ in range(6)]
    for m in mcus:
        m[0][0] = (3, 5)                                       # (0, 3): the 16-bit-only DC table holds categories 0 .. 11
    add("table_ids_dc_3_2_1_ac_1_2_3", "tables", write(24, 16, ids_a, {0: q_ramp(1), 1: q_ramp(2), 2: q_ramp(3)}, dht4, mcus), tables_used=[(0, 3), (0, 2), (0, 1), (1, 1), (1, 2), (1, 3)])
    add("table_ids_dc_0_ac_0_one_dht_segment_of_eight_tables", "tables",
        write(24, 16, GREY, {0: q_ramp(1)}, dht4, [[comb_block(rng)[:1] + coded(0, {1: 3, 17: -200, 63: 1})[1:]] for _ in range(6)], one_dht_segment=True),
        tables_used=[(0, 0), (1, 0)], dht_segment_of=8)
    junk = Table([0] * 7 + [3] + [0] * 8, [9, 10, 11])
    add("table_defined_twice_last_wins", "tables", grey([comb_block(rng) for _ in range(8)], [(0, 0, junk), (1, 0, junk), (0, 0, COMB_DC), (1, 0, COMB_AC)], q_ramp(1)),
        defined_twice=[(0, 0), (1, 0)])

    q16 = [40000, 32768, 16384, 8192, 300, 0, 65535, 256] * 8
    blocks = [coded(d, {1: 2, 2: 4, 3: -8, 4: 123, 5: 77, 6: -3, 7: 128, 8: 1, 9: 3, 13: 9, 14: -1, 15: 255}) for d in (1, 1, 2, -5, 1000, -2000, 7, 1)]
    add("dqt_16_bit_values_products_wrap_int16_and_quantiser_0", "tables", grey(blocks, q=q16), dqt_precision={0: 1}, zero_products=True)

    # ---- symbol grammar -----------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(7)

    def around(special, n=8):
        """the special block between good neighbours"""
        blocks = [coded(int(rng.integers(-50, 50)), {int(z): int(rng.integers(1, 30)) for z in rng.choice(np.arange(1, 64), 5, replace=False)}) for _ in range(n)]
        blocks[n // 2] = special
        return blocks

    add("block_of_63_coded_ac_no_eob", "grammar", grey(around(coded(5, {z: (z % 7 + 1) * (-1) ** z for z in range(1, 64)}))), symbols={"full": 1})
    b63 = coded(-3, {63: 9})
    assert [s for s, _ in b63[1:]] == [0xF0, 0xF0, 0xF0, 0xE4]
    add("only_coefficient_63_zrl_x3_then_run_14", "grammar", grey(around(b63)), symbols={"zrl": 3, "full": 1})
    add("zrl_then_eob_max_zag_is_where_eob_was_read", "grammar", grey(around([(2, 3), (0x01, 1), (0xF0, 0), (0x00, 0)])), symbols={"zrl": 1}, max_zag=(4, 18))
    add("zrl_x3_then_eob", "grammar", grey(around([(0, 0), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0x00, 0)])), symbols={"zrl": 3}, max_zag=(4, 49))
    for r in (1, 7, 14):
        add("symbol_%d_0_ends_the_block_like_eob" % r, "grammar", grey(around([(2, -2), (0x02, 3), (0x11, -1), (r << 4, 0)])), wellformed=False)
    add("ac_sizes_11_to_15", "grammar", grey(around([(1, 1)] + [(s, ((1 << s) - 1 - s) * (-1) ** s) for s in range(11, 16)] + [(0x2B, 1024), (0x00, 0)]), q=q_ramp(1)),
        symbols={("ac", 11): 2, ("ac", 15): 1})
    add("ac_sizes_11_to_15_products_wrap", "grammar", grey(around([(1, 1)] + [(s, ((1 << s) - 1) * (-1) ** s) for s in range(11, 16)] + [(0x00, 0)]), q=q_ramp(3, 7)))
    add("dc_categories_12_to_15", "grammar", grey([[(12 + i % 4, ((1 << (12 + i % 4)) - 1 - i) * (-1) ** (i // 4)), (0x00, 0)] for i in range(16)], q=q_ramp(1)),
        symbols={("dc", 12): 4, ("dc", 15): 4}, dc_wraps=True)
    add("dc_categories_12_to_15_quantiser_17", "grammar", grey([[(12 + i % 4, ((1 << (12 + i % 4)) - 1 - i) * (-1) ** (i // 5)), (0x03, 5), (0x00, 0)] for i in range(16)], q=q_ramp(17)))
    add("run_lands_exactly_on_63", "grammar", grey(around([(3, 4), (0x01, 1), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0xD2, -3)])), symbols={"full": 1})
    add("run_lands_exactly_on_63_from_48", "grammar", grey(around(coded(1, {47: 2, 63: 2}))), symbols={"full": 1})
    bad_run = [(3, 4), (0x01, 1), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0xF2, -3)]
    bad_zrl = [(3, 4), (0x01, 1), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0x00, 0)]
    add("run_past_63_alone", "grammar", grey([bad_run]), "null", wellformed=False)
    add("run_past_63_between_good_neighbours", "grammar", grey(around(bad_run)), "null", wellformed=False)
    add("zrl_past_64_alone", "grammar", grey([bad_zrl]), "null", wellformed=False)
    add("zrl_past_64_between_good_neighbours", "grammar", grey(around(bad_zrl)), "null", wellformed=False)
    add("zrl_lands_exactly_on_64", "grammar", grey(around([(3, 4)] + [(0x01, 1)] * 15 + [(0xF0, 0)] * 3)), symbols={"zrl": 3, "full": 1}, max_zag=(4, 64))
    dc17 = by_length([(5, s) for s in range(16)] + [(6, 17)])
    add("dc_symbol_above_15", "grammar", grey(around([(17, 1), (0x00, 0)]), [(0, 0, dc17), (1, 0, FLAT_AC)]), "undefined", wellformed=False)

    # DC differences of +-2047 until the predictor has left int16 dozens of times, in a scan long enough for the many-lane kernel: the lanes' DC sums
    # and the 16-bit copies in the checkpoints wrap
    n = 2048
    blocks = []
    for i in range(n):
        up = (i // 300) % 3 != 2
        blk = [(11, 2047 if up else -2047)]
        if i % 3 == 0:
            blk.append((0x01, 1 if i % 2 else -1))
        blk.append((0x00, 0))
        blocks.append(blk)
    add("dc_differences_2047_predictor_passes_2_16_many_lanes", "grammar", grey(blocks, q=q_ramp(3)), dc_wraps=True, segment_at_least=SMIN)
    add("dc_differences_2047_comb_tables_4_4_4", "grammar",
        write(8 * 32, 8 * 20, MODES[1], {0: q_ramp(1), 1: q_ramp(5)}, COMB_DHT,
              [[[(11, 2047 if (i // 100) % 2 == 0 else -2047), (0x01, 1), (0x00, 0)], [(11, -2047), (0x00, 0)], [(11, 2047 if i % 7 else -2047), (0x11, -1), (0x00, 0)]] for i in range(640)]),
        dc_wraps=True, segment_at_least=SMIN)

    # products that are 0: the token hand-off writes a token for every coded coefficient, the dense hand-off a zero
    qz = [2, 0, 3, 0, 32768, 16384, 1, 0] * 8
    rng = np.random.default_rng(8)
    mcus = []
    for i in range(16 * 6):
        ac = {int(z): int(rng.integers(1, 9)) * 2 for z in rng.choice(np.arange(1, 64), 30, replace=False)}
        mcus.append(coded(int(rng.integers(-6, 6)) * 2, ac))
    mcus = [mcus[6 * k:6 * k + 6] for k in range(16)]
    add("products_that_wrap_to_0_4_2_0_long_scan", "grammar", write(64, 64, MODES[4], {0: qz, 1: qz[1:] + [4]}, STD_DHT + [(0, 1, FLAT_DC), (1, 1, FLAT_AC)], mcus),
        zero_products=True, segment_at_least=SMIN)

    # ---- bytes and lengths --------------------------------------------------------------------------------------------------------------
    BYTE_DHT = [(0, 0, BYTE_DC), (1, 0, BYTE_AC)]
    # every data byte 0xFF: complete tables whose all-ones code words carry values -- category 8 and the symbol (0, 8), each followed by eight
    # 1-bits (+255) -- and blocks of 63 coded coefficients, so no EOB breaks the run: half the raw scan is stuffing
    ff_dc = by_length([(1, 0)] + [(ln, ln - 1) for ln in range(2, 8)] + [(8, 7), (8, 8)])           # 11111111 -> category 8, value 11111111 = +255
    ff_ac = by_length([(1, 0x00)] + [(ln, ln - 1) for ln in range(2, 8)] + [(8, 0x07), (8, 0x08)])   # 11111111 -> (0, 8), value 11111111 = +255
    assert ff_dc.enc[8] == (0xFF, 8) and ff_ac.enc[0x08] == (0xFF, 8) and ff_dc.kraft == 65536
    blocks = [[(8, 255)] + [(0x08, 255)] * 63 for _ in range(12)]
    made = grey(blocks, [(0, 0, ff_dc), (1, 0, ff_ac)], q_ramp(1))
    add("every_data_byte_ff", "bytes", made, stuffed_is=12 * 128, segment_is=[12 * 128])
    blocks = [[(8, 255)] + [(0x08, 255)] * 63 for _ in range(40)]
    add("every_data_byte_ff_many_lanes", "bytes", grey(blocks, [(0, 0, ff_dc), (1, 0, ff_ac)], q_ramp(1)), stuffed_is=40 * 128, segment_is=[40 * 128])

    def byte_stream(n_blocks, targets, seed, block_len=22):
        """grey blocks over the byte tables (every symbol one byte) with a ZRL -- the byte FF -- wherever a raw offset of `targets` falls"""
        r = np.random.default_rng(seed)
        raw = 0
        blocks, hit = [], set()
        for _ in range(n_blocks):
            L = block_len
            for t in targets:
                if t - raw in (L - 1, L, L + 1):
                    L += 3
            blk = []
            zrls = 0
            for i in range(L):
                if i == L - 1:
                    blk.append((0x00, 0)); raw += 1; continue
                if i and raw in targets and zrls < 2:
                    blk.append((0xF0, 0)); raw += 2; zrls += 1; hit.add(raw - 2); continue
                s = int(r.integers(1, 8))
                v = int(r.integers(1 << (s - 1), 1 << s)) * (1 if r.integers(2) else -1)
                blk.append((s, v)); raw += 1
            blocks.append(blk)
        assert hit == set(targets), (hit, targets)
        return blocks

    blocks = byte_stream(384, [TILE - 1, 2 * TILE - 1], 9)
    add("ff_last_byte_of_a_tile_its_00_first_of_the_next", "bytes", grey(blocks, BYTE_DHT), stuffed_at=[TILE - 1, 2 * TILE - 1], raw_at_least=2 * TILE + 1)
    # an RSTn marker split by the tile boundary: an interval of exactly TILE - 1 bytes (195 blocks of 21 bytes for 4 KiB tiles)
    per = next(L for L in range(17, 60) if (TILE - 1) % L == 0)
    dri = (TILE - 1) // per
    blocks = byte_stream(3 * dri - 7, [], 10, per)
    w, h = 8 * (3 * dri - 7), 8
    add("rst_marker_split_across_a_tile_boundary", "bytes", write(w, h, GREY, {0: Q1}, BYTE_DHT, [[b] for b in blocks], dri=dri), marker_at=[TILE - 1], intervals=3)

    rng = np.random.default_rng(11)
    for delta in (-1, 0, 1):
        t = SMIN + delta
        blocks = fit_segment(FLAT_DC, FLAT_AC, 80, t, rng)
        add("unstuffed_length_sync_min_bytes_%s" % ("minus_1", "exactly", "plus_1")[delta + 1], "bytes", grey(blocks, q=q_ramp(1)), segment_is=[t])
    for delta in (-4, 0, 1):
        t = LMIN * LANES + delta
        blocks = fit_segment(FLAT_DC, FLAT_AC, 640, t, rng)
        add("unstuffed_length_64_bytes_x_all_lanes_%s" % {-4: "minus_4", 0: "exactly", 1: "plus_1"}[delta], "bytes", grey(blocks, q=q_ramp(1)), segment_is=[t],
            **({"lanes_grow": True} if delta > 0 else {"lanes": (LMIN, LANES)}))        # - 4 and 0: the minimum per lane, every lane; + 1: more per lane, fewer lanes
    # 31-bit symbols: a 16-bit code and 15 value bits, repeated -- every lane boundary falls inside one
    sym31 = by_length([(1, 0x00), (16, 0x0F)])
    blocks = [[(15, (-1) ** i * (20000 + i))] + [(0x0F, (-1) ** (i + j) * (16384 + 97 * j + i)) for j in range(63)] for i in range(20)]
    add("31_bit_symbols_repeated_lane_boundaries_inside_symbols", "bytes", grey(blocks, [(0, 0, by_length([(16, 15), (1, 0)])), (1, 0, sym31)], q_ramp(1)),
        lengths={(0, 0): [16], (1, 0): [16]}, segment_at_least=SMIN)

    # ---- phase-locked streams -----------------------------------------------------------------------------------------------------------
    PH = [(0, 0, PHASE), (1, 0, PHASE)]

    def phase_block(r, n_sym, end=False):
        blk = []
        for _ in range(n_sym - (1 if end else 0)):
            s = int(r.integers(1, 8))
            blk.append((s, int(r.integers(1 << (s - 1), 1 << s)) * (1 if r.integers(2) else -1)))
        if end:
            blk.append((0x00, 0))
        return blk

    for lanes in (LANES // 8, LANES):
        r = np.random.default_rng(12 + lanes)
        total = LMIN * lanes
        blocks = [phase_block(r, LMIN // 2, True)] + [phase_block(r, 64) for _ in range(total // 64 - 1)] + [phase_block(r, 64 - LMIN // 2, True)]
        add("phase_locked_grey_zigzag_index_%d_lanes" % lanes, "phase", grey(blocks, PH, q_ramp(1)), segment_is=[total], lanes=(LMIN, lanes), phase_lock="all")
        n_mcu = (total // 64) // 3
        n_mcu += 1 if n_mcu * 192 < SMIN else 0                   # whole MCUs, and a segment the many-lane kernel is given
        mcus = [[phase_block(r, 64) for _ in range(3)] for _ in range(n_mcu)]
        w, h = grey_dims(n_mcu)
        comps = [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 0, 0), (3, 1, 1, 2, 0, 0)]
        add("phase_locked_4_4_4_block_of_the_mcu_%d_lanes" % (n_mcu * 3), "phase", write(w, h, comps, {0: q_ramp(1), 1: q_ramp(2, 3), 2: q_ramp(100, -1)}, PH, mcus),
            segment_is=[n_mcu * 192], lanes=(LMIN, n_mcu * 3), phase_lock="mod3")

    # ---- restart structure ----------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(13)
    blocks = [comb_block(rng) for _ in range(24)]
    add("dri_1_an_interval_per_mcu_rst_numbers_wrap", "restart", grey(blocks, COMB_DHT[:2], q_ramp(1), dri=1), intervals=24)
    add("dri_larger_than_the_mcu_count", "restart", grey(blocks, COMB_DHT[:2], q_ramp(1), dri=1000), intervals=1)
    add("partial_last_interval_padding_bits_0", "restart", grey(blocks, COMB_DHT[:2], q_ramp(1), dri=7, pad_ones=False), intervals=4)
    mcus = [[comb_block(rng) for _ in range(6)] for _ in range(12)]
    add("rst_numbering_past_7_4_2_0", "restart", write(64, 48, MODES[4], {0: q_ramp(1), 1: q_ramp(2)}, COMB_DHT, mcus, dri=1), intervals=12)
    add("fill_bytes_ff_ff_ff_in_front_of_markers", "restart", grey(blocks, COMB_DHT[:2], q_ramp(1), dri=5, fill={0: 3, 2: 1, 3: 3}), intervals=5, fill=[3, 0, 1, 3])
    # long and short intervals in one file: interval 0 and 2 of SMIN bytes and more, 1 and 3 a few bytes
    dri = 64
    r = np.random.default_rng(14)
    blocks = []
    for k in range(4):
        blocks += fit_segment(FLAT_DC, FLAT_AC, dri, SMIN + 200 + k, r) if k % 2 == 0 else [coded(int(r.integers(-9, 9)), {1: 1}) for _ in range(dri)]
    blocks = blocks[:4 * dri - 20]
    add("long_and_short_intervals_in_one_file", "restart", grey(blocks, q=q_ramp(1), dri=dri), intervals=4, segment_is_first=[SMIN + 200])

    # ---- sampling -----------------------------------------------------------------------------------------------------------------------
    for mode, (w, h) in ((0, (24, 16)), (1, (24, 16)), (2, (40, 16)), (3, (16, 40)), (4, (40, 24))):
        r = np.random.default_rng(20 + mode)
        mcus = [[comb_block(r) for _ in range(NB[mode])] for _ in range(n_mcus(mode, w, h))]
        add("comb_tables_scan_type_%d" % mode, "sampling", write(w, h, MODES[mode], {0: q_ramp(1), 1: q_ramp(2)}, COMB_DHT, mcus), scan_type=mode)
    # 4:2:0, one segment of SMIN bytes or more: the files that hand over tokens
    r = np.random.default_rng(30)
    mcus = [[comb_block(r, dense=True) for _ in range(6)] for _ in range(n_mcus(4, 120, 56))]
    add("comb_tables_4_2_0_long_scan_tokens", "sampling", write(120, 56, MODES[4], {0: q_ramp(1), 1: q_ramp(2)}, COMB_DHT, mcus), scan_type=4, segment_at_least=SMIN)
    mcus = [[full_blocks(1, 1000 + 7 * i + j, dense=True)[0] for j in range(6)] for i in range(n_mcus(4, 128, 64))]
    add("complete_code_4_2_0_long_scan_tokens", "sampling",
        write(128, 64, MODES[4], {0: q_ramp(1), 1: q16}, FULL_DHT + [(0, 1, full_dc), (1, 1, full_ac)], mcus), scan_type=4, segment_at_least=SMIN, complete=[(0, 0), (1, 0)])
    # a baseline frame of three scans, one per component: T.81 defines it, the reference decodes sequential frames of ONE interleaved scan only -- a
    # scan of one component leaves its MCU buffers a size they were not made for (no defined result), the library refuses the file
    r = np.random.default_rng(31)
    units = [[[comb_block(r)] for _ in range(6)] for _ in range(3)]
    add("three_non_interleaved_scans_no_defined_result_in_the_reference", "sampling",
        write(24, 16, MODES[1], {0: q_ramp(1), 1: q_ramp(2)}, COMB_DHT, scans=[([c], units[c]) for c in range(3)]), "undefined", wellformed=True, scans=3)
    return out
