"""DEFLATE streams no encoder writes, for the inflate kernel (gamut_amd/csrc/inflate.hip): a bit-level builder (stored, fixed and dynamic blocks;
a dynamic header takes its code-length code and the spelling of its lengths as given, so illegal ones can be written too; token runs become
numpy bit arrays) and the list of cases, each named for the mechanism of the kernel it is aimed at.  A case is (name, data, expect, status,
note, meta): expect = the bytes the builder's own tokens stand for (None: the stream is corrupt), status = the GAMUT_HIP_INFLATE_E_* the
kernel names for it (None: a good stream, ANY: corrupt, but which check meets it first is the kernel's business), meta = the facts the
builder laid the stream out for (bit positions, lanes), which tests/test_inflate_cases_cpu.py checks against the census of
tests/inflate_ref.py.  Everything is deterministic: one seeded generator per case.  zlib and tests/inflate_ref.py must agree with `expect`
on every case (test_inflate_cases_cpu.py); the kernel is compared with zlib in tests/test_inflate_cases_gpu.py."""
import collections

import numpy as np

from inflate_ref import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA, LONG_MATCH, ROUND_BYTES, TILE_BYTES

# The geometry of the kernel the cases are laid out against (inflate.hip: kT, kSubBits, kRoundBytes, kNewMax, kTokCap, kLongCap, kLongMin and the
# 64 lanes x 32 bits a round of read_code_lengths takes).  Written down here, not read from the source: a kernel retuned to other sizes still has to
# inflate these streams, and tests/test_inflate_cases_cpu.py says which mechanism each size stands for.
# (ROUND_BYTES, TILE_BYTES and LONG_MATCH are the census's: tests/inflate_ref.py)
LANES, LANE_BITS = 1024, 256                         # ROUND_BYTES = LANES * LANE_BITS / 8
assert LANES * LANE_BITS // 8 == ROUND_BYTES
TOKEN_CAP = 32768                                    # tokens a round's list holds
LONG_CAP, LONG_MIN = 768, LONG_MATCH                 # long matches a tile's list holds; what counts as long
CL_ROUND_BITS = 64 * 32                              # bits of code-length stream wave 0 takes per round of read_code_lengths
WAVE = 64
SLICE_MIN = 33 * 1024                                # streams longer than this can suspend in a sliced call (kRoundBytes + 64 is the smallest span)

E_BLOCK_TYPE, E_STORED, E_LENGTHS, E_CODE, E_DISTANCE, E_INPUT = 1, 2, 3, 4, 5, 6       # GAMUT_HIP_INFLATE_E_* (include/gamut_hip.h)
ANY = -1
STATUS_OF_REASON = {"block type": E_BLOCK_TYPE, "stored": E_STORED, "lengths": E_LENGTHS, "code": E_CODE, "distance": E_DISTANCE, "input": E_INPUT}

Case = collections.namedtuple("Case", "name data expect status note meta")

_LEN_BASE, _LEN_EXTRA = np.array(LEN_BASE + [0, 0]), np.array(LEN_EXTRA + [0, 0])          # (+ symbols 286, 287: no extra bits)
_DIST_BASE, _DIST_EXTRA = np.array(DIST_BASE + [0, 0]), np.array(DIST_EXTRA + [0, 0])       # (+ symbols 30, 31)


# ------------------------------------------------------------------------------------------------------------------------ the builder
class BitWriter:
    """bits in stream order: fields LSB first, Huffman codes MSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self._chunks, self._small, self.nbits = [], [], 0

    def bits(self, value, n):
        self._small += [(value >> i) & 1 for i in range(n)]
        self.nbits += n

    def code(self, code, n):
        self._small += [(code >> i) & 1 for i in range(n - 1, -1, -1)]
        self.nbits += n

    def array(self, arr):
        if self._small:
            self._chunks.append(np.array(self._small, np.uint8)); self._small = []
        self._chunks.append(np.asarray(arr, np.uint8))
        self.nbits += len(arr)

    def align(self):
        self.bits(0, -self.nbits % 8)

    def raw(self, data):
        assert self.nbits % 8 == 0
        self.array(np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little"))

    def getvalue(self):
        self.array(np.zeros(0, np.uint8))
        return np.packbits(np.concatenate(self._chunks), bitorder="little").tobytes()


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol (0 for a symbol without one); an over-subscribed set gets the codes the algorithm gives"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


def _reversed_codes(lengths):
    """per symbol: the code as the stream holds it (first bit in bit 0)"""
    return np.array([int(format(c, f"0{l}b")[::-1], 2) if l else 0 for c, l in zip(canonical_codes(lengths), lengths)], np.int64)


def lits(data):
    """literal tokens: rows (literal / length symbol, extra bits, distance symbol or -1, extra bits)"""
    t = np.full((len(data), 4), 0, np.int64)
    t[:, 0] = np.frombuffer(bytes(data), np.uint8)
    t[:, 2] = -1
    return t


def matches(lengths, dists, as_284=False):
    """match tokens of the given lengths and distances; as_284: length 258 spelled as symbol 284 with extra bits 31"""
    lengths, dists = np.atleast_1d(np.asarray(lengths, np.int64)), np.atleast_1d(np.asarray(dists, np.int64))
    lengths, dists = np.broadcast_arrays(lengths, dists)
    ls = np.searchsorted(_LEN_BASE[:29], lengths, "right") - 1
    if as_284:
        ls = np.where(lengths == 258, 27, ls)
    ds = np.searchsorted(_DIST_BASE[:30], dists, "right") - 1
    return np.stack([ls + 257, lengths - _LEN_BASE[ls], ds, dists - _DIST_BASE[ds]], 1)


def raw_match(lsym, lextra, dsym, dextra):
    return np.array([[lsym, lextra, dsym, dextra]], np.int64)


def cat(*parts):
    return np.concatenate([np.asarray(p, np.int64).reshape(-1, 4) for p in parts])


def token_bits(tokens, lit_lens, dist_lens):
    """the tokens as a numpy array of stream bits"""
    tokens = np.asarray(tokens, np.int64).reshape(-1, 4)
    if not len(tokens):
        return np.zeros(0, np.uint8)
    ll, dl = np.array(list(lit_lens) + [0] * (288 - len(lit_lens))), np.array(list(dist_lens) + [0] * (32 - len(dist_lens)))
    lc, dc = _reversed_codes(list(ll)), _reversed_codes(list(dl))
    ls, ds = tokens[:, 0], tokens[:, 2]
    is_match = ds >= 0
    dsx = np.where(is_match, ds, 0)
    assert (ll[ls] > 0).all() and (dl[dsx][is_match] > 0).all(), "a token uses a symbol without a code"
    lx = np.where(ls > 256, _LEN_EXTRA[np.maximum(ls - 257, 0)], 0)
    values = np.stack([lc[ls], tokens[:, 1], np.where(is_match, dc[dsx], 0), tokens[:, 3]], 1).ravel()
    widths = np.stack([ll[ls], lx, np.where(is_match, dl[dsx], 0), np.where(is_match, _DIST_EXTRA[dsx], 0)], 1).ravel()
    starts = np.cumsum(widths) - widths
    field = np.repeat(np.arange(values.size), widths)
    return ((values[field] >> (np.arange(int(widths.sum())) - starts[field])) & 1).astype(np.uint8)


def expand(tokens, out):
    """the bytes the tokens stand for, appended to `out` (a bytearray that holds the stream's output so far)"""
    tokens = np.asarray(tokens, np.int64).reshape(-1, 4)
    where = np.flatnonzero(tokens[:, 2] >= 0)
    lit_bytes = tokens[:, 0].astype(np.uint8)
    at = 0
    for k, (ls, lx, ds, dx) in zip(where.tolist(), tokens[where].tolist()):
        if k > at:
            out += lit_bytes[at:k].tobytes()
        at = k + 1
        length, dist = int(_LEN_BASE[ls - 257]) + lx, int(_DIST_BASE[ds]) + dx     # (symbols 286, 287, 30 and 31 of corrupt streams: nothing)
        assert dist <= len(out), "the builder asked for a distance beyond its own output"
        if not dist or not length:
            continue
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            piece = bytes(out[len(out) - dist:])
            out += (piece * (length // dist + 1))[:length]
    out += lit_bytes[at:].tobytes()
    return out


def spell_single(lengths):
    return [(l, 0) for l in lengths]


def spell_runs(lengths, rng=None):
    """the lengths with repeats the way an encoder would write them (rng: a random mix of single lengths and repeats of random size instead)"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        run = 1
        while i + run < n and lengths[i + run] == lengths[i]:
            run += 1
        v = lengths[i]
        if rng is not None and rng.random() < 0.3:
            run = 1
        if v == 0 and run >= 3:
            take = min(run, 138) if rng is None else int(rng.integers(3, min(run, 138) + 1))
            out.append((17, take - 3) if take <= 10 else (18, take - 11))
            i += take
        elif run >= 4:
            take = min(run - 1, 6) if rng is None else int(rng.integers(3, min(run - 1, 6) + 1))
            out += [(v, 0), (16, take - 3)]
            i += 1 + take
        else:
            out.append((v, 0)); i += 1
    return out


def balanced_lengths(symbols, size):
    """a complete code over the given symbols (two or more), as flat as it can be: lengths of a code of `size` symbols"""
    n = len(symbols)
    assert n >= 2
    k = n.bit_length() - 1
    short = (2 << k) - n                              # codes of k bits; the rest have k + 1
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    return lens


def random_complete_lengths(rng, symbols, size, maxlen):
    """a random complete code over the given symbols (two or more): leaves split at random down to maxlen"""
    depths = [1, 1]
    while len(depths) < len(symbols):
        open_ = [i for i, d in enumerate(depths) if d < maxlen]
        i = open_[int(rng.integers(len(open_)))]
        depths[i] += 1
        depths.append(depths[i])
    order = rng.permutation(len(symbols))
    lens = [0] * size
    for d, k in zip(depths, order):
        lens[symbols[int(k)]] = d
    return lens


def cl_boundaries(spelling, cl_lens):
    """the bit every symbol of the code-length stream begins at (from the stream's first bit), and the stream's length as the last entry"""
    at, out = 0, []
    for s, _ in spelling:
        out.append(at)
        at += cl_lens[s] + (0 if s < 16 else 2 if s == 16 else 3 if s == 17 else 7)
    return out + [at]


def lanes_awake(blocks):
    """Per block of a census (tests/inflate_ref.py; [] for a stored block): the lanes k_inflate wakes in each round of the block -- its `awake` estimate from
    the bit length of the Huffman block before (last_block_bits; 0 in front of the stream's first Huffman block: all kT lanes), rounded up to whole waves.  A
    round ends with lane `awake` (kT - 1 of a full round); the few bits its last token hangs over are counted as 0."""
    last, out = 0, []
    for b in blocks:
        if b["type"] == 0:
            out.append([])
            continue
        begin, end = b["begin_bit"], b["begin_bit"] + b["bits"]
        base = b["at_bit"] // 32 * 32                                    # (the header's window serves the first round if the data begins within 16 lanes of it)
        if begin - base >= 16 * LANE_BITS:
            base = begin // 32 * 32
        pos, rounds = begin, []
        while pos < end:
            awake = LANES
            if last:
                left = max(last - (pos - begin), 0)
                want = (pos - base) + left + left // 4 + 4 * LANE_BITS
                awake = LANES if want // LANE_BITS >= LANES else min((want // LANE_BITS + 64) & ~63, LANES)
            rounds.append(awake)
            pos = base + (awake if awake < LANES else LANES - 1) * LANE_BITS
            base = pos // 32 * 32
        last = b["bits"]
        out.append(rounds)
    return out


def header_on_phase(at_bit, phase, lit_lens, dist_lens):
    """keywords for Stream.dynamic (dist_lens, spelling, cl_lens, hclen) of a header that begins at bit `at_bit` and whose block data begins on bit `phase` of a
    byte: the header's own length is varied -- code-length slots that stay 0 (hclen, 3 bits each) and zero distance lengths at the end, spelled singly.  No short
    Huffman block in front: that would narrow every round of this block to a wave (lanes_awake)."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    spelling = spell_runs(lit_lens + dist_lens)
    used = sorted({s for s, _ in spelling} | {0})
    cl = balanced_lengths(used if len(used) > 1 else used + [18], 19)
    least = max([4] + [k + 1 for k in range(19) if cl[CL_ORDER[k]]])
    for zeros in range(31 - len(dist_lens)):
        for hclen in range(least, 20):
            kw = dict(dist_lens=dist_lens + [0] * zeros, spelling=spelling + [(0, 0)] * zeros, cl_lens=cl, hclen=hclen)
            probe = Stream(); probe.w.bits(0, at_bit)
            probe.dynamic_header(0, lit_lens, **kw)
            if probe.w.nbits % 8 == phase:
                return kw
    raise AssertionError("no header of that phase")


class Stream:
    """a stream under construction and the bytes it stands for"""

    def __init__(self):
        self.w, self.out, self.meta = BitWriter(), bytearray(), {}

    def header(self, final, btype):
        self.w.bits(final, 1); self.w.bits(btype, 2)

    def stored(self, data, final=0, length=None, nlen=None, cut=None):
        self.header(final, 0)
        self.w.align()
        length = len(data) if length is None else length
        self.w.bits(length, 16); self.w.bits(length ^ 0xFFFF if nlen is None else nlen, 16)
        self.w.raw(data if cut is None else data[:cut])
        self.out += data
        return self

    def fixed(self, tokens, final=0, eob=True):
        self.header(final, 1)
        self.w.array(token_bits(tokens, FIXED_LIT, FIXED_DIST))
        if eob:
            self.w.code(0, 7)
        expand(tokens, self.out)
        return self

    def dynamic_header(self, final, lit_lens, dist_lens, spelling=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if spelling is None:
            spelling = spell_runs(lit_lens + dist_lens)
        if cl_lens is None:
            used = sorted({s for s, _ in spelling})
            cl_lens = balanced_lengths(used if len(used) > 1 else used + [(used[0] + 1) % 19], 19)
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        self.header(final, 2)
        self.w.bits((len(lit_lens) if hlit is None else hlit) - 257, 5)
        self.w.bits((len(dist_lens) if hdist is None else hdist) - 1, 5)
        self.w.bits(hclen - 4, 4)
        for k in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[k]], 3)
        codes = canonical_codes(cl_lens)
        self.meta.setdefault("cl_begin", []).append(self.w.nbits)
        for s, x in spelling:
            self.w.code(codes[s], cl_lens[s])
            if s >= 16:
                self.w.bits(x, (2, 3, 7)[s - 16])
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=0, eob=True, **header):
        self.dynamic_header(final, lit_lens, dist_lens, **header)
        self.meta.setdefault("data_begin", []).append(self.w.nbits)
        self.w.array(token_bits(tokens, lit_lens, dist_lens))
        if eob:
            self.meta.setdefault("eob_at", []).append(self.w.nbits)
            self.w.code(canonical_codes(list(lit_lens))[256], lit_lens[256])
        expand(tokens, self.out)
        return self

    def case(self, name, note, status=None, **meta):
        self.meta.update(meta)
        return Case(name, self.w.getvalue(), bytes(self.out) if status is None else None, status, note, dict(self.meta))


def lens_of(pairs, size):
    lens = [0] * size
    for s, l in pairs.items():
        lens[s] = l
    return lens


def history_tokens(n):
    """tokens (for a fixed block) that stand for exactly n bytes of period 251 beginning with a zero byte: a distance that is off by less than
    251 shows in the bytes"""
    seed = bytes((7 * i) % 256 for i in range(251))
    if n <= 251 + 3:
        return lits((seed * 2)[:n])
    parts, left = [lits(seed)], n - 251
    while left:
        take = 258 if left >= 258 + 3 or left == 258 else left if left <= 258 else left - 3
        parts.append(matches(take, 251)); left -= take
    return cat(*parts)


def random_tokens(rng, n, lit_lens, dist_lens, produced):
    """n random tokens the two codes can write, with `produced` bytes of history in front"""
    lsyms = [s for s, l in enumerate(lit_lens) if l and s != 256 and s < 286]
    literals = [s for s in lsyms if s < 256]
    dsyms = [s for s, l in enumerate(dist_lens) if l and s < 30]
    rows = []
    for _ in range(n):
        s = lsyms[int(rng.integers(len(lsyms)))]
        near = [d for d in dsyms if DIST_BASE[d] <= produced]
        if s > 256 and not near:
            if not literals:
                continue
            s = literals[int(rng.integers(len(literals)))]
        if s < 256:
            rows.append((s, 0, -1, 0)); produced += 1
            continue
        d = near[int(rng.integers(len(near)))]
        dx = int(rng.integers(0, min(1 << DIST_EXTRA[d], produced - DIST_BASE[d] + 1)))
        lx = int(rng.integers(0, 1 << LEN_EXTRA[s - 257]))
        rows.append((s, lx, d, dx)); produced += LEN_BASE[s - 257] + lx
    return np.array(rows, np.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------------------ the cases
# Codes that use every length 1 .. 15: sixteen symbols, one per length and two of 15 bits (the only such set: the lengths 1 .. 15 leave 2^-15).
ALL_LIT = lens_of({0x41: 1, 257: 2, 258: 3, 0x00: 4, 0x10: 5, 0x20: 6, 0x30: 7, 0x40: 8, 0x50: 9, 0x60: 10, 0x70: 11, 0xC8: 12, 285: 13, 0xFF: 14, 256: 15, 284: 15}, 286)
ALL_DIST_A = lens_of({**{k: 5 * k % 14 + 1 for k in range(14)}, 28: 15, 29: 15}, 30)                   # symbols 0-13, 28, 29
ALL_DIST_B = lens_of({**{14 + k: k + 1 for k in range(13)}, 27: 13}, 28)                               # symbols 14-27: lengths 1 .. 13, 13
LIT_B = lens_of({**{k: 4 for k in range(1, 10)}, 257: 3, 258: 3, 285: 4, 284: 4, 256: 4}, 286)
HISTORY = 33017                                       # bytes history_tokens() is asked for in front of window-sized distances (> 32 768)
LENGTH_SPELLINGS = ((257, 0), (258, 0), (285, 0), (284, 31))                                           # lengths 3, 4, 258 and 258 again


def _every_distance(dist_lens):
    return cat(*[raw_match(ls, lx, d, dx) for d, l in enumerate(dist_lens) if l for dx in (0, (1 << DIST_EXTRA[d]) - 1) for ls, lx in LENGTH_SPELLINGS])


def code_table_cases():
    out = []
    s = Stream().fixed(history_tokens(HISTORY))
    a_literals = lits(bytes(k for k, l in enumerate(ALL_LIT[:256]) if l))
    longest = cat(*[raw_match(284, 31, 29, 8191 - k) for k in range(40)])                               # 15 + 5 + 15 + 13 = 48 bits each
    s.dynamic(cat(a_literals, _every_distance(ALL_DIST_A), longest), ALL_LIT, ALL_DIST_A)
    s.dynamic(cat(lits(bytes(range(1, 10))), _every_distance(ALL_DIST_B)), LIT_B, ALL_DIST_B, final=1)
    out.append(s.case("long codes", "build_tables / CodeRange / LongLit / LongDist (read_code, lut entry 0): literal / length and distance codes of every length 1-15, "
                      "every distance symbol with extra bits all 0 and all 1 at lengths 3, 4, 258 and 258 as 284 + 31, forty 48-bit tokens back to back (lane_trace: used <= 36)"))
    rng = np.random.default_rng(101)
    s = Stream().stored(bytes(expand(history_tokens(HISTORY), bytearray())))            # (stored: the block behind it is the stream's first Huffman block, all lanes awake)
    d_a = [d for d, l in enumerate(ALL_DIST_A) if l]
    n = 52000
    ds = np.array(d_a)[rng.integers(0, len(d_a), n)]
    rows = np.stack([np.where(rng.random(n) < 0.5, 257, 258), np.zeros(n, np.int64), ds, rng.integers(0, 1 << 13, n) & ((1 << _DIST_EXTRA[ds]) - 1)], 1)
    literal = rng.random(n) < 0.5
    rows[literal] = np.stack([np.array([0xC8, 0xFF, 0x70, 0x60])[rng.integers(0, 4, int(literal.sum()))], np.zeros(int(literal.sum()), np.int64),
                              np.full(int(literal.sum()), -1), np.zeros(int(literal.sum()), np.int64)], 1)
    s.dynamic(rows, ALL_LIT, ALL_DIST_A)
    s.stored(rng.integers(0, 256, 65535, dtype=np.uint8).tobytes())
    s.fixed(matches([258, 3], [32768, 1]), final=1)
    out.append(s.case("long codes, three rounds, then a full stored block", "three full-width rounds of 1-15 bit codes (LongLit / LongDist in every lane); a sliced call suspends inside the block "
                      "(tables rebuilt from InfState.lens) and in front of a 65 535-byte stored block (p + 4 + 65535 > have)"))

    # literal pairs (INFLATE_PAIRS): lengths 1 .. 7, 7 -- 5 + 6 and 4 + 7 are pairs, 6 + 6 and 5 + 7 are not, 1 + 1 is
    pair_lit = lens_of({ord("a"): 1, ord("b"): 2, ord("c"): 3, ord("d"): 4, ord("e"): 5, ord("f"): 6, ord("g"): 7, 256: 7}, 257)
    rng = np.random.default_rng(102)
    text = b"ef" * 9 + b"fe" * 9 + b"ff" * 9 + b"eg" * 9 + b"dg" * 9 + b"gd" * 9 + b"a" * 301 + b"gg" * 5 + bytes(rng.choice(list(b"abcdefg"), 3000).tolist())
    out.append(Stream().dynamic(lits(text), pair_lit, [0], final=1).case("literal pairs of 11 and 12 bits", "build_tables: a pair needs l1 + l2 <= kLitBits = 11 (5 + 6, 4 + 7: pairs; "
               "6 + 6, 5 + 7: single literals); a 1-bit literal with itself; the second code looked up with lengths up to kLitBits - l1 only"))
    lit56 = lens_of({**{k: 5 for k in range(20)}, **{k: 6 for k in range(20, 43)}, 256: 6}, 257)
    rng = np.random.default_rng(103)
    body = rng.integers(0, 43, 62000, dtype=np.uint8).tobytes()
    out.append(Stream().dynamic(lits(body), lit56, [0], final=1).case("literal pairs on every phase of a lane", "read_code: at + l1 >= end takes the first literal of a pair "
               "alone; 5- and 6-bit literals for more than a round put pair boundaries on every bit of a lane's 256"))

    # incomplete and degenerate sets
    three = lens_of({ord("x"): 2, 257: 2, 256: 1}, 258)
    out.append(Stream().dynamic(cat(lits(b"xx"), raw_match(257, 0, 0, 0), lits(b"x"), raw_match(257, 0, 0, 0)), three, [1], final=1)
               .case("one 1-bit distance code, bit 0", "build_tables: an incomplete distance set is legal when no code is longer than one bit"))
    s = Stream().dynamic_header(1, three, [1])
    s.w.array(token_bits(lits(b"xx"), three, [1])); s.w.code(canonical_codes(three)[257], 2); s.w.bits(1, 1); s.w.bits(0, 24)
    out.append(s.case("one 1-bit distance code, bit 1", "CodeRange::decode finds no code -> kind 3 (invalid), as zlib's 'invalid distance code'", status=E_CODE))
    out.append(Stream().dynamic(cat(lits(b"xx"), raw_match(257, 0, 1, 0), raw_match(257, 0, 0, 0)), three, [1, 1], final=1)
               .case("two 1-bit distance codes", "build_tables: the smallest complete distance set"))
    only_lit = lens_of({ord("x"): 1, 256: 1}, 257)
    out.append(Stream().dynamic(lits(b"xxxxx"), only_lit, [0], final=1).case("hdist 1 with length 0, literals only", "build_tables: a block with no distance code at all "
               "(kraft 0, maxlen 0) is legal; hlit = 257"))
    s = Stream().dynamic_header(1, three, [0])
    s.w.array(token_bits(lits(b"xx"), three, [0])); s.w.code(canonical_codes(three)[257], 2); s.w.bits(0, 24)
    out.append(s.case("hdist 1 with length 0, then a match", "read_code with an empty distance table: lut entry 0, LongDist finds nothing -> invalid", status=E_CODE))
    eob_only = lens_of({256: 1}, 257)
    out.append(Stream().stored(b"only an end of block follows").dynamic(lits(b""), eob_only, [0], final=1)
               .case("a literal code that is just end-of-block", "build_tables: an incomplete literal / length set of one 1-bit code"))
    s = Stream().stored(b"stored").dynamic_header(1, eob_only, [0]); s.w.bits(1, 1); s.w.bits(0, 24)
    out.append(s.case("a literal code that is just end-of-block, the other bit", "the unused half of an incomplete 1-bit code is an invalid code", status=E_CODE))
    rng = np.random.default_rng(104)
    lit257 = random_complete_lengths(rng, list(range(257)), 257, 15)
    out.append(Stream().dynamic(lits(rng.integers(0, 256, 400, dtype=np.uint8).tobytes()), lit257, [0], final=1).case("hlit 257", "the smallest literal / length alphabet"))

    # header limits
    flat286 = [8] * 226 + [9] * 60
    flat30 = [4, 4] + [5] * 28
    rng = np.random.default_rng(105)
    tok = random_tokens(rng, 200, flat286, flat30, 0)
    out.append(Stream().dynamic(tok, flat286, flat30, final=1).case("hlit 286 and hdist 30", "the largest alphabets (threads 0-285 and 288-317 of build_tables hold a symbol)"))
    for hlit in (287, 288):
        out.append(Stream().dynamic(tok, flat286, flat30, final=1, hlit=hlit).case(f"hlit {hlit}", "k_inflate, header: hlit > 286", status=E_LENGTHS))
    for hdist in (31, 32):
        out.append(Stream().dynamic(tok, flat286, flat30, final=1, hdist=hdist).case(f"hdist {hdist}", "k_inflate, header: hdist > 30", status=E_LENGTHS))
    bad_sets = {
        "no end-of-block code": (lens_of({0: 1, 1: 1}, 257), [0], None, "k_inflate, header: S.lens[256] == 0"),
        "over-subscribed literal set": (lens_of({0: 1, 1: 1, 256: 1}, 257), [0], None, "build_tables: kraft > 32768"),
        "over-subscribed distance set": (only_lit, [1, 1, 1], None, "build_tables: kraft > 32768 (distance row)"),
        "over-subscribed code-length set": (only_lit, [0], lens_of({0: 1, 1: 1, 18: 1}, 19), "read_code_lengths: kraft != 128"),
        "incomplete literal set": (lens_of({0: 2, 256: 2}, 257), [0], None, "build_tables: kraft < 32768 and maxlen > 1"),
        "incomplete distance set": (only_lit, [2], None, "build_tables: kraft < 32768 and maxlen > 1 (distance row)"),
        "incomplete code-length set": (only_lit, [0], lens_of({0: 2, 1: 2, 18: 2}, 19), "read_code_lengths: kraft != 128"),
        "a code-length code of one 1-bit symbol": (lens_of({256: 8}, 257), [0], lens_of({8: 1}, 19), "read_code_lengths: kraft != 128 (zlib: an incomplete code-length code is never legal)"),
    }
    for name, (ll, dl, cl, note) in bad_sets.items():
        spelling = spell_runs(ll + dl) if "one 1-bit" not in name else [(8, 0)] * 258
        s = Stream().dynamic_header(1, ll, dl, spelling=spelling, cl_lens=cl); s.w.bits(0, 24)
        out.append(s.case(name, note, status=E_LENGTHS))

    # the fixed code
    for sym in (286, 287):
        out.append(Stream().fixed(cat(lits(b"abc"), raw_match(sym, 0, 0, 0)), final=1).case(f"fixed block, literal / length symbol {sym}", "lit_payload: s > 285 is invalid", status=E_CODE))
    for sym in (30, 31):
        out.append(Stream().fixed(cat(lits(b"abc"), raw_match(257, 0, sym, 0)), final=1).case(f"fixed block, distance symbol {sym}", "dist_payload: d > 29 is invalid", status=E_CODE))
    d30 = np.packbits(np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0], np.uint8), 2000), bitorder="little").tobytes()      # symbol 257, then distance symbol 30
    out.append(Stream().fixed(lits(b"in front of stored blocks that read as invalid codes")).stored(b"\x63" * 3000).fixed(lits(b"!")).stored(d30, final=1)
               .case("fixed block, then stored bytes that read as invalid codes", "the sweep loop: lanes behind the end-of-block stop see F_BAD (symbol 286 on every byte boundary, "
                     "distance symbol 30) -- only the first stop of the chain counts"))
    return out


def _long_cl_case(name, note, lit_lens, dist_lens, spelling, rng):
    cl = lens_of({**{k: 7 for k in range(19)}, 1: 1, 2: 2, 3: 3}, 19)
    s = Stream().stored(bytes(range(40)))
    tok = random_tokens(rng, 50, lit_lens, dist_lens, 40)
    s.dynamic(tok, lit_lens, dist_lens, final=1, spelling=spelling, cl_lens=cl, hclen=19)
    b = cl_boundaries(spelling, cl)
    second = next(k for k, at in enumerate(b) if at >= CL_ROUND_BITS)
    return s.case(name, note, cl_bits=b[-1], round2_first_symbol=spelling[second][0] if second < len(spelling) else None, round2_begin=b[second], cl_symbols=len(spelling))


def code_length_cases():
    out = []
    flat286, flat30 = [8] * 226 + [9] * 60, [4, 4] + [5] * 28
    rng = np.random.default_rng(201)
    every = flat286 + flat30
    out.append(_long_cl_case("code lengths: 2 212 bits, all single", "read_code_lengths: the second round (done, carry and h carried over); hclen 19; 7-bit code-length codes",
                             flat286, flat30, spell_single(every), rng))
    sp = spell_single(every[:293]) + [(16, 3)] + spell_single(every[299:])
    out.append(_long_cl_case("code lengths: round 2 begins with a repeat-16", "read_code_lengths: lane 0 of round 2 has nothing in front: `before = carry`",
                             flat286, flat30, sp, rng))
    gap30 = [4] * 6 + [0] * 6 + [4] * 2 + [5] * 16
    sp = spell_single(flat286 + gap30[:6]) + [(17, 0), (16, 0)] + spell_single(gap30[12:])
    out.append(_long_cl_case("code lengths: a 17 ends round 1, a repeat-16 begins round 2", "cl_walk: a 17 sets the running length to 0 (last = 0x100 | 0), and `carry` takes it "
                             "into round 2, where the 16 repeats 0", flat286, gap30, sp, rng))
    tail5 = [8] * 181 + [9] * 102 + [5] * 3
    dist5 = [5] * 28 + [4] * 2
    sp = spell_single(tail5[:284]) + [(16, 3)] + spell_single((tail5 + dist5)[290:])
    out.append(_long_cl_case("code lengths: a repeat-16 from the literal lengths into the distance lengths", "the lengths are one sequence of hlit + hdist (cl_walk<true> writes S.lens[i + k] "
                             "across the seam)", tail5, dist5, sp, rng))
    # the stream's end against the 32-bit lanes of round 2: repeats of 3-6 at the tail move it (a 16 takes 9 bits for 3-6 lengths of 7 each)
    cl = lens_of({**{k: 7 for k in range(19)}, 1: 1, 2: 2, 3: 3}, 19)
    for want, label in ((0, "on"), (31, "one bit before"), (1, "one bit after")):
        found = None
        for reps in ((), (6,), (3,), (4,), (5,), (3, 3), (3, 4), (4, 4), (3, 5), (4, 5), (5, 5), (3, 6), (4, 6), (5, 6), (6, 6), (3, 3, 3), (3, 3, 4), (3, 4, 4), (4, 4, 4), (3, 3, 5),
                     (3, 4, 5), (3, 3, 3, 3), (3, 3, 3, 4), (3, 3, 3, 3, 3), (3, 3, 3, 3, 4), (3, 3, 3, 3, 3, 4), (3, 3, 3, 3, 3, 4, 4)):
            sp = spell_single(every[:316 - sum(reps)]) + [(16, r - 3) for r in reps]
            b = cl_boundaries(sp, cl)
            begin2 = next(at for at in b if at >= CL_ROUND_BITS)
            if b[-1] > begin2 and (b[-1] - begin2) % 32 == want:
                found = sp
                break
        assert found, label
        out.append(_long_cl_case(f"code lengths: the last length ends {label} a lane boundary of round 2", "read_code_lengths: end_pos comes from the lane that writes the last length; "
                                 "`need` = the first lane whose prefix sum reaches `total`", flat286, flat30, found, rng))

    # spellings
    s = Stream().dynamic_header(1, [0] * 257, [0], spelling=[(18, 127), (18, 109)], cl_lens=lens_of({0: 1, 18: 1}, 19), hclen=4); s.w.bits(0, 24)
    out.append(s.case("hclen 4", "read_code_lengths: `place < hclen` -- only 16, 17, 18 and 0 can have codes, so every length is 0 and the end-of-block code is missing", status=E_LENGTHS))
    wide = lens_of({0: 2, 1: 2, 256: 1}, 257)
    out.append(Stream().dynamic(lits(bytes([0, 1, 1, 0])), wide, [0], final=1, spelling=[(2, 0), (2, 0), (18, 127), (18, 105), (1, 0), (0, 0)])
               .case("an 18 with 138 zeros", "cl_walk: rep = 11 + 127"))
    out.append(Stream().dynamic(lits(bytes([0, 1, 1, 0])), wide, [0], final=1, spelling=[(2, 0), (2, 0)] + [(17, 7)] * 25 + [(17, 1), (1, 0), (17, 0)], hdist=3)
               .case("a run of 17s", "cl_walk: rep = 3 + x, twenty-six in a row and one that ends the lengths"))
    out.append(Stream().dynamic(lits(bytes([0, 1])), wide, [0], final=1, spelling=[(2, 0), (2, 0), (18, 0), (16, 3), (18, 127), (18, 88), (1, 0), (0, 0)])
               .case("a repeat-16 behind an 18", "cl_walk: `prev = val` for 17 and 18 too: the 16 repeats 0"))
    s = Stream().dynamic_header(1, wide, [0], spelling=[(16, 0), (2, 0), (2, 0), (18, 127), (18, 102), (1, 0), (0, 0)]); s.w.bits(0, 24)
    out.append(s.case("a repeat-16 as the first symbol", "cl_walk<true>: sym == 16 && i == 0", status=E_LENGTHS))
    s = Stream().dynamic_header(1, wide, [0], spelling=[(2, 0), (2, 0), (18, 127), (18, 105), (1, 0), (17, 0)]); s.w.bits(0, 24)
    out.append(s.case("a repeat that runs past hlit + hdist", "cl_walk<true>: i + rep > total", status=E_LENGTHS))
    s = Stream().dynamic_header(1, wide, [0], spelling=[(2, 0), (2, 0), (18, 127)])
    out.append(s.case("lengths that stop short: the stream ends", "read_code_lengths reads zeros behind the stream's end; the header ends beyond src_bits, or its lengths are no code", status=ANY))

    for k in range(64):
        rng = np.random.default_rng(1000 + k)
        n_lit = int(rng.integers(3, 286))
        lit_syms = sorted(set(rng.choice(286, n_lit, replace=False).tolist()) | {256, int(rng.integers(0, 256)), int(rng.integers(257, 286))})
        lit_lens = random_complete_lengths(rng, lit_syms, int(max(lit_syms[-1] + 1, 257 + rng.integers(0, 30))), 15)
        lit_lens = lit_lens[:286]
        n_dist = int(rng.integers(2, 31))
        dist_syms = sorted(rng.choice(30, n_dist, replace=False).tolist())
        dist_lens = random_complete_lengths(rng, dist_syms, int(max(dist_syms[-1] + 1, rng.integers(1, 31))), 15)
        spelling = spell_runs(lit_lens + dist_lens, rng)
        used = sorted({s for s, _ in spelling})
        cl = random_complete_lengths(rng, used if len(used) > 1 else used + [(used[0] + 1) % 19], 19, 7)
        s = Stream().stored(rng.integers(0, 256, 600, dtype=np.uint8).tobytes())
        s.dynamic(random_tokens(rng, 50, lit_lens, dist_lens, 600), lit_lens, dist_lens, final=1, spelling=spelling, cl_lens=cl)
        out.append(s.case(f"random header {k}", "read_code_lengths / build_tables: random complete codes, a random mix of single lengths and repeats"))
    return out


def _never_resyncs(kind, rng, n_bytes):
    """(literal / length lengths, distance lengths, tokens) of a block whose tokens all have the same even length"""
    if kind == "2-bit codes":
        lit = lens_of({0x00: 2, 0x55: 2, 0xAA: 2, 256: 2}, 257)
        return lit, [0], lits(np.array([0x00, 0x55, 0xAA], np.uint8)[rng.integers(0, 3, n_bytes * 4)].tobytes())
    if kind == "4-bit codes":
        lit = lens_of({**{17 * k: 4 for k in range(15)}, 256: 4}, 257)
        return lit, [0], lits((rng.integers(0, 15, n_bytes * 2) * 17).astype(np.uint8).tobytes())
    if kind == "8-bit codes":
        lit = [8] * 255 + [0, 8]
        return lit, [0], lits(rng.integers(0, 255, n_bytes, dtype=np.uint8).tobytes())
    lit = lens_of({0x00: 2, 0xFF: 2, 257: 2, 256: 2}, 258)                                    # 2-bit literals, 2 + 2-bit matches of length 3
    n = n_bytes * 3
    rows = lits(np.array([0x00, 0xFF], np.uint8)[rng.integers(0, 2, n)].tobytes())
    is_match = rng.random(n) < 0.35
    is_match[:8] = False
    rows[is_match] = np.stack([np.full(int(is_match.sum()), 257), np.zeros(int(is_match.sum()), np.int64), rng.integers(0, 4, int(is_match.sum())), np.zeros(int(is_match.sum()), np.int64)], 1)
    return lit, [2, 2, 2, 2], rows


FILLER = lens_of({0: 1, 256: 1}, 257)                # a block of k 1-bit literals (zero bytes) and a 1-bit end-of-block: moves what follows by k bits


def speculation_cases():
    out = []
    for f, kind in enumerate(("2-bit codes", "4-bit codes", "8-bit codes", "even tokens with matches")):
        for phase in range(8):
            rng = np.random.default_rng(300 + 8 * f + phase)
            lit, dist, tok = _never_resyncs(kind, rng, 2 * ROUND_BYTES + 700)
            tok[0] = (0, 0, -1, 0)
            s = Stream()
            if f == 0 and phase == 0:
                s.stored(b"")                        # (once: an empty stored block in front, the header on a byte boundary)
            kw = header_on_phase(s.w.nbits, phase, lit, dist)
            s.dynamic(tok, lit, kw.pop("dist_lens"), final=1, **kw)
            out.append(s.case(f"never resynchronises: {kind}, phase {phase}", "the sweep loop: where the phase is no multiple of the token length a lane's speculative chain never "
                              "meets the true one, and the lanes are walked again from their predecessor's exit one per turn (2 kT turns are the proven bound; turn > 4 kT must not "
                              "fire).  The stream's first Huffman block: all kT lanes are awake in each of its rounds, two full ones and a short third", family=kind))
    rng = np.random.default_rng(340)
    s = Stream()
    lit8 = [8] * 255 + [0, 8]
    lit56 = lens_of({**{k: 5 for k in range(20)}, **{k: 6 for k in range(20, 43)}, 256: 6}, 257)
    s.dynamic(lits(b"whip!"), lens_of({**{c: 3 for c in b"whip!"}, 256: 3, 0: 3, 1: 3}, 257), [0])
    s.dynamic(lits(rng.integers(0, 255, 3 * ROUND_BYTES + 100, dtype=np.uint8).tobytes()), lit8, [0])
    s.dynamic(lits(b"x"), lens_of({ord("x"): 1, 256: 1}, 257), [0])
    s.dynamic(lits(rng.integers(0, 43, 2 * ROUND_BYTES * 8 // 5, dtype=np.uint8).tobytes()), lit56, [0], final=1)
    out.append(s.case("block-size whiplash", "the `awake` estimate from last_block_bits: a 5-token block, then 98 KB (three rounds' worth, taken a wave of lanes at a time: the short block in front narrows every round), "
                      "one token (all lanes awake for it), then 66 KB, narrow again -- a longer block just takes more rounds"))

    # the end-of-block code in the last valid lane of a round, and as the first token of a lane: 8-bit codes in the stream's first block (all lanes awake, the lanes
    # count from bit 0), the header padded so that the data begins on a byte boundary
    for want_lane, first_of_lane in ((LANES - 2, False), (LANES - 2, True), (LANES - 1, True), (5, True)):
        s, base = Stream(), 0
        kw = header_on_phase(0, 0, lit8, [0])
        probe = Stream().dynamic(lits(b""), lit8, kw["dist_lens"], **{k: v for k, v in kw.items() if k != "dist_lens"})
        data0 = probe.meta["data_begin"][-1]
        n = (want_lane * LANE_BITS + (0 if first_of_lane else 96) - data0) // 8
        rng = np.random.default_rng(350 + want_lane + first_of_lane)
        s.dynamic(lits(rng.integers(0, 255, n, dtype=np.uint8).tobytes()), lit8, kw.pop("dist_lens"), **kw)
        eob = s.meta["eob_at"][-1]
        s.fixed(lits(b"behind the round"), final=1)
        out.append(s.case(f"end-of-block in lane {want_lane}" + (", the lane's first token" if first_of_lane else ""), "nvalid = first_stop + 1 against last_lane = kT - 1: the stop in the "
                          "round's last valid lane (1022), in the lane that is never part of a round (1023), and a lane whose map holds the end-of-block code alone",
                          eob_lane=(eob - base) // LANE_BITS, eob_bit_in_lane=(eob - base) % LANE_BITS))

    cap = lens_of({0x5A: 2, 257: 1, 256: 2}, 258)
    out.append(Stream().dynamic(cat(lits(b"\x5a"), matches([3] * 40000, 1)), cap, [1], final=1)
               .case("40 000 tokens in one round", "the token cut: tok_incl > kTokCap cuts the round at a lane (C_CUT, was_cut); 2-bit matches cannot pair"))
    return out


def byte_cases():
    out = []
    cycle = np.array([1, 31, 32, 33, 4096, 32768])
    for length in (32, 31, 33):
        rng = np.random.default_rng(400 + length)
        s = Stream().fixed(cat(history_tokens(HISTORY), lits(rng.integers(0, 256, 64, dtype=np.uint8).tobytes()), matches([length] * 2000, cycle[np.arange(2000) % 6])), final=1)
        out.append(s.case(f"2 000 matches of length {length}", "the token pass: slot >= kLongCap -- a tile of 32-byte matches holds 896, the list 768, the rest take the per-byte from[] loop; "
                          "31: none is long; 33: the tiles cut some below kLongMin"))
    seed = bytes(range(65, 81))
    for n in (70, 130, 1030):
        for length, dist, how in ((5, 9, "len < dist"), (8, 8, "len == dist"), (20, 3, "len > dist")):
            out.append(Stream().fixed(cat(lits(seed), matches([length] * n, dist)), final=1)
                       .case(f"{n} matches of one distance, {how}", "goes_on / RUN_STEP: a run's first token is looked for among the wave's 64 tokens; runs across waves and lanes", run=n))
    out.append(Stream().fixed(cat(lits(seed), matches([6] * 100, 7), lits(b"#"), matches([6] * 100, 7)), final=1)
               .case("a literal inside a same-distance run", "goes_on needs the token right in front to be a match", run=100))
    out.append(Stream().fixed(cat(lits(seed), matches([6] * 100, 7), matches([6] * 100, 8)), final=1)
               .case("the distance changes by 1 inside a run", "goes_on compares distances: the second run has its own root", run=100))
    out.append(Stream().fixed(cat(lits(seed), matches([258] * 1030, 7)), final=1).case("a same-distance run across tiles", "root > o0 ? root : o0: a run that began in front of the tile "
               "copies from the tile's edge", run=1030))
    out.append(Stream().fixed(cat(lits(seed), matches([4] * 24000, 5)), final=1).case("a same-distance run across rounds", "the first match of a round has no token in front of it", run=24000))
    out.append(Stream().fixed(cat(lits(b"abc"), matches([3] * 9000, 3)), final=1).case("9 000 matches of length 3 at distance 3", "one tile, one run: every byte points at the three literals", run=9000))
    rng = np.random.default_rng(410)
    lengths = rng.integers(3, 7, 9000)
    out.append(Stream().fixed(cat(lits(b"abcdef"), matches(lengths, np.concatenate([[6], lengths[:-1]]))), final=1)
               .case("9 000 matches, each copying the one before", "resolve_copies: a chain of 9 000 dependent copies is done after log2 rounds of pointer doubling (at most 20)"))

    for produced in (1, 2, 32767, 32768):
        s = Stream().fixed(cat(history_tokens(produced), matches(7, produced), lits(b"after")), final=1)
        out.append(s.case(f"distance {produced} with {produced} bytes produced", "too_far: dist > produced0 + at is the first illegal distance"))
        if produced < 32768:
            s = Stream().fixed(history_tokens(produced), eob=False)
            s.w.array(token_bits(matches(7, produced + 1), FIXED_LIT, FIXED_DIST)); s.w.code(0, 7); s.header(1, 1); s.w.code(0, 7)
            out.append(s.case(f"distance {produced + 1} with {produced} bytes produced", "too_far -> E_DISTANCE", status=E_DISTANCE))
    out.append(Stream().fixed(cat(history_tokens(40000), matches(100, 32768), history_tokens(30000)[251:], matches(258, 32768), matches(40, 32767)), final=1)
               .case("distance 32 768 behind 40 000 and 70 000 bytes", "the ring: the 32 KiB history survives a tile (kNewMax), produced0 >= kHist skips too_far"))
    rng = np.random.default_rng(420)
    out.append(Stream().stored(rng.integers(0, 256, 300, dtype=np.uint8).tobytes()).fixed(cat(matches([10, 258, 4], [300, 150, 1]), lits(b"z"), matches(30, 311)), final=1)
               .case("a match into a stored block's bytes", "the stored bytes go through the ring: they are window history for the block behind"))
    return out


def stored_cases():
    out = []
    rng = np.random.default_rng(500)
    out.append(Stream().stored(b"", final=1).case("stored, LEN 0", "the stored loop runs zero times"))
    out.append(Stream().stored(b"\x81", final=1).case("stored, LEN 1", "one byte"))
    out.append(Stream().stored(rng.integers(0, 256, 65535, dtype=np.uint8).tobytes(), final=1).case("stored, LEN 65 535", "three pieces of kNewMax at the most"))
    s = Stream()
    for k in range(8):
        s.dynamic(lits(bytes(k)), FILLER, [0]).stored(rng.integers(0, 256, 5 + k, dtype=np.uint8).tobytes(), final=int(k == 7))
    out.append(s.case("stored blocks behind Huffman blocks that end on every bit of a byte", "p = (pos + 7) >> 3"))
    out.append(Stream().stored(b"one").stored(b"").stored(b"three", final=1).case("three stored blocks in a row", "block headers on byte boundaries"))
    out.append(Stream().stored(b"abcde", final=1, nlen=0xFEFA).case("stored, a bad NLEN", "len != (nlen ^ 0xFFFF)", status=E_STORED))
    out.append(Stream().stored(b"abcde", final=1, cut=3).case("stored, the bytes cut short", "p + 4 + len > src_len", status=E_INPUT))
    s = Stream(); s.header(1, 0); s.w.align(); s.w.bits(5, 8)
    out.append(s.case("stored, the header cut inside LEN", "p + 4 > src_len", status=E_INPUT))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = code_table_cases() + code_length_cases() + speculation_cases() + byte_cases() + stored_cases()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def by_name(name):
    return next(c for c in cases() if c.name == name)
