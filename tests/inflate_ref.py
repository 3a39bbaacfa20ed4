"""A plain inflate written from RFC 1951, and a census of what a stream holds.  Deliberately naive: a code is found by walking the
stream bit by bit against the counts of the canonical code (no lookup tables), a match is copied byte by byte.  It is the second opinion
on zlib for the constructed streams of tests/inflate_cases.py, and its census is what turns "this case reaches that line of
gamut_amd/csrc/inflate.hip" into something a test can check (tests/test_inflate_cases_cpu.py).

inflate(data) -> (bytes, Census), or raises InflateError whose `reason` is one of REASONS -- the names of GAMUT_HIP_INFLATE_E_*.
Accepts and rejects what zlib's inflate does: an incomplete literal / length or distance code only if its longest code is one bit, a
complete code-length code only, a block without an end-of-block code never, trailing bytes behind the final block always.

memo=True remembers every code the naive walk has found, keyed by the 15 stream bits it began at: the same answers, some ten times faster
on megabytes of encoder output (the census of the existing suite)."""
import collections

import numpy as np

REASONS = ("block type", "stored", "lengths", "code", "distance", "input")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

ROUND_BYTES = 32768          # compressed bytes the kernel takes per round (1024 lanes of 256 bits)
TILE_BYTES = 28672           # output bytes the kernel resolves per tile
LONG_MATCH = 32              # matches at least this long go to the tile's list of long matches


class InflateError(Exception):
    def __init__(self, reason, detail=""):
        assert reason in REASONS
        super().__init__(f"{reason}: {detail}" if detail else reason)
        self.reason = reason


class Census:
    """what the stream held.  Per stream: blocks (one dict per block: type, and for a dynamic block hlit, hdist, hclen, cl_bits = the bit
    length of its code-length stream), the maxima over them, max_lit_len / max_dist_len = the longest literal / length and distance code
    a token USED, len_syms / dist_syms = the symbols used, spelled_258_as_284 = length 258 written as symbol 284 + 31, tokens, rounds = the
    32 KiB rounds the Huffman blocks need (a block's bits over ROUND_BYTES, rounded up), max_round_tokens = the most tokens that begin
    within ROUND_BYTES of input counted from a block's first token, max_same_dist_run = the longest run of consecutive matches of one
    distance, max_long_per_tile = the most matches of LONG_MATCH bytes or more that begin within one span of TILE_BYTES of output."""

    def __init__(self):
        self.blocks = []
        self.max_lit_len = self.max_dist_len = 0
        self.len_syms, self.dist_syms = set(), set()
        self.spelled_258_as_284 = 0
        self.tokens = self.rounds = self.max_round_tokens = 0
        self.max_same_dist_run = self.max_long_per_tile = 0
        self.max_cl_bits = 0
        self.hlit, self.hdist, self.hclen = set(), set(), set()
        self.dist_code_sizes = set()      # number of distance codes of each dynamic block (0: a block with none)

    def merge(self, other):
        self.blocks += other.blocks
        for k in ("max_lit_len", "max_dist_len", "max_round_tokens", "max_same_dist_run", "max_long_per_tile", "max_cl_bits"):
            setattr(self, k, max(getattr(self, k), getattr(other, k)))
        for k in ("len_syms", "dist_syms", "hlit", "hdist", "hclen", "dist_code_sizes"):
            getattr(self, k).update(getattr(other, k))
        for k in ("spelled_258_as_284", "tokens", "rounds"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        return self


class _Code:
    """a canonical code: count[l] codes of length l, the symbols in canonical order"""

    def __init__(self, lengths, what):
        self.count = [0] * 16
        for l in lengths:
            self.count[l] += 1
        self.symbols = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]
        self.max = max(lengths) if lengths else 0
        left = 1
        for l in range(1, 16):
            left = 2 * left - self.count[l]
            if left < 0:
                raise InflateError("lengths", f"over-subscribed {what} code")
        self.incomplete = left > 0
        self.memo = {}


class _Reader:
    def __init__(self, data, memo):
        arr = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")
        self.n = arr.size
        self.bits = arr.tobytes() + bytes(16)
        self.pos = 0
        self.win = None
        if memo:
            padded = np.concatenate([arr, np.zeros(16, np.uint8)]).astype(np.uint16)
            w = np.zeros(self.n + 1, np.uint16)
            for i in range(15):
                w |= padded[i:i + self.n + 1] << i
            self.win = w

    def take(self, n):
        if self.pos + n > self.n:
            raise InflateError("input", "the stream ends inside a field")
        v = 0
        for i in range(n):
            v |= self.bits[self.pos + i] << i
        self.pos += n
        return v

    def symbol(self, code):
        """-> (symbol, code length)"""
        if self.win is not None:
            hit = code.memo.get(int(self.win[self.pos]))
            if hit is not None:
                if self.pos + hit[1] > self.n:
                    raise InflateError("input", "the stream ends inside a code")
                self.pos += hit[1]
                return hit
            key = int(self.win[self.pos])
        value = first = index = 0
        for l in range(1, 16):
            if self.pos + l > self.n:
                raise InflateError("input", "the stream ends inside a code")
            value |= self.bits[self.pos + l - 1]
            cnt = code.count[l]
            if value - cnt < first:
                self.pos += l
                hit = (code.symbols[index + value - first], l)
                if self.win is not None:
                    code.memo[key] = hit
                return hit
            index += cnt
            first = (first + cnt) << 1
            value <<= 1
        raise InflateError("code", "no code matches")


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _dynamic_header(r, block):
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    block.update(hlit=hlit, hdist=hdist, hclen=hclen)
    if hlit > 286 or hdist > 30:
        raise InflateError("lengths", "too many length or distance symbols")
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = r.take(3)
    code = _Code(cl, "code-length")
    if code.incomplete:
        raise InflateError("lengths", "incomplete code-length code")
    lens, begin = [], r.pos
    while len(lens) < hlit + hdist:
        s, _ = r.symbol(code)
        if s < 16:
            lens.append(s)
            continue
        if s == 16 and not lens:
            raise InflateError("lengths", "repeat with nothing to repeat")
        rep, val = (3 + r.take(2), lens[-1]) if s == 16 else (3 + r.take(3), 0) if s == 17 else (11 + r.take(7), 0)
        if len(lens) + rep > hlit + hdist:
            raise InflateError("lengths", "repeat past the last length")
        lens += [val] * rep
    block["cl_bits"] = r.pos - begin
    if lens[256] == 0:
        raise InflateError("lengths", "no end-of-block code")
    lit, dist = _Code(lens[:hlit], "literal / length"), _Code(lens[hlit:], "distance")
    for c, what in ((lit, "literal / length"), (dist, "distance")):
        if c.incomplete and c.max > 1:
            raise InflateError("lengths", f"incomplete {what} code")
    block["dist_codes"] = sum(dist.count[1:])
    return lit, dist


def inflate(data, memo=False):
    r = _Reader(bytes(data), memo)
    out = bytearray()
    cs = Census()
    long_starts = collections.deque()
    fixed = None
    final = 0
    while not final:
        final, btype = r.take(1), r.take(2)
        block = {"type": btype, "at_bit": r.pos - 3}
        cs.blocks.append(block)
        if btype == 3:
            raise InflateError("block type")
        if btype == 0:
            r.pos = (r.pos + 7) & ~7
            if r.pos + 32 > r.n:
                raise InflateError("input", "the stream ends inside LEN / NLEN")
            length, nlen = r.take(16), r.take(16)
            if length != nlen ^ 0xFFFF:
                raise InflateError("stored", "LEN and NLEN disagree")
            at = r.pos >> 3
            if at + length > len(data):
                raise InflateError("input", "the stored bytes are cut short")
            out += data[at:at + length]
            r.pos += 8 * length
            block["len"] = length
            continue
        if btype == 1:
            if fixed is None:
                fixed = _Code(FIXED_LIT, "fixed"), _Code(FIXED_DIST, "fixed")
            lit, dist = fixed
        else:
            lit, dist = _dynamic_header(r, block)
            cs.hlit.add(block["hlit"]); cs.hdist.add(block["hdist"]); cs.hclen.add(block["hclen"])
            cs.max_cl_bits = max(cs.max_cl_bits, block["cl_bits"])
            cs.dist_code_sizes.add(block["dist_codes"])
        begin = r.pos
        round_end, round_tokens = begin + 8 * ROUND_BYTES, 0
        run, run_dist, tokens = 0, 0, 0
        while True:
            if r.pos >= round_end:
                cs.max_round_tokens = max(cs.max_round_tokens, round_tokens)
                round_end, round_tokens = round_end + 8 * ROUND_BYTES, 0
            s, l = r.symbol(lit)
            if l > cs.max_lit_len:
                cs.max_lit_len = l
            if s == 256:
                break
            tokens += 1; round_tokens += 1
            if s < 256:
                out.append(s)
                run = 0
                continue
            if s > 285:
                raise InflateError("code", f"literal / length symbol {s}")
            x = r.take(LEN_EXTRA[s - 257])
            length = LEN_BASE[s - 257] + x
            cs.len_syms.add(s)
            if s == 284 and x == 31:
                cs.spelled_258_as_284 += 1
            d, l = r.symbol(dist)
            if l > cs.max_dist_len:
                cs.max_dist_len = l
            if d > 29:
                raise InflateError("code", f"distance symbol {d}")
            cs.dist_syms.add(d)
            distance = DIST_BASE[d] + r.take(DIST_EXTRA[d])
            if distance > len(out):
                raise InflateError("distance", f"distance {distance} with {len(out)} bytes produced")
            run = run + 1 if run and distance == run_dist else 1
            run_dist = distance
            if run > cs.max_same_dist_run:
                cs.max_same_dist_run = run
            if length >= LONG_MATCH:
                at = len(out)
                long_starts.append(at)
                while at - long_starts[0] >= TILE_BYTES:
                    long_starts.popleft()
                if len(long_starts) > cs.max_long_per_tile:
                    cs.max_long_per_tile = len(long_starts)
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
        cs.max_round_tokens = max(cs.max_round_tokens, round_tokens)
        cs.tokens += tokens
        cs.rounds += max(1, -(-(r.pos - begin) // (8 * ROUND_BYTES)))
        block.update(tokens=tokens, bits=r.pos - begin, begin_bit=begin)
    return bytes(out), cs
