"""A position-parallel model of SQZ's read side in numpy: what the device reader (gamut_amd/csrc/sqz_read.hip) computes, without its
windows and lanes.  The chain of (band, bit plane) segments is walked serially; INSIDE a segment nothing is: every bit position of a
sorting pass is classified by its parity from the pass's start, every record's run comes from the 32 data bits in front of its closing
flag and from where the flag before it lies, the targets are a prefix sum of advances, and the first target past the list ends the
pass.  A refinement pass is one bit per LSP entry.  coeffs(file) -> None for a refused header, else (int16 coefficients, info): the
buffer behind SQZ_decode_round_coefficients, to be compared with sqz_ref_c.coeffs."""
import numpy as np

import sqz_ref
import sqz_ref_c as R


def _bands(info):
    """Coder::layout: {(plane, level, o): [base, w, h, stride, round]}"""
    W, H, L, mode = info["width"], info["height"], info["levels"], info["color_mode"]
    out = {}
    for p in range(info["planes"]):
        w, h = W, H
        for level in range(L - 1, -1, -1):
            for o in range(1 if level > 0 else 0, 4):
                stride = W << (L - level)
                base = p * W * H + (((w + 1) >> 1) if o & 1 else 0) + ((stride >> 1) if o > 1 else 0)
                out[p, level, o] = dict(base=base, w=(w + (0 if o & 1 else 1)) >> 1, h=(h + (0 if o > 1 else 1)) >> 1, stride=stride,
                                        round=sqz_ref.schedule(mode, p, level, o) + (info["subsampling"] & int(p > 0)))
            w, h = (w + 1) >> 1, (h + 1) >> 1
    return out


def sorting_pass(bits, s, n):
    """the pass that starts at bit s over a LIP of n entries -> (targets applied, their signs, position behind the pass, closed?)"""
    N = len(bits)
    flags = s + 1 + 2 * np.flatnonzero(bits[s + 1:N:2]).astype(np.int64)
    if (N - s) & 1:
        flags = np.append(flags, N)                                         # the end rule: the stream ends where a flag is due
    if not len(flags):
        return flags, flags, N, False
    prev = np.concatenate(([s - 1], flags[:-1]))
    k = (flags - prev - 2) // 2
    even = bits[s:N:2].astype(np.uint64)                                    # signs and run data, by (position - s) / 2
    last32 = np.zeros(len(even) + 1, np.uint64)                             # [e]: the 32 even-offset bits that end at index e
    for i in range(min(32, len(even))):
        last32[i:len(even)] |= even[:len(even) - i] << np.uint64(i)
    data = last32[(flags - 1 - s) // 2]
    kk = np.minimum(k, 32).astype(np.uint64)
    run = np.where(k >= 32, data, (np.uint64(1) << kk) | (data & ((np.uint64(1) << kk) - np.uint64(1)))) & np.uint64(0xFFFFFFFF)
    advance = ((run.astype(np.int64) - 1) & 0xFFFFFFFF) + 1                 # run 0 advances 2^32
    target = np.cumsum(advance) - 1
    over = np.flatnonzero(target >= n)
    count = over[0] if len(over) else len(flags)
    signs = even[(prev[:count] + 1 - s) // 2].astype(np.int64)
    if len(over):
        return target[:count], signs, int(flags[over[0]]) + 1, True
    return target[:count], signs, N, False


def coeffs(data):
    v, info = R.header(data)
    if v != R.OK:
        return None
    bits = np.unpackbits(np.frombuffer(data, np.uint8))
    N = len(bits)
    co = np.zeros(info["planes"] * info["width"] * info["height"], np.uint16)
    bands = _bands(info)
    for b in bands.values():
        b.update(lip=None, lsp=np.zeros(0, np.int64), bitplane=0, max_bitplane=0)
    idle = dict(round=0, bitplane=0)
    pos = 48
    planes, L = info["planes"], info["levels"]

    def visit(b, first):
        nonlocal pos
        if first:
            if (pos & 7) > 4 and (pos >> 3) + 1 >= len(data):
                b["max_bitplane"] = b["bitplane"] = -1
                pos = N
            else:
                b["max_bitplane"] = b["bitplane"] = int(bits[pos:pos + 4] @ (8, 4, 2, 1))
                pos += 4
            xy = R.scan(info["scan_order"], b["w"], b["h"]).astype(np.int64)
            b["lip"] = b["base"] + xy[:, 1] * b["stride"] + xy[:, 0]       # the entries as coefficient indices
        bp, nsp = b["bitplane"], np.zeros(0, np.int64)
        if len(b["lip"]) and bp > 0:
            target, signs, pos, closed = sorting_pass(bits, pos, len(b["lip"]))
            nsp = b["lip"][target]
            co[nsp] |= np.uint16(1 << bp) | signs.astype(np.uint16)
            if not closed or pos >= N:
                return False
            keep = np.ones(len(b["lip"]), bool)
            keep[target] = False
            b["lip"] = b["lip"][keep]
        m = min(len(b["lsp"]), max(N - pos, 0))
        co[b["lsp"][:m][bits[pos:pos + m] == 1]] |= np.uint16(1 << (bp & 15))
        pos += m
        if m < len(b["lsp"]) or pos >= N:
            return False
        b["lsp"] = np.concatenate((b["lsp"], nsp))
        b["bitplane"] -= bp > 0
        return True

    state = plane = level = o = 0
    rnd, done, stop = 0, False, False
    while not done and pos < N and not stop:                                # SQZ_schedule_task
        done = True
        while True:
            b = bands.get((plane, level, o), idle)
            if rnd < b["round"] or (rnd > b["round"] and b["bitplane"] == 0):
                done = done and rnd > b["round"]
            else:
                if not visit(b, b["round"] == rnd):
                    stop = True
                    break
                done = done and b["bitplane"] == 0
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
    for b in bands.values():                                                # SQZ_decode_round_coefficients: merged entries only
        if b["max_bitplane"] != 0 and b["bitplane"] >= 2:
            co[b["lsp"]] |= np.uint16(((1 << b["bitplane"]) - 1) ^ 1)
    return co.view(np.int16), info


def mutations(count, seed=20):
    """seeded mutations of small files: truncation plus a random, all-zero or all-one tail, and bit flips"""
    import sqz_cases
    rng = np.random.default_rng(seed)
    seeds = [f for _, f, e in sqz_cases.small_cases() if e == "ok" and 40 <= len(f) <= 1200]
    out = []
    for k in range(count):
        f = bytearray(seeds[k % len(seeds)])
        if k % 4 == 3:
            for _ in range(int(rng.integers(1, 6))):
                f[int(rng.integers(6, len(f)))] ^= 1 << int(rng.integers(0, 8))
        else:
            del f[int(rng.integers(7, len(f) + 1)):]
            n = int(rng.integers(0, 200))
            f += (bytes(rng.integers(0, 256, n, dtype=np.uint8)), bytes(n), b"\xff" * n)[k % 4]
        out.append(bytes(f))
    return out
