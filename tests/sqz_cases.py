"""Named SQZ test files as (name, bytes, expectation), expectation "ok" or "refused" (what SQZ_decode's header stage says; a file that
passes it always decodes: the stream is embedded, every prefix of at least 7 bytes of a good file is a good file).  Files are made with
the restated encoder (tests/c/sqz_ref.c) or bit by bit.

A note on the smallest sides: SQZ_validate_input allows ilog2(min side) - 3 levels with ilog2 = bsr + 1, which is ONE level for a side
of 8..15 (ilog2 = 4).  Such files are accepted by the reference and here; two levels are refused, and so is a side of 7."""
import functools

import numpy as np

import sqz_ref_c as R

MODES = ("grey", "ycocg", "oklab", "logl1")
SCANS = ("raster", "snake", "morton", "hilbert")


def picture(w, h, planes, seed):
    """smooth ramps, an edge and some noise: every subband gets coefficients on several bit planes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    chans = []
    for c in range(planes):
        v = (xx * (3 + c) + yy * (5 - c)) % 256
        v = np.where((xx + c * 3) % 17 < 8, v, 255 - v) // 2 + rng.integers(0, 128, (h, w))
        chans.append(v.astype(np.uint8))
    return np.ascontiguousarray(chans[0] if planes == 1 else np.stack(chans, 2))


def make(w, h, mode, levels, scan=R.SNAKE, subsampling=0, budget=None, seed=0):
    return R.encode(picture(w, h, 1 if mode == R.GREY else 3, seed), mode, levels, scan, subsampling, budget)


# ---- files by hand ----
def header_bits(w, h, mode, levels, scan, subsampling):
    v = 0xA5 << 40 | (w - 1) << 24 | (h - 1) << 8 | mode << 6 | (levels - 1) << 3 | scan << 1 | subsampling
    return [(v >> (47 - k)) & 1 for k in range(48)]


def header_bytes(w, h, mode=0, levels=1, scan=0, subsampling=0):
    return pack(header_bits(w, h, mode, levels, scan, subsampling))


def run_code(run):
    """what SQZ_decode_read_wdr_run reads as `run` (before its 32-bit wrap): a 0 in front of every bit below the top one, then a 1"""
    bits = []
    for b in bin(run)[3:]:
        bits += [0, int(b)]
    return bits + [1]


def pack(bits, pad=0):
    bits = list(bits)
    bits += [pad] * (-len(bits) % 8)
    return bytes(int("".join(map(str, bits[k:k + 8])), 2) for k in range(0, len(bits), 8))


def nibble(v):
    return [(v >> 3) & 1, (v >> 2) & 1, (v >> 1) & 1, v & 1]


def hand_set():
    """16 x 16 grey, one level, raster scan: round 0 is the 8 x 8 LL band alone"""
    hd = header_bits(16, 16, 0, 1, 0, 0)
    out = []
    # bit plane 15: 1 << 15 is the sign bit of a short; three coefficients, then a run past the 64-entry LIP ends the pass
    bits = hd + nibble(15) + [1] + run_code(1) + [0] + run_code(5) + [1] + run_code(2) + [0] + run_code(100)
    out.append(("hand_max_bitplane_15", pack(bits) + b"\xff\x0f\xf0\x55\xaa" * 8))
    bits = hd + nibble(9) + [0] + run_code(3) + [1] + run_code(1000)
    out.append(("hand_run_overshoots_the_lip", pack(bits) + b"\xc3\x5a" * 12))
    # 2^32 + 3 in 33 bits: the 32-bit accumulator keeps 3, so the run lands on the third entry
    bits = hd + nibble(11) + [1] + run_code(2 ** 32 + 3) + [0] + run_code(2) + [1] + run_code(2 ** 33 + 2 ** 32 + 7) + [0] + run_code(200)
    out.append(("hand_run_accumulator_wraps", pack(bits) + b"\x9d\x37" * 12))
    # the stream ends inside the FIRST sorting pass of the band: its NSP is never merged, so those coefficients are not rounded
    bits = hd + nibble(6)
    for k in range(9):
        bits += [k & 1] + run_code(1 + k % 3)
    out.append(("hand_ends_inside_a_sorting_pass", pack(bits)))      # (padding zeros, if any: a run still being read)
    # plane 6 completes (five coefficients, an overshooting run closes the sorting pass, the LSP is still empty), round 1 starts plane 5
    # with one more coefficient and a closing run, and the stream ends after two of the refinement bits
    bits = hd + nibble(6)
    for k in range(5):
        bits += [k & 1] + run_code(2)
    bits += [0] + run_code(90)
    bits += [1] + run_code(4) + [0] + run_code(77)
    while (len(bits) + 2) % 8:                                     # one more coefficient in the first pass until the byte boundary lies behind the second refinement bit
        bits = bits[:52] + [0] + run_code(1) + bits[52:]
    out.append(("hand_ends_inside_a_refinement_pass", pack(bits + [1, 0])))
    return [(n, f, "ok") for n, f in out]


@functools.lru_cache(maxsize=None)
def small_cases():
    c = []
    ok, bad = "ok", "refused"
    base = make(16, 16, R.GREY, 1)
    # ---- header refusals
    c.append(("header_wrong_magic", b"\xa4" + base[1:], bad))
    for n in range(7):
        c.append((f"header_length_{n}", base[:n], bad))
    c.append(("header_six_bytes_and_one", base[:7], ok))
    c.append(("header_side_7", header_bytes(7, 16) + base[6:40], bad))
    c.append(("header_side_7_high", header_bytes(16, 7) + base[6:40], bad))
    c.append(("header_width_65536", header_bytes(65536, 16) + base[6:40], bad))
    c.append(("header_side_15_two_levels", header_bytes(15, 15, levels=2) + base[6:40], bad))
    c.append(("header_side_8_two_levels", header_bytes(8, 8, levels=2) + base[6:40], bad))
    c.append(("header_16x16_three_levels", header_bytes(16, 16, levels=3) + base[6:40], bad))
    c.append(("header_64x40_four_levels", header_bytes(64, 40, levels=4) + base[6:40], bad))
    c.append(("header_256x256_seven_levels", header_bytes(256, 256, levels=7) + base[6:40], bad))
    c.append(("header_2048x31_three_levels", header_bytes(2048, 31, levels=3) + base[6:40], bad))
    # one level on a side of 8..15: accepted by SQZ_validate_input (module docstring)
    c.append(("side_15_one_level", make(15, 15, R.YCOCG, 1, R.HILBERT, seed=3), ok))
    c.append(("side_8_one_level", make(8, 8, R.GREY, 1, R.MORTON, seed=4), ok))
    c.append(("side_8x13_one_level_oklab", make(8, 13, R.OKLAB, 1, R.SNAKE, 1, seed=5), ok))
    # ---- every colour mode x scan order, 16 x 16, one level; subsampling alternates
    for m in range(4):
        for s in range(4):
            c.append((f"mode_{MODES[m]}_scan_{SCANS[s]}", make(16, 16, m, 1, s, (m + s) & 1, seed=10 + 4 * m + s), ok))
    # ---- geometries: the mirror and the odd tails of both passes
    k = 0
    for (w, h, lv) in ((16, 16, 1), (17, 16, 1), (16, 17, 1), (19, 23, 1), (31, 33, 1), (32, 33, 2), (47, 32, 2), (64, 40, 2), (128, 72, 4), (256, 256, 5)):
        for m in ((0, 1, 2, 3) if w * h < 2000 else ((k % 4), 2)):
            c.append((f"geometry_{w}x{h}_{lv}_levels_{MODES[m]}", make(w, h, m, lv, (k + m) % 4, k & 1, seed=100 + k), ok))
        k += 1
    c.append(("geometry_64x40_3_levels_oklab", make(64, 40, R.OKLAB, 3, R.SNAKE, 1, seed=120), ok))
    c.append(("geometry_300x130_5_levels_logl1", make(300, 130, R.LOGL1, 5, R.HILBERT, 0, seed=121), ok))    # more than one tile in both directions
    # ---- budgets: header plus one byte .. lossless
    full = make(47, 32, R.OKLAB, 2, R.SNAKE, 1, seed=7)
    fullg = make(47, 32, R.GREY, 2, R.MORTON, 0, seed=8)
    for b in (7, 8, 9, 16, 40, 100, 300, 1000, len(full) // 2, len(full) - 1):
        c.append((f"budget_{b}_oklab", make(47, 32, R.OKLAB, 2, R.SNAKE, 1, budget=b, seed=7), ok))
        assert c[-1][1] == full[:b]                                 # the embedded property on the encoder's side
    for b in (7, 12, 33, 150, 700, len(fullg) - 3):
        c.append((f"budget_{b}_grey", make(47, 32, R.GREY, 2, R.MORTON, 0, budget=b, seed=8), ok))
    c.append(("budget_lossless_oklab", full, ok))
    c.append(("budget_lossless_grey", fullg, ok))
    c += hand_set()
    return c


@functools.lru_cache(maxsize=None)
def prefix_files():
    """two small files whose every prefix from 7 bytes on is a case: (grey, oklab)"""
    return make(16, 16, R.GREY, 1, R.HILBERT, 0, seed=31), make(16, 17, R.OKLAB, 1, R.SNAKE, 1, seed=32)


def prefixes(f, step=1):
    return [f[:n] for n in range(7, len(f) + 1, step)]


@functools.lru_cache(maxsize=None)
def big_case():
    """2048 x 2048 grey, 8 levels, a small budget: a short stream under a deep IDWT"""
    return make(2048, 2048, R.GREY, 8, R.SNAKE, 0, budget=6000, seed=77)


def tiny_files(count=600):
    rng = np.random.default_rng(5)
    files = []
    for k in range(count):
        w, h = int(rng.integers(16, 25)), int(rng.integers(16, 25))
        files.append(make(w, h, k % 4, 1 + k % 2, (k // 4) % 4, (k // 16) & 1, budget=None if k % 3 else 40 + k % 90, seed=1000 + k))
    return files
