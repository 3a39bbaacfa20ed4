"""QOI streams for the decode kernels (gamut_amd/csrc/qoi.hip), each named for what it is about: a builder that writes a file from a
header and a list of ops, the constructed cases, and the arbitrary streams no encoder writes.  The geometry the cases are laid out
against -- window, bytes per lane of the one-wave kernel, the pixel-buffer threshold, the batch thresholds -- is read from the kernels'
source (the library has no query for it yet), never written down here.  tests/test_qoi_cases_cpu.py checks, without a GPU, that every
property a case is named for is really in its bytes, and the oracle against a second decoder on all of them.  On the GPU every case,
constructed and arbitrary, goes through all three decode kernels at output channels 0, 3 and 4 in tests/test_qoi_batch_gpu.py (laid
out by tests/qoi_batch.py); the arbitrary streams also run in tests/test_qoi_gpu.py."""
import collections
import functools
import os
import re

import numpy as np

import oracle_lib as O


def param(which):
    """0: window bytes (kQoiWin), 1: bytes per lane of the one-wave kernel (k_qoi_decode<1>: the window over its 64 lanes), 2: kQoiBufGroup,
    3: kQoiWideBelow, 4: the streams per launch of the host-memory entry (kGroup); anything else: -1"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gamut_amd", "csrc", "qoi.hip")).read()
    def const(name):
        found = re.findall(r"\b" + name + r" = (\d+)[,;]", src)
        assert len(found) == 1, name
        return int(found[0])
    if which == 1:
        assert re.search(r"kQoiT = kQoiWaves \* 64, kQoiLaneBytes = kQoiWin / kQoiT;", src)
        return const("kQoiWin") // 64
    names = {0: "kQoiWin", 2: "kQoiBufGroup", 3: "kQoiWideBelow", 4: "kGroup"}
    return const(names[which]) if which in names else -1


WIN, LANE, BUF_GROUP, WIDE_BELOW, HOST_GROUP = (param(k) for k in range(5))
GROUP = 64                                                             # ops per group: one per lane of a wave
HEADER = 14
PADDING = bytes(7) + b"\x01"                                           # qoi_padding (qoi.d:268)
ODD_PADDING = bytes([0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0x88])  # the decoder never checks it, and reads it as the tail of an op

Case = collections.namedtuple("Case", "name data")


def hash_of(px):
    """QOI_COLOR_HASH (qoi.d:239-242) of (r, g, b, a), modulo the table's 64 slots"""
    return (3 * px[0] + 5 * px[1] + 7 * px[2] + 11 * px[3]) & 63


def encode_ops(ops):
    out = bytearray()
    for op in ops:
        kind = op[0]
        if kind == "rgb":
            out += bytes([0xFE, op[1], op[2], op[3]])
        elif kind == "rgba":
            out += bytes([0xFF, op[1], op[2], op[3], op[4]])
        elif kind == "index":
            assert 0 <= op[1] < 64
            out.append(op[1])
        elif kind == "diff":
            assert all(-2 <= d <= 1 for d in op[1:4])
            out.append(0x40 | (op[1] + 2) << 4 | (op[2] + 2) << 2 | (op[3] + 2))
        elif kind == "luma":                                           # (dg, dr - dg, db - dg)
            assert -32 <= op[1] <= 31 and -8 <= op[2] <= 7 and -8 <= op[3] <= 7
            out += bytes([0x80 | (op[1] + 32), (op[2] + 8) << 4 | (op[3] + 8)])
        elif kind == "run":
            assert 1 <= op[1] <= 62
            out.append(0xC0 | (op[1] - 1))
        elif kind == "raw":
            out += bytes(op[1])
        else:
            raise ValueError(kind)
    return bytes(out)


def qoi_file(width, height, channels, ops, padding=PADDING):
    """a QOI file: the 14-byte header, the ops, the padding"""
    return b"qoif" + width.to_bytes(4, "big") + height.to_bytes(4, "big") + bytes([channels, 0]) + encode_ops(ops) + padding


def op_pixels(ops):
    assert all(op[0] != "raw" for op in ops)
    return sum(op[1] if op[0] == "run" else 1 for op in ops)


def _dims(npx, spare=0):
    """an image of exactly npx pixels (spare = 0), or one of at least npx + spare whose last pixels the stream does not reach"""
    if spare == 0:
        for w in range(97, 30, -1):
            if npx % w == 0:
                return w, npx // w
        return npx, 1
    return 61, (npx + spare + 60) // 61


def _filler(n, seed=0):
    """n one-byte DIFF ops, every combination of deltas in turn: the pixel drifts, no two neighbours are alike"""
    return [("diff", (i + seed) % 4 - 2, (i + seed) // 4 % 4 - 2, (i + seed) // 16 % 4 - 2) for i in range(n)]


def _ordinary(seed=0):
    """64 ops, a pixel each, of every kind but INDEX and RUN"""
    ops = _filler(GROUP, seed)
    ops[7] = ("luma", 9, -4, 3); ops[20] = ("rgb", 31 + seed, 200, 77); ops[21] = ("luma", -20, 7, -8); ops[40] = ("rgba", 5, 6, 7 + seed, 255); ops[63] = ("luma", 3, 0, -1)
    return ops


def _group(npx, seed=0):
    """64 ops that make exactly npx pixels: DIFF ops, and as many RUN ops (of 62 while they fit) as it takes, spread over the lanes"""
    assert GROUP <= npx <= GROUP * 62
    runs, extra = [], npx - GROUP
    while extra > 0:
        n = min(62, extra + 1)
        runs.append(n); extra -= n - 1
    ops = _filler(GROUP, seed)
    for j, n in enumerate(runs):
        ops[(j * GROUP) // len(runs) + (GROUP // len(runs)) // 2] = ("run", n)
    assert op_pixels(ops) == npx and len(ops) == GROUP
    return ops


def _mixed(nbytes, seed):
    """ops of every kind, in exactly nbytes bytes"""
    rng = np.random.default_rng(seed)
    ops, left = [], nbytes
    while left > 0:
        kind = ["diff", "luma", "index", "rgb", "rgba", "run"][int(rng.choice(6, p=[0.35, 0.25, 0.15, 0.1, 0.05, 0.1]))]
        size = {"luma": 2, "rgb": 4, "rgba": 5}.get(kind, 1)
        if size > left:
            continue
        v = [int(x) for x in rng.integers(0, 256, 4)]
        ops.append({"diff": ("diff", v[0] % 4 - 2, v[1] % 4 - 2, v[2] % 4 - 2), "luma": ("luma", v[0] % 64 - 32, v[1] % 16 - 8, v[2] % 16 - 8),
                    "index": ("index", v[0] % 64), "rgb": ("rgb", v[0], v[1], v[2]), "rgba": ("rgba", v[0], v[1], v[2], v[3]), "run": ("run", 1 + v[0] % 6)}[kind])
        left -= size
    assert len(encode_ops(ops)) == nbytes
    return ops


def _pal(k, v=0):
    """an RGB op whose pixel (alpha 255) lands in table slot _slot(k), whatever v: another colour for the same slot"""
    return ("rgb", k % 64 + 64 * (v % 4), 64 * (v // 4 % 4), 64 * (v // 16 % 4))


def _slot(k):
    return (3 * (k % 64) + 11 * 255) & 63


STRADDLES = ((2, 1), (4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (5, 3), (5, 4))       # (op length, bytes of it behind the boundary)
BOUNDARIES = ("window", "lane", "end")
CHUNK_LENGTHS = (0, 1, 31, 32, 33, WIN - 1, WIN, WIN + 1, 2 * WIN)
_STRADDLE_OP = {2: ("luma", -7, 3, -5), 4: ("rgb", 201, 17, 93), 5: ("rgba", 17, 201, 93, 140)}
_AFTER = [("luma", 5, -3, 2)] + _filler(37, 5) + [("rgb", 1, 2, 3), ("diff", 1, -2, 0), ("run", 3), ("luma", -1, 1, 1)]


def _straddle_cases():
    out = []
    for ch in (3, 4):
        for (length, s) in STRADDLES:
            op = _STRADDLE_OP[length]
            # the op starts s bytes before a window boundary: the first one at 3 channels; the second one at 4, behind a LUMA op that
            # already straddles the first (the entry offset is carried from window to window)
            if ch == 3:
                ops = _filler(WIN - s) + [op] + _AFTER
            else:
                ops = _filler(WIN - 1) + [("luma", 2, -1, 4)] + _filler(WIN - 1 - s, 9) + [op] + _AFTER
            w, h = _dims(op_pixels(ops), 0 if ch == 3 else 11)
            out.append(Case(f"straddle-window-L{length}-s{s}-ch{ch}", qoi_file(w, h, ch, ops)))
            # ... before a lane boundary inside a window: in the middle of the window, and between its last two lanes
            ops = _filler((37 if ch == 3 else WIN // LANE - 1) * LANE - s, 3) + [op] + _AFTER
            w, h = _dims(op_pixels(ops), 0 if ch == 4 else 7)
            out.append(Case(f"straddle-lane-L{length}-s{s}-ch{ch}", qoi_file(w, h, ch, ops)))
            # ... before the end of the chunk bytes: the op's tail is the padding (inside the first window, or across the first boundary)
            chunk = 5 * LANE + 2 if ch == 3 else WIN + 2
            ops = _filler(chunk - s, 6)
            w, h = _dims(op_pixels(ops) + 1, 9)
            out.append(Case(f"straddle-end-L{length}-s{s}-ch{ch}", qoi_file(w, h, ch, ops + [("raw", encode_ops([op])[:s])], PADDING if ch == 3 else ODD_PADDING)))
    return out


def _chunk_length_cases():
    out = []
    for k, n in enumerate(CHUNK_LENGTHS):
        ops = _mixed(n, 100 + k)
        w, h = (5, 3) if n == 0 else _dims(op_pixels(ops), 5)
        out.append(Case(f"chunk-{n}-bytes", qoi_file(w, h, 3 + (k & 1), ops)))
    return out


def _pixel_buffer_cases():
    """(three-channel outputs wait in the one-wave kernel's LDS buffer; a group of more than BUF_GROUP pixels goes round it)"""
    out = []
    def add(name, ops, spare):
        w, h = _dims(op_pixels(ops), spare)
        out.append(Case(name, qoi_file(w, h, 3, ops)))
    long_group = _group(10 * 62 + 54, 2)                             # ten RUN-62 ops among 54 DIFF ops
    assert op_pixels(long_group) > BUF_GROUP
    for waiting in (1, 255, 256):                                    # pixels in front of the long group: 257 (256 leave, 1 waits), 255, 256 (all leave)
        add(f"buffer-long-group-behind-{waiting}", _group(257 if waiting == 1 else waiting, waiting) + long_group + _ordinary(1) + _ordinary(2), 0 if waiting == 255 else 3)
    add("buffer-group-of-exactly-the-threshold", _group(255, 4) + _group(BUF_GROUP, 5) + _ordinary(3), 0)
    add("buffer-group-of-the-threshold-plus-1", _group(255, 6) + _group(BUF_GROUP + 1, 7) + _ordinary(4), 5)
    add("buffer-64-runs-of-62", _ordinary(5) + [("run", 62)] * GROUP + _ordinary(6), 0)
    add("buffer-fill-256-exactly", _group(100, 8) + _group(156, 9) + _ordinary(7), 2)
    add("buffer-fill-512-exactly", _group(100, 10) + _group(412, 11) + _ordinary(8), 0)
    return out


def _image_full_cases():
    out = []
    junk = [("rgb", 250, 1, 2), ("diff", 1, 1, 1), ("rgba", 9, 9, 9, 9), ("index", 5)] * 16
    out.append(Case("full-run-first-lane", qoi_file(12, 7, 3, _ordinary(9) + [("run", 40)] + junk[:63] + _ordinary(10))))            # 84 = 64 + 20
    out.append(Case("full-run-last-lane", qoi_file(137, 1, 4, _ordinary(11) + _filler(63, 2) + [("run", 40)] + junk)))                # 137 = 64 + 63 + 10
    out.append(Case("full-run-long-group", qoi_file(47, 20, 3, _group(255, 12) + _group(1500, 13) + _ordinary(12))))                  # 940 = 255 + 685: round the buffer
    out.append(Case("full-run-long-group-cut-below-the-threshold", qoi_file(47, 15, 3, _group(255, 12) + _group(900, 13) + _ordinary(12))))      # 705 = 255 + 450: through it
    ops = _mixed(1000, 21)
    w, h = _dims(op_pixels(ops))
    noise = np.random.default_rng(22).integers(0, 256, WIN + 300, dtype=np.uint8).tobytes()
    out.append(Case("full-then-a-window-of-noise", qoi_file(w, h, 4, ops + [("raw", noise)])))
    ops = _mixed(300, 23)
    w, h = _dims(op_pixels(ops) + 1)
    out.append(Case("ends-one-pixel-short", qoi_file(w, h, 3, ops)))
    out.append(Case("ends-after-its-first-op", qoi_file(7, 5, 4, [("rgb", 9, 8, 7)])))
    return out


def _index_cases():
    out = []
    def add(name, ch, ops, spare=4):
        w, h = _dims(op_pixels(ops), spare)
        out.append(Case(name, qoi_file(w, h, ch, ops)))
    # a slot nothing has written is (0, 0, 0, 0): alpha 0, which an RGBA output shows and an RGB output drops
    add("index-slot-never-written", 4, [("index", 17)] + _filler(3) + [_pal(1), ("index", 41), ("diff", 1, 1, 1), _pal(2), ("index", _slot(1)), ("index", 29)])
    add("index-slot-written-in-the-same-group", 3, [_pal(k) for k in range(1, 11)] + [("index", _slot(3)), _pal(11), ("index", _slot(11)), ("index", _slot(1)), ("luma", 4, 1, -2)])
    every = [_pal(k, k) for k in range(GROUP)]
    add("index-slot-written-in-the-previous-group", 4, every + [("index", _slot(5)), ("diff", 1, 0, -1), ("index", _slot(63)), _pal(6, 33), ("index", _slot(6)), ("index", _slot(40))])
    runs = WIN - 4 - 4 - 4
    add("index-slot-written-in-the-previous-window", 3, [_pal(9, 7), _pal(20, 2)] + [("run", 1)] * (runs // 2) + [_pal(21, 5)] + [("run", 2)] * (runs - runs // 2) +
        [_pal(30), ("index", _slot(9)), ("diff", -2, 1, 0), ("index", _slot(21)), ("index", _slot(20))])
    add("index-slot-written-twice-in-one-group", 4, [_pal(4, 1)] + [_pal(k, 3) for k in range(5, 5 + GROUP - 1)] +
        [("index", _slot(4)), _pal(4, 2), ("index", _slot(4)), _pal(4, 27), _pal(5), ("index", _slot(4)), ("luma", -3, 2, 2), _pal(8, 1), _pal(8, 2), ("index", _slot(8))])
    add("index-slot-written-by-a-run", 3, [("run", 5), _pal(1), _pal(2, 9), ("index", 11 * 255 & 63), ("diff", 1, 1, -2), _pal(3), ("run", 7), _pal(4), ("index", _slot(3))])
    add("index-64-ops-in-one-group", 4, every + [("index", _slot(37 * k + 5)) for k in range(GROUP)] + _ordinary(13))
    add("index-64-ops-on-one-slot", 3, every + [("index", _slot(7))] * GROUP + _ordinary(14))
    first = [_pal(k, k // 3) for k in range(WIN // 4)]                # WIN / 4 four-byte ops: the next op is the first of the second window
    add("index-first-op-of-a-window", 4, first + [("index", _slot(2)), ("index", _slot(3)), ("diff", 0, 1, -1), ("index", _slot(2))])
    return out


def _alpha_cases():
    """RGBA ops in a file whose header says three channels: the alpha they set is carried by every later DIFF, LUMA and RUN pixel, and an
    INDEX op brings back the alpha of the pixel it names -- all of it visible at output 4 only"""
    a, b = (10, 20, 30, 77), (100, 100, 100, 255)
    ops = ([("rgb",) + b[:3]] + _filler(5) + [("rgba",) + a] + _filler(4, 3) + [("luma", 6, -2, 1), ("run", 3), ("index", hash_of(b)), ("diff", 1, -1, 0),
            ("index", hash_of(a)), ("luma", -9, 4, 4)] + _filler(70, 8) + [("rgb", 40, 50, 60), ("diff", -1, -1, -1), ("rgba", 1, 2, 3, 0), ("run", 9), ("luma", 1, 1, 1),
            ("index", hash_of(a))] + _filler(6, 1))
    w, h = _dims(op_pixels(ops), 6)
    return [Case("alpha-rgba-ops-in-a-three-channel-file", qoi_file(w, h, 3, ops))]


def _arbitrary_streams():
    """streams no encoder writes: random chunk bytes under a valid header (every byte sequence is a QOI op sequence) -- too short, too
    long, op mixes that change every window's entry offset, runs across the end of the image"""
    rng = np.random.default_rng(31)
    out = []
    for k in range(24):
        w, h, ch = int(rng.integers(1, 400)), int(rng.integers(1, 60)), 3 + (k & 1)
        need = w * h
        nbytes = int(rng.integers(0, 3 * need + 40))
        body = rng.integers(0, 256, nbytes, dtype=np.uint8)
        if k % 3 == 0:
            body[rng.random(nbytes) < 0.5] = 0xC0 | int(rng.integers(0, 62))          # many RUN ops
        if k % 4 == 1:
            body[rng.random(nbytes) < 0.6] &= 0x3F                                    # many INDEX ops
        out.append(b"qoif" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([ch, 0]) + body.tobytes() + bytes(7) + b"\x01")
    # RGB, RGBA and INDEX ops close together among DIFF / LUMA ops: every combination of "the most recent op that set the colour" and "the most
    # recent op that set alpha" inside one group of 64 ops (qoi_group_scan's three alpha cases), in densities from a few per group to most ops
    for k in range(16):
        w, h, ch = int(rng.integers(40, 500)), int(rng.integers(8, 50)), 3 + (k & 1)
        nbytes = int(rng.integers(w * h, 3 * w * h))
        body = rng.integers(0x40, 0xC0, nbytes, dtype=np.uint8)                         # DIFF and LUMA ops (a LUMA op's second byte: any of these)
        p_rgb, p_rgba, p_idx = [(0.02, 0.0, 0.01), (0.0, 0.02, 0.02), (0.05, 0.05, 0.05), (0.3, 0.2, 0.2)][k // 4]
        r = rng.random(nbytes)
        body[r < p_rgb] = 0xFE
        body[(r >= p_rgb) & (r < p_rgb + p_rgba)] = 0xFF
        body[(r >= p_rgb + p_rgba) & (r < p_rgb + p_rgba + p_idx)] &= 0x3F
        if k % 4 == 3:
            body[rng.random(nbytes) < 0.03] = 0xC0 | int(rng.integers(0, 62))
        out.append(b"qoif" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([ch, 0]) + body.tobytes() + bytes(7) + b"\x01")
    return out


CONSTRUCTED = _straddle_cases() + _chunk_length_cases() + _pixel_buffer_cases() + _image_full_cases() + _index_cases() + _alpha_cases()
ARBITRARY = [Case(f"arbitrary-{k:02d}", f) for k, f in enumerate(_arbitrary_streams())]
CASES = CONSTRUCTED + ARBITRARY
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def header(data):
    """(width, height, file channels)"""
    return int.from_bytes(data[4:8], "big"), int.from_bytes(data[8:12], "big"), data[12]


@functools.lru_cache(maxsize=None)
def expected(name, channels):
    """the oracle's pixels of a case (qoi_decode, qoi.d:448-550), flat; computed once, shared, read-only"""
    px = O.qoi_decode(BY_NAME[name].data, channels)[0].reshape(-1)
    px.setflags(write=False)
    return px

