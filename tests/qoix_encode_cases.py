"""Source images and byte strings for the QOIX encoder tests (tests/test_qoix_encode_cpu.py, tests/test_qoix_encode_gpu.py): the smallest
shapes at which each mechanism of qoix_encode / LZ4_compress / the container choice can go wrong.  Everything is seeded."""
import numpy as np

import qoix_gen

HEIGHTS = (1, 2, 5)
CONTENTS = ("photo", "flat", "noise", "alphabet", "vgrad", "hgrad")

# (image, op stream with the pad, hex) -- derived by hand from qoi2avg.d:376-615; every one is a stored file
KNOWN_STREAMS = [
    ("1x1 rgb black", np.zeros((1, 1, 3), np.uint8), "f800ffffffff"),
    ("1x1 rgba zero", np.zeros((1, 1, 4), np.uint8), "80ffffffff"),
    ("2x1 rgb grey 10", np.full((1, 2, 3), 10, np.uint8), "fc0af800ffffffff"),
    ("1x1 rgb (1,2,1)", np.array([[[1, 2, 1]]], np.uint8), "65ffffffff"),
    ("1x1 rgba alpha 254", np.array([[[0, 0, 0, 254]]], np.uint8), "eb4affffffff"),
    ("1030x1 rgb black", np.zeros((1, 1030, 3), np.uint8), "fbfff805ffffffff"),
]


def content(kind, w, h, ch, seed):
    rng = np.random.default_rng(seed)
    if kind == "photo":
        return qoix_gen.photo_like(w, h, ch, seed)
    if kind == "flat":
        return qoix_gen.flat_image(w, h, ch, seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, ch)).astype(np.uint8)
    if kind == "alphabet":                                                  # five colours: index hits, short runs
        return rng.integers(0, 256, (5, ch)).astype(np.uint8)[rng.integers(0, 5, (h, w))]
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (yy if kind == "vgrad" else xx).astype(np.int64)
    return np.stack([(ramp * (k + 1) + 7 * k) & 255 for k in range(ch)], -1).astype(np.uint8)


def matrix_images(widths):
    """[(name, image)]: every width x HEIGHTS x rgb8 / rgba8 x CONTENTS"""
    out, seed = [], 0
    for w in widths:
        for h in HEIGHTS:
            for ch in (3, 4):
                for kind in CONTENTS:
                    seed += 1
                    out.append((f"{kind} {w}x{h}x{ch}", content(kind, w, h, ch, seed)))
    return out


def _distinct_noise(n, ch, seed):
    """n pixels, no two neighbours equal"""
    px = np.random.default_rng(seed).integers(0, 256, (n, ch)).astype(np.uint8)
    same = np.flatnonzero((px[1:] == px[:-1]).all(1)) + 1
    px[same, 0] ^= 1
    return px


RUN_LENGTHS = (1, 8, 9, 1023, 1024, 1025, 2049)


def run_images():
    """a pixel repeated `run` more times, mid-row, across a row end, ending at the last pixel"""
    out = []
    for k, run in enumerate(RUN_LENGTHS):
        for ch in (3, 4):
            wide = _distinct_noise(2 * (run + 120), ch, 100 + k).reshape(2, run + 120, ch)
            wide[1, 50:51 + run] = wide[1, 50]
            out.append((f"run {run} mid-row x{ch}", wide))
            w = 300
            h = (250 + run + 10) // w + 2
            flat = _distinct_noise(w * h, ch, 200 + k)
            flat[w + 250:w + 251 + run] = flat[w + 250]
            out.append((f"run {run} across a row end x{ch}", flat.reshape(h, w, ch)))
            flat = _distinct_noise(w * h, ch, 300 + k)
            flat[w * h - 1 - run:] = flat[w * h - 1 - run]
            out.append((f"run {run} to the last pixel x{ch}", flat.reshape(h, w, ch)))
    return out


_VG = (-65, -64, -17, -16, -5, -4, -1, 0, 3, 4, 15, 16, 63, 64)
_VRB = (-33, -32, -9, -8, -3, -2, -1, 0, 1, 2, 3, 7, 8, 31, 32)


def _delta_walk(alpha_step):
    """pixels whose deltas to their predecessor sit on every LUMA / LUMA2 / LUMA3 bound and one past it (row 0: the reference colour is
    the previous pixel); grey pixels that also fit LUMA2 (GRAY is tested first) and LUMA (which wins) follow"""
    px, cur, a = [], np.array([90, 100, 110], np.int64), 128
    for vg in _VG:
        for vr in _VRB:
            for vb in (vr, 0):
                cur = (cur + np.array([vg + vr, vg, vg + vb])) & 255
                a = (a + alpha_step) & 255
                px.append([*cur, a])
    g = 40
    for step in (10, -10, 2, -3, 12, 15, -16, 40, 100):
        g = (g + step) & 255
        a = (a + alpha_step) & 255
        px.append([g, g, g, a])
    return np.array(px, np.uint8)


def op_images():
    """alpha steps, LUMA bounds, the FIFO and the hash table"""
    out = []
    walk = _delta_walk(0)
    out.append(("luma bounds row 0", walk[:, :3].reshape(1, -1, 3).copy()))
    n = walk.shape[0] // 7 * 7
    out.append(("luma bounds with the predictor", walk[:n, :3].reshape(7, -1, 3).copy()))
    out.append(("ADIFF in front of every colour op", _delta_walk(1).reshape(1, -1, 4)))
    out.append(("ADIFF -2 with the predictor", _delta_walk(-2)[:n].reshape(7, -1, 4).copy()))
    rng = np.random.default_rng(7)
    steps = (-5, -4, -1, 3, 4)
    a, px = 128, []
    for k in range(40):
        a = (a + steps[k % 5]) & 255
        rgb = rng.integers(0, 256, 3) if k % 3 else (px[-1][:3] if px else [1, 2, 3])      # every third: the colour stays, alpha alone moves
        px.append([*rgb, a])
    out.append(("alpha steps", np.array(px, np.uint8).reshape(2, 20, 4)))
    for gap in (63, 64, 65):
        for ch in (3, 4):
            d = _distinct_noise(gap + 3, ch, 400 + gap)
            d[gap + 1] = d[0]                                               # `gap` misses lie between the two
            out.append((f"recurs after {gap} misses x{ch}", d.reshape(1, -1, ch)))
    c1, c2 = equal_hash_pair()
    alt = np.array([c1, c2] * 20, np.uint8)
    out.append(("two colours of equal hash", alt.reshape(2, 20, 4)))
    z = _distinct_noise(70, 4, 500)
    z[0] = 0; z[65] = 0                                                     # (0,0,0,0) first: INDEX 0; again behind 64 misses
    out.append(("zero pixel first and after 64 misses", z.reshape(1, -1, 4)))
    return out


def color_hash(c):
    v = int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16 | int(c[3]) << 24
    return ((v * 2654435769) & 0xFFFFFFFF) >> 22 & 1023


def equal_hash_pair():
    rng, seen = np.random.default_rng(11), {}
    while True:
        c = tuple(int(x) for x in rng.integers(0, 256, 4))
        h = color_hash(c)
        if h in seen and seen[h] != c:
            return seen[h], c
        seen[h] = c


def parse_ops(stream):
    """the op kinds of a stream (pad removed by the caller) in order"""
    kinds, p = [], 0
    while p < len(stream):
        b = stream[p]
        kind, n = (("LUMA", 1) if b < 0x80 else ("INDEX", 1) if b < 0xc0 else ("LUMA2", 2) if b < 0xe0 else ("LUMA3", 3) if b < 0xe8 else
                   ("ADIFF", 1) if b < 0xf0 else ("RUN", 1) if b < 0xf8 else ("RUN2", 2) if b < 0xfc else ("GRAY", 2) if b == 0xfc else
                   ("RGB", 4) if b == 0xfd else ("RGBA", 5) if b == 0xfe else ("END", 1))
        kinds.append(kind)
        p += n
    assert p == len(stream)
    return kinds


# ---- LZ4 strings
def _noise(n, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n).astype(np.uint8).tobytes()


def lz4_strings():
    out = [(f"length {n}", _noise(n, n, 3)) for n in (0, 1, 12, 13, 14)]
    for n in (65546, 65547):                                                # byU16's last length, byU32's first
        out.append((f"length {n}", (_noise(3000, n, 8) + _noise(500, n + 1)) * 18 + _noise(n - 18 * 3500, n + 2, 5)))
    out.append(("noise 70000", _noise(70000, 1)))
    out.append(("pattern 140000", (_noise(64, 2) * 2200)[:140000]))
    for dist in (65535, 65536, 70000):
        s = bytearray(_noise(140000, 3))
        s[1000 + dist:6000 + dist] = s[1000:6000]
        out.append((f"recurs {dist} later", bytes(s)))
    x = _noise(100, 4)
    out.append(("literal runs between matches", x + _noise(14, 5) + x + _noise(15, 6) + x + _noise(269, 7) + x + _noise(270, 8) + x + _noise(20, 9)))
    s = _noise(200, 10)
    out.append(("match to end - 5", s + s[:100]))
    s = _noise(300, 11)
    out.append(("last 12 bytes match", s + s[10:22]))
    out.append(("zeros 1000", bytes(1000)))
    return out


def lz4_mixed(count=100, seed=12):
    rng = np.random.default_rng(seed)
    return [_noise(int(rng.integers(0, 3000)), 1000 + k, int(rng.choice([2, 4, 16, 256]))) for k in range(count)]


# ---- the container choice: images whose lz4Size + 4 - datalen sits at the boundary (found by a sweep with the restatement over
# qoix_gen.photo_like / flat_image at small sizes; tests/test_qoix_encode_cpu.py asserts the differences)
BOUNDARY = [
    # (kind, w, h, ch, seed, lz4Size + 4 - datalen)
    ("flat", 9, 21, 4, 293, -2), ("flat", 11, 15, 3, 384, -2),
    ("flat", 38, 10, 4, 71, -1), ("flat", 35, 7, 3, 132, -1), ("flat", 9, 11, 4, 207, -1), ("flat", 28, 14, 3, 238, -1),
    ("photo", 39, 14, 4, 245, 0), ("flat", 19, 9, 4, 303, 0), ("flat", 20, 7, 3, 332, 0), ("flat", 29, 11, 4, 347, 0),
    ("flat", 26, 14, 4, 19, 1), ("flat", 19, 12, 3, 24, 1), ("flat", 39, 7, 3, 136, 1), ("flat", 29, 9, 3, 152, 1),
    ("flat", 23, 8, 4, 25, 2), ("flat", 16, 9, 3, 54, 2),
]


def boundary_images():
    return [(f"{kind} {w}x{h}x{ch} seed {seed}: {diff:+d}", content(kind, w, h, ch, seed), diff) for kind, w, h, ch, seed, diff in BOUNDARY]
