"""Writers of QOI-Plane test files (QOIX with 8 bits and 1 or 2 channels), from the format description: op builders that return nibble
lists, the packing of nibbles into bytes, and an encoder that follows the rules of qoiplane_encode (source/gamut/codecs/qoiplane.d:109-365:
a run is cut at 258 pixels and at the last pixel; an alpha step of -7..7 is an ADIFF followed by a colour op, any other an LA; the colour
op is the first of DIFF1, DIFF2, DIRECT that fits; nine f nibbles close the stream, and one more to reach a byte boundary).  The
container and the LZ4 block come from tests/qoix_gen.py."""
import numpy as np

import qoix_gen as G

F = 15
CLOSING = [F] * 8                                                           # the four closing bytes as nibbles


def DIFF1(d):
    assert -4 <= d <= 3
    return [d + 4]


def DIFF2(d):
    assert -16 <= d <= 15
    return [8 | (d + 16) >> 4, (d + 16) & 15]


def DIRECT(v):
    return [10, v >> 4, v & 15]


def ADIFF(d):
    assert -7 <= d <= 7 and d != 0
    return [11, d + 8]


def LA(l, a):
    return [11, 0, l >> 4, l & 15, a >> 4, a & 15]


def REPEAT1(pixels):
    assert 1 <= pixels <= 3
    return [12 | (pixels - 1)]


def REPEAT2(pixels):
    assert 4 <= pixels <= 258
    return [F, (pixels - 4) >> 4, (pixels - 4) & 15]


TO_END = [F, F, F]


def pack(nibbles):
    """nibbles, high one first, -> bytes; an odd count is completed with f"""
    nibbles = list(nibbles) + [F] * (len(nibbles) & 1)
    return bytes(h << 4 | l for h, l in zip(nibbles[::2], nibbles[1::2]))


def stored(w, h, nibbles, channels=1, closing=CLOSING, **kw):
    """an uncompressed file: header, the op nibbles and the closing nibbles right behind them"""
    return G.header(w, h, channels, **kw) + pack(list(nibbles) + list(closing))


def compressed(w, h, nibbles, channels=1, closing=CLOSING, **kw):
    return G.compressed(w, h, pack(list(nibbles) + list(closing)), channels, pad=b"", **kw)


def _s8(v):
    v &= 255
    return v - 256 if v >= 128 else v


def encode_nibbles(img):
    """(h, w, 1 or 2) uint8 -> the op nibbles and the closing ones, as qoiplane_encode writes them"""
    h, w, ch = img.shape
    la = np.full((h, w, 2), 255, np.uint8)
    la[..., :ch] = img
    flat = [(int(p[0]), int(p[1])) for p in la.reshape(-1, 2)]
    out, px, run, n = [], (0, 255), 0, w * h

    def end_run():
        nonlocal run
        out.extend(REPEAT1(run) if run <= 3 else REPEAT2(run))
        run = 0
    for i, t in enumerate(flat):
        ref, px = px, t
        if px == ref:
            run += 1
            if run == 258 or i + 1 == n:
                end_run()
            continue
        if run:
            end_run()
        va = _s8(px[1] - ref[1])
        if va and not -7 <= va <= 7:
            out.extend(LA(*px))
            continue
        if va:
            out.extend(ADIFF(va))
        top = flat[i - w][0] if i >= w else ref[0]
        d = _s8(px[0] - (top + ref[0] + 1) // 2)
        out.extend(DIFF1(d) if -4 <= d <= 3 else DIFF2(d) if -16 <= d <= 15 else DIRECT(px[0]))
    out.extend([F] * 9)
    return out + [F] * (len(out) & 1)


def encode(img, lz4=False, **kw):
    h, w, ch = img.shape
    body = pack(encode_nibbles(img))
    return G.compressed(w, h, body, ch, pad=b"", **kw) if lz4 else G.header(w, h, ch, **kw) + body


# ---- pictures
def noisy(w, h, ch=1, seed=0):
    """photo-like with flat stretches and a few outliers: every op kind"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, ch), np.uint8)
    img[..., 0] = np.clip(128 + 100 * np.sin(xx / 23.0 + seed) * np.cos(yy / 17.0) + rng.normal(0, 3, (h, w)), 0, 255)
    if ch == 2:
        img[..., 1] = np.clip(200 + 60 * np.sin(xx / 9.0 + yy / 5.0) + (rng.random((h, w)) < 0.05) * rng.integers(-90, 90, (h, w)), 0, 255)
    for _ in range(3):
        x0 = int(rng.integers(0, w))
        img[int(rng.integers(0, h)), x0:x0 + int(rng.integers(1, w + 1))] = rng.integers(0, 256, ch)
    img[rng.integers(0, h, 4), rng.integers(0, w, 4)] = rng.integers(0, 256, (4, ch))
    return img


def photo_like(w, h, ch=1, seed=0):
    """smooth gradients plus noise: mostly DIFF1 / DIFF2 ops"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, ch), np.uint8)
    img[..., 0] = np.clip(128 + 100 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + rng.normal(0, 3, (h, w)), 0, 255)
    if ch == 2:
        img[..., 1] = np.clip(200 + 50 * np.sin(xx / 40.0), 0, 255)
    return img


def flat_image(w, h, ch=1, seed=0):
    """a few flat rectangles: runs"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, ch), np.uint8)
    img[...] = rng.integers(0, 256, ch)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(1, h // 2 + 2)), x0:x0 + int(rng.integers(1, w // 2 + 2))] = rng.integers(0, 256, ch)
    return img


def few_levels(w, h, ch=1, seed=0, levels=4):
    rng = np.random.default_rng(seed)
    img = (rng.integers(0, levels, (h, w, ch)) * (255 // (levels - 1))).astype(np.uint8)
    return img


def alpha_ramp(w, h, seed=0, step=3):
    """luminance noise under an alpha that climbs by `step` a pixel and wraps: ADIFF ops, an LA at every wrap"""
    img = noisy(w, h, 2, seed)
    img[..., 1] = (np.arange(w * h).reshape(h, w) * step) & 255
    return img
