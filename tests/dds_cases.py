"""Inputs of the DDS / BC7 tests, generated: tiles of 16 rgba pixels for the blocks entry and images for the file entry.  The CPU
tests check with the restatement alone that these tiles reach every path of the encoder (tests/test_dds_cpu.py, the coverage floor);
the GPU tests use exactly these inputs."""
import functools

import numpy as np

import bc7_decode


def _opaque(rgb):
    rgb = np.asarray(rgb, np.int64).reshape(-1, 16, 3)
    return np.concatenate([np.clip(rgb, 0, 255), np.full(rgb.shape[:2] + (1,), 255)], axis=2).astype(np.uint8)


def solid_greys():
    v = np.arange(256).reshape(256, 1, 1)
    return _opaque(np.broadcast_to(v, (256, 16, 3)))


def two_colour():
    """every 2-subset partition pattern in two flat colours: all components even, all odd (mode 6 holds both colours exactly), and
    of mixed parity (no p-bit fits a colour, so mode 1 is tried and both subsets are single colours)"""
    out = []
    for parity in ((0, 0, 0), (1, 1, 1), (1, 0, 1)):
        for p, pattern in enumerate(bc7_decode.PARTITIONS):
            a = np.array([(40 + 2 * p) % 256, (200 - 2 * p) % 256, (16 + 6 * p) % 256]) // 2 * 2 + parity
            b = np.array([(220 - 2 * p) % 256, (30 + 2 * p) % 256, (140 + 4 * p) % 256]) // 2 * 2 + parity[::-1]
            out.append([b if bit else a for bit in pattern])
    return _opaque(out)


def grey_ramps():
    out = []
    for base, step in ((0, 1), (0, 17), (100, 1), (100, 2), (250, -3), (7, 5), (128, 0.25), (30, 0.5), (254, -0.125), (3, 9)):
        v = np.clip(np.floor(base + step * np.arange(16)), 0, 255)
        out.append(np.stack([v, v, v], axis=1))
        out.append(np.stack([v, v, v], axis=1).reshape(4, 4, 3).transpose(1, 0, 2).reshape(16, 3))
    return _opaque(out)


def noise(n=240, seed=7):
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 256, (n // 2, 16, 3))
    base = rng.integers(0, 256, (n - n // 2, 1, 3))
    amp = rng.integers(1, 24, (n - n // 2, 1, 1))
    return _opaque(np.concatenate([full, base + rng.integers(-1, 2, (n - n // 2, 16, 3)) * amp]))


def photo(w, h, comp, seed):
    """a smooth picture with edges and a little grain; alpha (comp 2 and 4) is 255 but for a soft-edged disc"""
    rng = np.random.default_rng([seed, w, h, comp])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for k in range(3):
        f = rng.uniform(0.02, 0.3, 4)
        v = 128 + 70 * np.sin(f[0] * x + f[1] * y + k) + 40 * np.cos(f[2] * x - f[3] * y)
        v += 60 * ((x * (k + 1) + 2 * y) % 23 < 9)
        ch.append(v + rng.normal(0, 2.5, (h, w)))
    rgb = np.clip(np.stack(ch, axis=2), 0, 255).astype(np.uint8)
    a = np.clip(255 - 40 * np.maximum(0, 0.35 * min(w, h) + 1 - np.hypot(x - w / 2, y - h / 3)), 0, 255).astype(np.uint8)
    if comp == 1:
        return rgb[:, :, 1:2].copy()
    if comp == 2:
        return np.stack([rgb[:, :, 1], a], axis=2)
    return rgb if comp == 3 else np.concatenate([rgb, a[:, :, None]], axis=2)


def tiles_of(img):
    """the 4 x 4 tiles of an (h, w, 4) image whose sides are multiples of 4, in row-major order"""
    h, w, _ = img.shape
    return img.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4).copy()


def photo_tiles():
    img = photo(64, 64, 3, 3)
    return tiles_of(np.concatenate([img, np.full((64, 64, 1), 255, np.uint8)], axis=2))


def alpha_tiles():
    base = noise(12, 21)
    out = []
    for k, t in enumerate(base):
        for where, value in ((0, 254), (15, 254), (0, 0), (15, 0), (0, 200 - 10 * k), (15, 3 + k)):
            u = t.copy(); u[where, 3] = value; out.append(u)
        u = t.copy(); u[:, 3] = 0; out.append(u)
        u = t.copy(); u[:, 3] = 254; out.append(u)
        u = t.copy(); u[:, 3] = np.arange(16) * 17; out.append(u)
    out.append(np.zeros((16, 4), np.uint8))
    out.append(np.full((16, 4), 255, np.uint8))
    flat = np.zeros((16, 4), np.uint8); flat[:] = (90, 14, 201, 254); out.append(flat)
    return np.asarray(out, np.uint8)


@functools.lru_cache(maxsize=None)
def groups():
    return (("solid", solid_greys()), ("two_colour", two_colour()), ("ramps", grey_ramps()), ("noise", noise()), ("photo", photo_tiles()),
            ("alpha", alpha_tiles()))


@functools.lru_cache(maxsize=None)
def all_tiles():
    """every tile above in one (n, 16, 4) array; n > 1000"""
    t = np.concatenate([g for _, g in groups()])
    t.setflags(write=False)
    return t


def image(w, h, comp, seed=0):
    """(h, w, comp) uint8"""
    im = photo(w, h, comp, seed)
    return im.reshape(h, w, comp)
