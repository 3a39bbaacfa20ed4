"""A second reading of the reference's QOIX loader for 8-bit grey files (1 or 2 channels), in Python, written from the D text on its own
(source/gamut/plugins/qoix.d:350-507, codecs/qoiplane.d:377-541) and not from tests/c/qoiplane_ref.c.  It works on whole-image arrays
where the C reading walks scanlines: the stream becomes one nibble array, the ops are listed first (their lengths and pixel counts do not
depend on pixel values), alpha is a segmented cumulative sum over the ops, luminance one flat array of width * height values in which
`top` is the value `width` places back, and runs are slices.  The container and the LZ4 block are those of tests/qoix_ref.py.
Deviation P1 (gamut_amd/csrc/qoix.hip) is part of it: a nibble read at byte index >= size refuses the file.

This is the library with gamut_hip_qoix_set_plane(1): parse(data) -> (verdict, info, size the sub-codec sees);
decode(data, channels) -> None or (pixels (h, w, channels) uint8, info).  Colour files are handed to tests/qoix_ref.py."""
import numpy as np

import qoix_ref
from qoix_ref import OK, REFUSED, UNSUPPORTED, Refused

DIFF, DIRECT, LA, ADIFF, REPEAT = range(5)


def parse(data):
    data = bytes(data)
    verdict, info, size = qoix_ref.parse(data)
    if verdict != UNSUPPORTED or info["bitdepth"] != 8:
        return verdict, info, size
    size = 25 + info["orig"] if info["compression"] == 1 else len(data)
    w, h = info["width"] & 0xFFFFFFFF, info["height"] & 0xFFFFFFFF
    bad = size < 29 or w == 0 or h == 0 or info["colorspace"] > 1 or info["version"] > 1 or not info["detected"] or h >= 400000000 // max(w, 1)
    return (REFUSED if bad else OK), info, size


def list_ops(nib, n):
    """the ops that produce the first n pixels -> [(kind, pixels, a, b)]; pixels is None for "to the end" """
    ops, i, pixels = [], 0, 0

    def take(k):
        nonlocal i
        if i + k > len(nib):
            raise Refused("nibble behind the stream")                        # deviation P1
        v = 0
        for t in nib[i:i + k]:
            v = v << 4 | int(t)
        i += k
        return v
    while pixels < n:
        op = take(1)
        if op < 8:
            ops.append((DIFF, 1, op - 4, 0))
        elif op < 10:
            ops.append((DIFF, 1, ((op & 1) << 4 | take(1)) - 16, 0))
        elif op == 10:
            ops.append((DIRECT, 1, take(2), 0))
        elif op == 11:
            d = take(1)
            if d:
                ops.append((ADIFF, 0, d - 8, 0))
            else:
                v = take(4)
                ops.append((LA, 1, v >> 8, v & 255))
        elif op < 15:
            ops.append((REPEAT, 1 + (op & 3), 0, 0))
        else:
            b = take(2)
            ops.append((REPEAT, n - pixels if b == 255 else b + 4, 0, 0))
        pixels += ops[-1][1]
    return ops


def plane(b, size, w, h):
    """qoiplane_decode's pixel loop over bytes b[25:size] -> (h * w, 2) uint8 of (luminance, alpha), or Refused"""
    n = w * h
    body = np.frombuffer(bytes(b[25:size]), np.uint8)
    nib = np.stack([body >> 4, body & 15], 1).reshape(-1)
    ops = list_ops(nib, n)
    # alpha per pixel op: LA sets it; the last ADIFF in front of an op adds to the alpha of the previous pixel
    kinds = np.array([o[0] for o in ops])
    is_pix = kinds != ADIFF
    after_adiff = np.concatenate([[False], kinds[:-1] == ADIFF])
    delta_in_front = np.concatenate([[0], np.array([o[2] for o in ops])[:-1]])
    step = np.where(after_adiff, delta_in_front, 0)[is_pix]
    pk = kinds[is_pix]
    absolute = pk == LA
    value = np.array([o[3] for o in ops])[is_pix]
    seg = np.cumsum(absolute)                                               # the number of the LA that governs the op
    base = np.concatenate([[255], value[absolute]])[seg]
    total = np.cumsum(np.where(absolute, 0, step))
    at_la = np.concatenate([[0], total[absolute]])[seg]                     # what had been added when that LA came
    alpha = (base + total - at_la) & 255
    counts = np.array([o[1] for o in ops])[is_pix]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    # luminance: one flat array, the only serial part
    lum = np.zeros(n + 258, np.int64)
    l = 0
    for (kind, cnt, a, _), i in zip([o for o in ops if o[0] != ADIFF], first.tolist()):
        if i >= n:
            break
        if kind == DIFF:
            top = lum[i - w] if i >= w else l
            l = ((top + l + 1) // 2 + a) & 255
        elif kind != REPEAT:
            l = a
        lum[i:i + cnt] = l
    out = np.zeros((n, 2), np.uint8)
    out[:, 0] = lum[:n]
    out[:, 1] = np.repeat(alpha, counts)[:n]
    return out


def decode(data, channels=0):
    """-> None when the load fails, else (pixels (h, w, channels or the file's) uint8, info)"""
    data = bytes(data)
    verdict, info, size = parse(data)
    if verdict != OK:
        return None
    if info["channels"] >= 3:
        return qoix_ref.decode(data, channels)
    try:
        if info["compression"] == 1:
            data = data[:16] + b"\0" + data[17:25] + qoix_ref.lz4_block(data[29:], info["orig"])
        img = plane(data, size, info["width"], info["height"])
    except Refused:
        return None
    ch = channels or info["channels"]
    return np.ascontiguousarray(img.reshape(info["height"], info["width"], 2)[..., :ch]), info
