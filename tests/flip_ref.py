"""CPU reference for the in-place flips (image.d flipHorizontal :1475-1509, flipVerticalPhysical :1926-1954).

TEST INFRASTRUCTURE.  Both functions work on a raw uint8 buffer addressed the way an Image addresses its storage: the byte
where scanline 0 of layer 0 starts, a signed pitch from one scanline to the next, a layer offset from one layer to the next.
For every layer and row the horizontal flip swaps pixel x with pixel W - 1 - x (x < W / 2); the vertical flip swaps the first
w * ps bytes of row y with those of row H - 1 - y (y < H / 2).  No byte outside [row, row + w * ps) is ever written.

`flip` is the vectorised form the GPU tests use; `flip_loops` is the literal pixel-by-pixel / byte-by-byte restatement, kept
for tests/test_flip_ref_cpu.py to check the vectorised form against.
"""
import numpy as np


def layout(w, h, layers, ps, pad=0, negative=False, gap=0, guard=64, lead=0):
    """Geometry of a test buffer: `guard` bytes, `lead` more (to move the base address), then `layers` layers of h rows of
    w * ps + pad bytes with `gap` bytes between layers, then `guard` bytes.  With `negative` the rows of a layer are stored
    bottom-up: scanline 0 is the highest-address row and the pitch is negative.
    -> (buffer size, offset of scanline 0 of layer 0, signed pitch, layer offset)"""
    step = w * ps + pad
    span = step * h
    layer_off = span + gap
    low = guard + lead
    size = low + layer_off * (layers - 1) + span + guard
    if negative:
        return size, low + (h - 1) * step, -step, layer_off
    return size, low, step, layer_off


def _check(buf, first, pitch, layer_off, w, h, layers, ps):
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags.c_contiguous and buf.flags.writeable
    assert w >= 0 and h >= 0 and layers >= 0 and ps >= 1
    if w == 0 or h == 0 or layers == 0:
        return False
    scan = w * ps
    assert h == 1 or abs(pitch) >= scan, "overlapping scanlines"
    for layer in (0, layers - 1):
        for y in (0, h - 1):
            at = first + layer * layer_off + y * pitch
            assert 0 <= at and at + scan <= buf.size, "a row lies outside the buffer"
    return True


def _layer_view(buf, at, pitch, w, h, ps):
    """(h, w, ps) writable view of one layer's pixel bytes; row y starts at byte at + y * pitch (pitch may be negative or 0)"""
    return np.lib.stride_tricks.as_strided(buf[at:], shape=(h, w, ps), strides=(pitch if h > 1 else 0, ps, 1), writeable=True)


def flip(buf, first, pitch, layer_off, w, h, layers, ps, vertical):
    """in place; returns buf"""
    if not _check(buf, first, pitch, layer_off, w, h, layers, ps):
        return buf
    for layer in range(layers):
        v = _layer_view(buf, first + layer * layer_off, pitch, w, h, ps)
        if vertical:
            half = h // 2
            if half:                                            # (h - 1 - half >= half - 1 >= 0: the slice end is never -1)
                top = v[:half].copy()
                v[:half] = v[h - 1:h - 1 - half:-1]
                v[h - 1:h - 1 - half:-1] = top
        else:
            half = w // 2
            if half:
                left = v[:, :half].copy()
                v[:, :half] = v[:, w - 1:w - 1 - half:-1]
                v[:, w - 1:w - 1 - half:-1] = left
    return buf


def flip_loops(buf, first, pitch, layer_off, w, h, layers, ps, vertical):
    """the reference's loops as they stand: one pixel (horizontal) or one byte (vertical) at a time.  In place; returns buf"""
    if not _check(buf, first, pitch, layer_off, w, h, layers, ps):
        return buf
    scan = w * ps
    for layer in range(layers):
        base = first + layer * layer_off
        if vertical:
            for y in range(h // 2):
                a, b = base + y * pitch, base + (h - 1 - y) * pitch
                for i in range(scan):
                    t = buf[a + i]
                    buf[a + i] = buf[b + i]
                    buf[b + i] = t
        else:
            for y in range(h):
                row = base + y * pitch
                for x in range(w // 2):
                    a, b = row + x * ps, row + (w - 1 - x) * ps
                    t = buf[a:a + ps].copy()
                    buf[a:a + ps] = buf[b:b + ps]
                    buf[b:b + ps] = t
    return buf
