"""The flip reference (tests/flip_ref.py) checks itself, without a GPU: the vectorised form the GPU tests compare against equals
the literal pixel-by-pixel restatement of image.d's loops, and both have the properties a flip must have."""
import itertools

import numpy as np
import pytest

import flip_ref as F

PIXEL_SIZES = [1, 2, 3, 4, 6, 8, 12, 16]
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (2, 3), (4, 4), (5, 3), (6, 5), (7, 7), (8, 6)]          # (w, h): odd, even, and 1


def _cases():
    for ps, (w, h), negative, layers in itertools.product(PIXEL_SIZES, SHAPES, (False, True), (1, 2, 3)):
        pad = (0, 3, 5)[(ps + w + h + layers) % 3]
        yield ps, w, h, negative, layers, pad, (0 if layers == 1 else 7 + ps)


def _buffer(rng, *geometry, **kw):
    size, first, pitch, layer_off = F.layout(*geometry, **kw)
    return rng.integers(0, 256, size, dtype=np.uint8), first, pitch, layer_off


def _pixel_mask(size, first, pitch, layer_off, w, h, layers, ps):
    m = np.zeros(size, bool)
    for layer in range(layers):
        for y in range(h):
            at = first + layer * layer_off + y * pitch
            m[at:at + w * ps] = True
    return m


def _pixels(buf, first, pitch, layer_off, w, h, layers, ps):
    """(layers, h, w, ps) copy in logical order"""
    return np.stack([np.stack([buf[first + l * layer_off + y * pitch:][:w * ps].reshape(w, ps) for y in range(h)]) for l in range(layers)])


@pytest.mark.parametrize("vertical", [0, 1], ids=["horizontal", "vertical"])
def test_vectorised_equals_loops(vertical):
    rng = np.random.default_rng(31 + vertical)
    n = 0
    for ps, w, h, negative, layers, pad, gap in _cases():
        buf, first, pitch, layer_off = _buffer(rng, w, h, layers, ps, pad=pad, negative=negative, gap=gap, guard=16, lead=(ps + w) % 4)
        a = F.flip(buf.copy(), first, pitch, layer_off, w, h, layers, ps, vertical)
        b = F.flip_loops(buf.copy(), first, pitch, layer_off, w, h, layers, ps, vertical)
        assert np.array_equal(a, b), (ps, w, h, negative, layers, pad, gap)
        n += 1
    assert n == len(PIXEL_SIZES) * len(SHAPES) * 2 * 3


def test_twice_is_identity_and_pads_are_untouched():
    rng = np.random.default_rng(32)
    for ps, w, h, negative, layers, pad, gap in _cases():
        buf, first, pitch, layer_off = _buffer(rng, w, h, layers, ps, pad=pad, negative=negative, gap=gap)
        outside = ~_pixel_mask(buf.size, first, pitch, layer_off, w, h, layers, ps)
        for fn in (F.flip, F.flip_loops):
            for vertical in (0, 1):
                once = fn(buf.copy(), first, pitch, layer_off, w, h, layers, ps, vertical)
                assert np.array_equal(once[outside], buf[outside]), "canary bytes in pads, gaps and guards"
                twice = fn(once.copy(), first, pitch, layer_off, w, h, layers, ps, vertical)
                assert np.array_equal(twice, buf), (ps, w, h, negative, layers, vertical)


def test_both_flips_reverse_both_axes():
    rng = np.random.default_rng(33)
    for ps, w, h, negative, layers, pad, gap in _cases():
        buf, first, pitch, layer_off = _buffer(rng, w, h, layers, ps, pad=pad, negative=negative, gap=gap)
        px = _pixels(buf, first, pitch, layer_off, w, h, layers, ps)
        for fn in (F.flip, F.flip_loops):
            hz = fn(buf.copy(), first, pitch, layer_off, w, h, layers, ps, 0)
            assert np.array_equal(_pixels(hz, first, pitch, layer_off, w, h, layers, ps), px[:, :, ::-1])
            vt = fn(buf.copy(), first, pitch, layer_off, w, h, layers, ps, 1)
            assert np.array_equal(_pixels(vt, first, pitch, layer_off, w, h, layers, ps), px[:, ::-1])
            both = fn(hz, first, pitch, layer_off, w, h, layers, ps, 1)
            assert np.array_equal(_pixels(both, first, pitch, layer_off, w, h, layers, ps), px[:, ::-1, ::-1])


def test_degenerate_sizes_and_one_row_with_any_pitch():
    rng = np.random.default_rng(34)
    buf = rng.integers(0, 256, 256, dtype=np.uint8)
    for fn in (F.flip, F.flip_loops):
        for w, h, layers in [(0, 3, 1), (3, 0, 1), (3, 3, 0)]:
            assert np.array_equal(fn(buf.copy(), 64, 16, 64, w, h, layers, 4, 0), buf)
        for pitch in (0, -5, 3):                               # h == 1: the pitch is never used
            got = fn(buf.copy(), 64, pitch, 0, 5, 1, 1, 3, 0)
            exp = buf.copy(); exp[64:79] = buf[64:79].reshape(5, 3)[::-1].reshape(-1)
            assert np.array_equal(got, exp)
            assert np.array_equal(fn(buf.copy(), 64, pitch, 0, 5, 1, 1, 3, 1), buf)
    with pytest.raises(AssertionError):
        F.flip(buf.copy(), 64, 8, 0, 3, 2, 1, 4, 1)            # overlapping scanlines are outside the contract
    with pytest.raises(AssertionError):
        F.flip(buf.copy(), 8, -16, 0, 2, 2, 1, 4, 1)           # a row below the buffer


def test_large_row_count_is_cheap():
    """the 131 075-row case of the GPU tests, vectorised against closed-form indexing"""
    w, h, ps = 3, 131075, 3
    size, first, pitch, layer_off = F.layout(w, h, 2, ps, pad=2, gap=5)
    buf = np.random.default_rng(35).integers(0, 256, size, dtype=np.uint8)
    got = F.flip(buf.copy(), first, pitch, layer_off, w, h, 2, ps, 1)
    for layer in range(2):
        for y in (0, 1, 65534, 65535, 65536, 65537, 131073, 131074):
            a, b = first + layer * layer_off + y * pitch, first + layer * layer_off + (h - 1 - y) * pitch
            assert np.array_equal(got[a:a + 9], buf[b:b + 9]) and np.array_equal(got[a + 9:a + 11], buf[a + 9:a + 11])
