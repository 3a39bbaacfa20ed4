"""GPU parity of flip.hip through the C ABI: gamut_hip_flip_device (pixels in HBM, signed pitch, layers), the host drop-in
gamut_hip_flip, and Image.flipHorizontal / flipVertical on top of them, against tests/flip_ref.py.

Every device case fills the WHOLE allocation -- pixel rows, row pads, the gaps between layers and a guard region on both sides --
with seeded random bytes, flips in place, and compares the whole allocation byte for byte with the reference applied to the
same host bytes: a swap that lands anywhere it should not is seen, not only one that is missing."""
import ctypes as C

import numpy as np
import pytest

import flip_ref as F
from oracle_lib import PT, PT_SIZE

pytestmark = pytest.mark.gpu

# one pixel type of every pixel size flip.hip instantiates (1, 2, 3, 4, 6, 8, 12, 16 bytes)
TYPE_OF_SIZE = {1: "l8", 2: "l16", 3: "rgb8", 4: "rgba8", 6: "rgb16", 8: "rgba16", 12: "rgbf32", 16: "rgbaf32"}
assert all(PT_SIZE[PT[t]] == s for s, t in TYPE_OF_SIZE.items())


class DevBuf:
    def __init__(self, L, host):
        from gamut_amd import _capi
        self.L, self.n = L, host.size
        self.p = L.gamut_hip_device_malloc(max(1, host.size))
        assert self.p
        _capi.check(L.gamut_hip_memcpy_h2d(self.p, host.ctypes.data, host.size, None))
        _capi.check(L.gamut_hip_stream_synchronize(None))

    def get(self):
        from gamut_amd import _capi
        out = np.empty(self.n, np.uint8)
        _capi.check(self.L.gamut_hip_stream_synchronize(None))
        _capi.check(self.L.gamut_hip_memcpy_d2h(out.ctypes.data, self.p, self.n, None))
        _capi.check(self.L.gamut_hip_stream_synchronize(None))
        return out

    def free(self):
        self.L.gamut_hip_device_free(self.p)


def _differs(got, exp, what):
    if np.array_equal(got, exp):
        return
    bad = np.flatnonzero(got != exp)
    raise AssertionError(f"{what}: {bad.size} of {exp.size} bytes differ, first at {bad[:8].tolist()}; got {got[bad[:8]].tolist()} "
                         f"exp {exp[bad[:8]].tolist()}")


def _flip_device(L, rng, tname, w, h, layers, vertical, **geometry):
    """random allocation of the given geometry (flip_ref.layout), flipped in place on the device, against the reference"""
    from gamut_amd import _capi
    t = PT[tname]
    ps = PT_SIZE[t]
    size, first, pitch, layer_off = F.layout(w, h, layers, ps, **geometry)
    host = rng.integers(0, 256, size, dtype=np.uint8)
    dev = DevBuf(L, host)
    try:
        _capi.check(L.gamut_hip_flip_device(t, dev.p + first, pitch, layer_off, w, h, layers, vertical, None))
        got = dev.get()
    finally:
        dev.free()
    exp = F.flip(host.copy(), first, pitch, layer_off, w, h, layers, ps, vertical)
    _differs(got, exp, f"{tname} {w}x{h}x{layers} {'vertical' if vertical else 'horizontal'} pitch={pitch} layer_off={layer_off} first={first}")


# ---------------------------------------------------------------- gamut_hip_flip_device
@pytest.mark.parametrize("ps", sorted(TYPE_OF_SIZE))
def test_every_pixel_size_and_width(hip, ps):
    """widths either side of one and two blocks of swaps (w / 2 = 255, 256, 257 and 512) and one with gridDim.x = 4 for the
    horizontal flip; the vertical flip of the same rows runs 1 to 97 blocks per row"""
    rng = np.random.default_rng(100 + ps)
    n = 0
    for w in (1, 2, 3, 511, 512, 513, 514, 1025, 1539):
        for h in (1, 2, 3, 8):
            for layers in (1, 3):
                pad = (0, 5, 4, 16)[n % 4]
                gap = 0 if layers == 1 else (12, 7)[n % 2]
                for vertical in (0, 1):
                    _flip_device(hip, rng, TYPE_OF_SIZE[ps], w, h, layers, vertical, pad=pad, gap=gap)
                n += 1


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("h", [65535, 65536, 65537, 131071])
def test_horizontal_row_chunks(hip, h, layers):
    """more rows than gridDim.y holds: the second (and third) launch starts at row 65535 (131070) of every layer"""
    rng = np.random.default_rng(200 + h + layers)
    for tname, w, pad in (("rgba8", 2, 0), ("rgb8", 3, 1), ("rgbaf32", 4, 0), ("l16", 5, 3)):
        _flip_device(hip, rng, tname, w, h, layers, 0, pad=pad, gap=0 if layers == 1 else 9)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("h", [131070, 131071, 131072, 131075])
def test_vertical_row_chunks(hip, h, layers):
    """h / 2 either side of 65535 row pairs: the later launches swap rows y0 + y and H - 1 - y0 - y.  Rows of 4 and 8 aligned
    bytes (k_flip_v<4>) and of 3 and 5 bytes (k_flip_v<1>)"""
    rng = np.random.default_rng(300 + h + layers)
    for tname, w, pad, gap in (("l16", 2, 0, 8), ("rgba8", 2, 4, 0), ("rgb8", 1, 0, 0), ("l8", 3, 2, 7), ("l8", 5, 0, 3)):
        _flip_device(hip, rng, tname, w, h, layers, 1, pad=pad, gap=gap if layers > 1 else 0)


def test_vertical_dword_or_byte_choice(hip):
    """k_flip_v moves dwords only when the row length, the pitch, the layer offset and the base address are all multiples of 4:
    from a case where all four hold, break one at a time.  Rows of 1200 bytes: two blocks of dwords, five of bytes."""
    rng = np.random.default_rng(400)
    h, layers = 6, 2

    def gap_for(step, want):                                   # gap that makes (step * h + gap) % 4 == want
        return (want - step * h) % 4 + 4

    for tname in ("rgba8", "rgbaf32", "rgbf32", "l16"):
        ps = PT_SIZE[PT[tname]]
        w = 1200 // ps
        _flip_device(hip, rng, tname, w, h, layers, 1, pad=8, gap=gap_for(w * ps + 8, 0))                       # all four hold
        _flip_device(hip, rng, tname, w, h, layers, 1, pad=0, gap=gap_for(w * ps, 0))
        for pad in (1, 2, 3):                                                                                   # pitch % 4 != 0
            _flip_device(hip, rng, tname, w, h, layers, 1, pad=pad, gap=gap_for(w * ps + pad, 0))
        for rem in (1, 2, 3):                                                                                   # layer_off % 4 != 0
            _flip_device(hip, rng, tname, w, h, layers, 1, pad=8, gap=gap_for(w * ps + 8, rem))
        for lead in (1, 2, 3):                                                                                  # base address % 4 != 0
            _flip_device(hip, rng, tname, w, h, layers, 1, pad=8, gap=gap_for(w * ps + 8, 0), lead=lead)
            _flip_device(hip, rng, tname, w, h, 1, 1, pad=8, lead=lead)
    # scan % 4 != 0 with pitch, layer offset and base aligned: 1203, 1202 and 1201 bytes in rows 1204 apart
    for tname, w, pad in (("rgb8", 401, 1), ("l16", 601, 2), ("l8", 1201, 3)):
        step = w * PT_SIZE[PT[tname]] + pad
        assert step % 4 == 0
        _flip_device(hip, rng, tname, w, h, layers, 1, pad=pad, gap=gap_for(step, 0))
    # a misaligned layer offset does not matter when there is one layer only ... but the kernel may not assume so either way
    _flip_device(hip, rng, "rgba8", 300, h, 1, 1, pad=8)


@pytest.mark.parametrize("ps", sorted(TYPE_OF_SIZE))
def test_negative_pitch_padded_rows_odd_base(hip, ps):
    """rows stored bottom-up: the pointer is at the highest-address row and the pitch is negative; padded rows, a base that is
    no multiple of 4, both directions"""
    rng = np.random.default_rng(500 + ps)
    for w in (5, 514, 1025):
        for h in (2, 7):
            for layers, gap in ((1, 0), (2, 5)):
                for lead, pad in ((1, 3), (3, 1), (0, 4), (2, 0)):
                    for vertical in (0, 1):
                        _flip_device(hip, rng, TYPE_OF_SIZE[ps], w, h, layers, vertical, pad=pad, gap=gap, lead=lead, negative=True)


def test_layer_limit(hip):
    """65535 layers (gridDim.z's limit) flip; one more is refused before anything is launched"""
    from gamut_amd import _capi
    rng = np.random.default_rng(600)
    for gap in (0, 1):
        for vertical in (0, 1):
            _flip_device(hip, rng, "l8", 2, 2, 65535, vertical, gap=gap)
    size, first, pitch, layer_off = F.layout(2, 2, 65536, 1)
    host = rng.integers(0, 256, size, dtype=np.uint8)
    dev = DevBuf(hip, host)
    try:
        for vertical in (0, 1):
            assert hip.gamut_hip_flip_device(PT["l8"], dev.p + first, pitch, layer_off, 2, 2, 65536, vertical, None) == _capi.ERR_UNSUPPORTED
            assert b"65535 layers" in hip.gamut_hip_last_error()
        _differs(dev.get(), host, "refused call")
    finally:
        dev.free()


def test_device_degenerate_and_error_contract(hip):
    from gamut_amd import _capi
    rng = np.random.default_rng(700)
    t = PT["rgba8"]
    for vertical in (0, 1):
        for w, h, layers in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (0, 0, 0)):
            assert hip.gamut_hip_flip_device(t, None, 16, 64, w, h, layers, vertical, None) == _capi.OK
    size, first, pitch, layer_off = F.layout(4, 4, 1, 4)
    host = rng.integers(0, 256, size, dtype=np.uint8)
    dev = DevBuf(hip, host)
    try:
        for vertical in (0, 1):
            for w, h, layers in ((-1, 4, 1), (4, -1, 1), (4, 4, -1)):
                assert hip.gamut_hip_flip_device(t, dev.p + first, pitch, layer_off, w, h, layers, vertical, None) == _capi.ERR_INVALID_ARG
                assert b"flip" in hip.gamut_hip_last_error()
            for bad_type in (-1, 18, 1000):
                assert hip.gamut_hip_flip_device(bad_type, dev.p + first, pitch, layer_off, 4, 4, 1, vertical, None) == _capi.ERR_INVALID_ARG
                assert b"flip" in hip.gamut_hip_last_error()
            assert hip.gamut_hip_flip_device(t, None, pitch, layer_off, 4, 4, 1, vertical, None) == _capi.ERR_INVALID_ARG
            assert b"null" in hip.gamut_hip_last_error()
        _differs(dev.get(), host, "refused calls")
        # one column has nothing to swap horizontally, one row nothing vertically: OK, and not a byte moves
        assert hip.gamut_hip_flip_device(t, dev.p + first, pitch, layer_off, 1, 4, 1, 0, None) == _capi.OK
        assert hip.gamut_hip_flip_device(t, dev.p + first, pitch, layer_off, 4, 1, 1, 1, None) == _capi.OK
        assert hip.gamut_hip_last_error() == b""
        _differs(dev.get(), host, "no-op calls")
    finally:
        dev.free()


def test_flips_keep_stream_order(hip):
    """rgba8 -> rgba16 into B, flip B both ways, B -> rgba8 into C, all on one created stream without a synchronisation in
    between: each kernel must see what the one before it wrote.  3 MB in, 6 MB in B (padded rows)."""
    from gamut_amd import _capi
    L = hip
    w, h = 1024, 768
    rng = np.random.default_rng(800)
    src = rng.integers(0, 256, w * h * 4, dtype=np.uint8)
    bpitch = w * 8 + 16
    a = DevBuf(L, src)
    b = DevBuf(L, np.zeros(bpitch * h, np.uint8))
    c = DevBuf(L, np.zeros(w * h * 4, np.uint8))
    st = L.gamut_hip_stream_create()
    assert st
    try:
        _capi.check(L.gamut_hip_scanlines_convert_device(PT["rgba8"], a.p, w * 4, 0, PT["rgba16"], b.p, bpitch, 0, w, h, 1, st))
        _capi.check(L.gamut_hip_flip_device(PT["rgba16"], b.p, bpitch, 0, w, h, 1, 0, st))
        _capi.check(L.gamut_hip_flip_device(PT["rgba16"], b.p, bpitch, 0, w, h, 1, 1, st))
        _capi.check(L.gamut_hip_scanlines_convert_device(PT["rgba16"], b.p, bpitch, 0, PT["rgba8"], c.p, w * 4, 0, w, h, 1, st))
        _capi.check(L.gamut_hip_stream_synchronize(st))
        got = c.get()
    finally:
        L.gamut_hip_stream_destroy(st)
        for buf in (a, b, c):
            buf.free()
    _differs(got, src.reshape(h, w, 4)[::-1, ::-1].reshape(-1), "convert, flip, flip, convert on one stream")


# ---------------------------------------------------------------- gamut_hip_flip (host rows)
def test_host_dropin_pitches_and_pads(hip):
    """host pointers with the row's own pitch, an odd pad, and bottom-up storage: the whole numpy buffer, pads and guards
    included, equals the reference"""
    from gamut_amd import _capi
    rng = np.random.default_rng(900)
    for tname in ("l8", "la16", "rgb8", "rgb16", "rgbf32", "rgbaf32"):
        t = PT[tname]
        ps = PT_SIZE[t]
        for w, h in ((1, 1), (2, 1), (37, 1), (1, 9), (2, 2), (37, 9), (300, 4), (700, 3)):
            for pad, negative in ((0, False), (5, False), (3, True), (0, True)):
                for vertical in (0, 1):
                    size, first, pitch, _ = F.layout(w, h, 1, ps, pad=pad, negative=negative)
                    pitches = [pitch] if h > 1 else [pitch, 0, -pitch, -1]          # one row: the pitch is never used
                    for pt in pitches:
                        buf = rng.integers(0, 256, size, dtype=np.uint8)
                        exp = F.flip(buf.copy(), first, pt, 0, w, h, 1, ps, vertical)
                        _capi.check(hip.gamut_hip_flip(t, buf.ctypes.data + first, pt, w, h, vertical))
                        _differs(buf, exp, f"{tname} {w}x{h} pitch={pt} vertical={vertical}")


def test_host_dropin_error_contract(hip):
    from gamut_amd import _capi
    rng = np.random.default_rng(901)
    t = PT["rgb8"]
    size, first, pitch, _ = F.layout(10, 4, 1, 3, pad=2)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    keep = buf.copy()
    p = buf.ctypes.data + first
    for vertical in (0, 1):
        for bad in (29, -29, 3, 0, -1):                        # |pitch| < 30 bytes of row, more than one row
            assert hip.gamut_hip_flip(t, p, bad, 10, 4, vertical) == _capi.ERR_INVALID_ARG
            assert b"overlapping" in hip.gamut_hip_last_error()
        for w, h in ((0, 4), (10, 0), (0, 0)):
            assert hip.gamut_hip_flip(t, None, 0, w, h, vertical) == _capi.OK
        for w, h in ((-1, 4), (10, -1)):
            assert hip.gamut_hip_flip(t, p, pitch, w, h, vertical) == _capi.ERR_INVALID_ARG
            assert b"flip" in hip.gamut_hip_last_error()
        for bad_type in (-1, 18):
            assert hip.gamut_hip_flip(bad_type, p, pitch, 10, 4, vertical) == _capi.ERR_INVALID_ARG
            assert b"flip" in hip.gamut_hip_last_error()
        assert hip.gamut_hip_flip(t, None, pitch, 10, 4, vertical) == _capi.ERR_INVALID_ARG
        assert b"null" in hip.gamut_hip_last_error()
    assert np.array_equal(buf, keep), "a refused call wrote to the buffer"


# ---------------------------------------------------------------- Image
@pytest.mark.parametrize("vert", ["straight", "flipped"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_image_flips_with_border_alignment_and_layers(hip, device, vert):
    """700 x 300 rgb16, 3 layers, a 1-pixel border, rows aligned to 128 bytes, storage order pinned (flipVertical is then the
    physical flip): flipHorizontal then flipVertical against the reference over the whole extent of the storage the image's own
    numbers describe -- borders, alignment pads and all -- so the bytes outside the pixel rows are seen not to move."""
    from gamut_amd import _capi
    from gamut_amd import image as gi
    w, h, layers, frame = 700, 300, 3, 1
    t = PT["rgb16"]
    ps = PT_SIZE[t]
    layout = gi.LAYOUT_BORDER[frame] | gi.LAYOUT_ALIGNED[128] | (gi.LAYOUT_VERT_STRAIGHT if vert == "straight" else gi.LAYOUT_VERT_FLIPPED)
    im = gi.Image(device=device)
    assert im.createLayered(w, h, layers, t, layout), im.errorMessage
    pitch, layer_off = im.pitchInBytes, im.layerOffsetInBytes
    step = abs(pitch)
    assert (pitch < 0) == (vert == "flipped") and step % 128 == 0 and step >= (w + 2 * frame) * ps and layer_off == step * (h + 2 * frame)
    assert im.layerptr(1, 0) - im.layerptr(0, 0) == layer_off and im.layerptr(0, 1) - im.layerptr(0, 0) == pitch
    # the storage from the first byte of layer 0's top border row to the end of the last layer's bottom border row
    lowest_row = min(im.layerptr(0, 0), im.layerptr(0, h - 1))
    start = lowest_row - frame * step - frame * ps
    extent = layer_off * layers
    first = im.layerptr(0, 0) - start
    rng = np.random.default_rng(1000 + device)
    host = rng.integers(0, 256, extent, dtype=np.uint8)
    if device:
        _capi.check(hip.gamut_hip_memcpy_h2d(start, host.ctypes.data, extent, None))
        _capi.check(hip.gamut_hip_stream_synchronize(None))
    else:
        C.memmove(start, host.ctypes.data, extent)

    def storage():
        out = np.empty(extent, np.uint8)
        if device:
            _capi.check(hip.gamut_hip_stream_synchronize(None))
            _capi.check(hip.gamut_hip_memcpy_d2h(out.ctypes.data, start, extent, None))
            _capi.check(hip.gamut_hip_stream_synchronize(None))
        else:
            C.memmove(out.ctypes.data, start, extent)
        return out

    rows = np.zeros(extent, bool)
    for layer in range(layers):
        for y in range(h):
            at = first + layer * layer_off + y * pitch
            rows[at:at + w * ps] = True
    exp = host.copy()
    for vertical, call in ((0, im.flipHorizontal), (1, im.flipVertical)):
        assert call(), im.errorMessage
        assert (im.pitchInBytes, im.layerOffsetInBytes, im.layerptr(0, 0) - start) == (pitch, layer_off, first), "the constraint pins the storage"
        F.flip(exp, first, pitch, layer_off, w, h, layers, ps, vertical)
        got = storage()
        for layer in range(layers):
            lo = layer * layer_off
            _differs(got[lo:lo + layer_off][rows[lo:lo + layer_off]], exp[lo:lo + layer_off][rows[lo:lo + layer_off]], f"layer {layer} after flip {vertical}")
            want = np.stack([exp[first + lo + y * pitch:][:w * ps] for y in range(h)])
            assert np.array_equal(im.pixels(layer), want), f"pixels({layer}) after flip {vertical}"
        _differs(got[~rows], host[~rows], f"bytes outside the pixel rows after flip {vertical}")
        _differs(got, exp, f"whole storage after flip {vertical}")
    src = np.stack([np.stack([host[first + l * layer_off + y * pitch:][:w * ps] for y in range(h)]) for l in range(layers)])
    for layer in range(layers):
        assert np.array_equal(im.pixels(layer), src[layer].reshape(h, w, ps)[::-1, ::-1].reshape(h, w * ps))
