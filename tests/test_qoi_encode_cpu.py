"""QOI encode without a device: the worst-case bound and its refusals (qoi.d:303-315), argument checks of the C ABI, the loud failure
when there is no GPU, the Image mirror's refusals, and the pinning of Pillow's QOI writer to tests/gen.py's serial encoder (Pillow is
the oracle of the GPU tests' large images, where gen.qoi_encode is too slow)."""
import ctypes as C
import io

import numpy as np
import pytest

import gen
from gamut_amd import _capi
from gamut_amd import image as gi


def desc(w, h, ch=4, cs=0):
    d = _capi.QoiDesc()
    d.width, d.height, d.channels, d.colorspace = w, h, ch, cs
    return d


def test_encode_bound():
    L = _capi.lib()
    b = lambda *a: L.gamut_hip_qoi_encode_bound(C.byref(desc(*a)))
    assert b(1, 1, 4) == 1 * 1 * 5 + 22
    assert b(3, 7, 3) == 3 * 7 * 4 + 22
    assert b(1920, 1080, 4, 1) == 1920 * 1080 * 5 + 22
    assert b(0, 5) == 0 and b(5, 0) == 0
    assert b(5, 5, 2) == 0 and b(5, 5, 5) == 0 and b(5, 5, 1) == 0
    assert b(5, 5, 4, 2) == 0
    # height >= 400000000 / width (u32 division) is refused
    w = 20000
    assert b(w, 400000000 // w - 1, 4) == w * (400000000 // w - 1) * 5 + 22
    assert b(w, 400000000 // w, 4) == 0
    w = 7                                                          # 400000000 / 7 = 57142857 (truncated)
    assert b(w, 57142856, 3) == w * 57142856 * 4 + 22
    assert b(w, 57142857, 3) == 0
    assert b(1, 399999999, 4) == 399999999 * 5 + 22               # beyond 2^31: int64
    assert L.gamut_hip_qoi_encode_bound(None) == 0


def test_argument_validation_without_device():
    L = _capi.lib()
    assert L.gamut_hip_qoi_encode_batch_device(None, None, None, 0, None, None, None, None, None) == _capi.OK       # empty batch
    assert L.gamut_hip_qoi_encode_batch_device(None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_qoi_encode_batch_device(None, None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    d = (_capi.QoiDesc * 1)(desc(2, 2))
    src = (C.c_void_p * 1)(0x1000); pitch = (C.c_int64 * 1)(8); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(0)
    assert L.gamut_hip_qoi_encode_batch_device(src, pitch, d, 1, off, None, ln, None, None) == _capi.ERR_INVALID_ARG      # no output
    assert L.gamut_hip_qoi_encode_batch_device(src, pitch, d, 1, off, 0x2000, None, None, None) == _capi.ERR_INVALID_ARG  # no lengths
    assert b"bad arguments" in L.gamut_hip_last_error()
    px = np.zeros(16, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoi_encode(None, C.byref(desc(2, 2)), 8, C.byref(n))
    assert not L.gamut_hip_qoi_encode(px.ctypes.data, None, 8, C.byref(n))
    assert not L.gamut_hip_qoi_encode(px.ctypes.data, C.byref(desc(2, 2)), 8, None)
    assert not L.gamut_hip_qoi_encode(px.ctypes.data, C.byref(desc(2, 2, 2)), 8, C.byref(n))
    assert b"invalid arguments" in L.gamut_hip_last_error() and n.value == -1


def test_no_device_is_a_loud_failure():
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = np.zeros(16, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoi_encode(px.ctypes.data, C.byref(desc(2, 2)), 8, C.byref(n))
    assert b"no HIP device" in L.gamut_hip_last_error() and n.value == -1
    d = (_capi.QoiDesc * 1)(desc(2, 2))
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(8); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1)
    out = np.full(64, 0xA5, np.uint8); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_qoi_encode_batch_device(src, pitch, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    assert (out == 0xA5).all()
    img = gi.Image()
    assert img.createView(np.zeros((2, 8), np.uint8), 2, 2, 12, 8)
    assert img.save_to_memory(gi.FORMAT_QOI) is None
    assert img.isValid and img.errorMessage is None


def test_image_save_refusals():
    img = gi.Image()
    assert img.save_to_memory(gi.FORMAT_QOI) is None                # errored ("Uninitialized image")
    assert img.errorMessage == "Uninitialized image"
    a16 = np.zeros((3, 4 * 8), np.uint8)
    img16 = gi.Image()
    assert img16.createView(a16, 4, 3, 13, 32)                     # rgba16
    assert img16.save_to_memory(gi.FORMAT_QOI) is None
    a8 = np.zeros((3, 4 * 4), np.uint8)
    img8 = gi.Image()
    assert img8.createView(a8, 4, 3, 12, 16)                       # rgba8: saveable as QOI only
    for fif in (gi.FORMAT_JPEG, gi.FORMAT_PNG, gi.FORMAT_UNKNOWN, 7):
        assert img8.save_to_memory(fif) is None
    assert img8.isValid and img8.type == 12 and img8.width == 4     # no side effect on the image
    grey = gi.Image()
    assert grey.createView(np.zeros((3, 4), np.uint8), 4, 3, 0, 4)   # l8
    assert grey.save_to_memory(gi.FORMAT_QOI) is None
    L = gi.lib()
    n = C.c_size_t(5)
    assert not L.gamut_image_save_to_memory(img16.h, gi.FORMAT_QOI, 0, C.byref(n)) and n.value == 0
    assert not L.gamut_image_save_to_file(img8.h, gi.FORMAT_PNG, b"/nonexistent/x.png", 0)
    L.gamut_free_encoded_image(None)


def _pillow_qoi(px):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, "RGBA" if px.shape[2] == 4 else "RGB").save(b, format="QOI")
    return b.getvalue()


def test_pillow_payload_equals_spec_encoder():
    """Pillow's QOI writer follows the reference's algorithm: its payload (bytes 14 on) equals gen.qoi_encode's on a few hundred small
    random images, palette ones included (runs, index hits, the leading (0,0,0,255) case); its header's colorspace byte is its own."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(2024)
    for it in range(300):
        ch = int(rng.integers(3, 5)); w = int(rng.integers(1, 24)); h = int(rng.integers(1, 10))
        pal = rng.integers(0, 256, (int(rng.integers(1, 6)), ch), dtype=np.uint8)
        if it % 3 == 0:
            pal[0] = (0, 0, 0, 255)[:ch]
        px = pal[rng.integers(0, len(pal), (h, w))] if it % 2 else rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        ours, pil = gen.qoi_encode(px), _pillow_qoi(px)
        assert pil[:13] == ours[:13], it
        assert pil[14:] == ours[14:], it
