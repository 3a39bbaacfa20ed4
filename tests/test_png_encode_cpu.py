"""PNG encode without a device: the serial restatement of the reference's writer (tests/c/png_write_ref.c) pinned to independent readers
(Pillow, the oracle's PNG decoder) and to hand-computed filtered bytes; header / Python / D binding agreement for the new symbols; the
bound formula; every refusal; the loud failure when there is no GPU; and the generic save entry, which does not dispatch PNG yet."""
import ctypes as C
import io
import os
import re
import zlib

import numpy as np
import pytest

import oracle_lib as O
import png_write_ref_c as PW
from gamut_amd import _capi
from gamut_amd import image as gi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("gamut_hip_png_encode_bound", "gamut_hip_png_write_to_mem", "gamut_hip_png_encode_batch_device")


def _rand(rng, h, w, c, dt):
    return rng.integers(0, 256 if dt == np.uint8 else 65536, (h, w, c)).astype(dt)


def test_restatement_against_independent_readers():
    """every (comp, is16bit), forced filters 0..4 and the heuristic, shapes including 1x1, 1xN, Nx1: the file around zlib.compress(filt)
    decodes in the oracle's PNG decoder and in Pillow to the input pixels"""
    from PIL import Image
    rng = np.random.default_rng(20261016)
    for h, w in ((1, 1), (1, 13), (13, 1), (6, 9), (17, 5)):
        for c in (1, 2, 3, 4):
            for dt in (np.uint8, np.uint16):
                px = _rand(rng, h, w, c, dt)
                if (h + w + c) % 2:
                    px = (px // 64 * 64).astype(dt)                     # few levels: the filters disagree more often
                for ff in (-1, 0, 1, 2, 3, 4):
                    data = PW.encode(px, ff)
                    got, n = O.stbi_load(data, 0, dt == np.uint16)
                    assert n == c and np.array_equal(got, px), (h, w, c, dt, ff)
                    im = Image.open(io.BytesIO(data)); im.load()
                    assert im.size == (w, h)
                    if dt == np.uint8:                                  # (Pillow reduces 16-bit colour on load; 8-bit it returns as is)
                        assert np.array_equal(np.asarray(im).reshape(h, w, c), px), (h, w, c, ff)
                    elif c == 1:
                        assert np.array_equal(np.asarray(im).astype(np.uint16).reshape(h, w, 1), px)
                    # the filter stream has one type byte per row, and forced types are written as given
                    f = PW.filt(px, ff)
                    types = f[::w * c * px.dtype.itemsize + 1]
                    assert len(f) == (w * c * px.dtype.itemsize + 1) * h
                    assert set(types) <= ({ff} if ff >= 0 else {0, 1, 2, 3, 4})
    assert PW.filt(px, 5) == PW.filt(px, -1) == PW.filt(px, 99)         # >= 5 selects (:365)


def test_hand_computed_16_bit_estimate():
    """The estimate sums |(int8)line[i]| over i < x * n (:394): for 16-bit rows that is the FIRST HALF of the row, taken AFTER the byte
    swap.  Tiny l16 images, bytes worked out by hand, that separate this from the two plausible misreadings."""
    # (a) against "over the whole row".  2 x 2, row 1 = [0x0303, 0x0303] under [0x0000, 0x0303]; candidates as big-endian bytes:
    #       None 03 03 03 03   Sub 03 03 00 00   Up 03 03 00 00   Average 03 03 00 00   Paeth 03 03 00 00
    #     first half (2 bytes): every candidate 6 -> the first one, None, stays.  Whole row: None 12, Sub 6 -> Sub.
    a = np.array([[[0x0000], [0x0303]], [[0x0303], [0x0303]]], np.uint16)
    assert PW.filt(a)[5:] == bytes([0, 3, 3, 3, 3])
    # (b) against "first half BEFORE the swap".  1 x 2 (x * n = 1: one byte of the two), row 1 = [0x0540] under [0x0500]:
    #       native (lo, hi): None 40 05   Sub 40 05   Up 40 00   Average 40 03 (05 - (05 >> 1))   Paeth 40 00
    #     after the swap byte 0 is the high byte: None 5, Sub 5, Up 0 -> Up, written 00 40.  Before the swap byte 0 would be 0x40 for
    #     every candidate: a tie, None.
    b = np.array([[[0x0500]], [[0x0540]]], np.uint16)
    assert PW.filt(b) == bytes([0, 0x05, 0x00, 2, 0x00, 0x40])
    # (c) both bytes of a sample count: row 1 = [0x0040, 0x0000] under itself.  None 00 40 | 00 00 = 64, Sub the same, Up 0 -> Up.
    #     Counting high bytes only would tie at 0 and keep None.
    c = np.array([[[0x0040], [0x0000]], [[0x0040], [0x0000]]], np.uint16)
    assert PW.filt(c)[5:] == bytes([2, 0, 0, 0, 0])
    # (d) row 0 of a 16-bit image (firstmap): [0x0104, 0x0005] -> None 01 04 00 05 (5), Sub 01 04 FF 01 (5), Up -> None (5),
    #     Average 01 04 00 03 (5), Paeth -> Sub (5): all tie, None; row 1 = [0x0105, 0x7F05]: None 01 05 (6), Sub 01 05 (6), Up 00 01 (1),
    #     Average 01 03 (4), Paeth 00 01 (1): Up comes before Paeth and wins the tie, bytes 00 01 7F 00.
    d = np.array([[[0x0104], [0x0005]], [[0x0105], [0x7F05]]], np.uint16)
    assert PW.filt(d) == bytes([0, 0x01, 0x04, 0x00, 0x05, 2, 0x00, 0x01, 0x7F, 0x00])


def test_row_zero_per_filter():
    """row 0 under each forced filter (firstmap, :279): Up -> copy, Average -> z - (left >> 1), Paeth -> z - left; the type byte stays"""
    px = np.array([[[10], [30], [100], [7]]], np.uint8)
    assert PW.filt(px, 0) == bytes([0, 10, 30, 100, 7])
    assert PW.filt(px, 1) == bytes([1, 10, 20, 70, (7 - 100) & 255])
    assert PW.filt(px, 2) == bytes([2, 10, 30, 100, 7])
    assert PW.filt(px, 3) == bytes([3, 10, 30 - 5, 100 - 15, (7 - 50) & 255])
    assert PW.filt(px, 4) == bytes([4, 10, 20, 70, (7 - 100) & 255])
    px16 = np.array([[[0x1234], [0x1334]]], np.uint16)                   # l16: left is the previous sample, bytewise; big-endian out
    assert PW.filt(px16, 0) == bytes([0, 0x12, 0x34, 0x13, 0x34])
    assert PW.filt(px16, 1) == bytes([1, 0x12, 0x34, 0x01, 0x00])
    assert PW.filt(px16, 3) == bytes([3, 0x12, 0x34, 0x13 - 0x09, 0x34 - 0x1A])


def test_header_python_and_d_binding_agree():
    header = open(os.path.join(ROOT, "include", "gamut_hip.h")).read()
    dtext = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    raw = C.CDLL(_capi.LIB_PATH)
    nargs = {"gamut_hip_png_encode_bound": 4, "gamut_hip_png_write_to_mem": 9, "gamut_hip_png_encode_batch_device": 14}
    for name in NEW:
        assert hasattr(raw, name) and name in _capi.SIGNATURES
        c = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
        d = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", dtext, re.S).group(1)
        strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
        assert len(strip(c).split(",")) == len(d.split(",")) == len(_capi.SIGNATURES[name][1]) == nargs[name], name
    assert _capi.SIGNATURES["gamut_hip_png_encode_bound"][0] is C.c_int64
    header2 = open(os.path.join(ROOT, "include", "gamut_image.h")).read()
    for name in ("gamut_image_save_png_to_memory", "gamut_image_save_png_to_file"):
        assert name in header2 and name in gi.IMAGE_SIGNATURES and hasattr(raw, name)
    assert "PNG has no encoder" not in header2
    for k in range(11):
        assert re.search(r"GAMUT_ENCODE_PNG_COMPRESSION_%d = %d\b" % (k, k + 1), header2) and getattr(gi, "ENCODE_PNG_COMPRESSION_%d" % k) == k + 1
    assert "GAMUT_ENCODE_PNG_FILTER_FAST = 16" in header2 and gi.ENCODE_PNG_FILTER_FAST == 16
    assert (gi.ENCODE_PNG_COMPRESSION_DEFAULT, gi.ENCODE_PNG_COMPRESSION_FAST, gi.ENCODE_PNG_COMPRESSION_SMALL) == (0, 2, 10)


def test_encode_bound():
    b = _capi.lib().gamut_hip_png_encode_bound
    def f(w, h, c, s):
        L = (w * c * (2 if s else 1) + 1) * h
        return 57 + 6 + L + 5 * (-(-L // 8192))
    assert b(1, 1, 1, 0) == f(1, 1, 1, 0) == 57 + 6 + 2 + 5
    assert b(1920, 1080, 4, 0) == f(1920, 1080, 4, 0) == PW.bound(1920, 1080, 4, 0)
    assert b(1920, 1080, 3, 1) == f(1920, 1080, 3, 1)
    assert b(8191, 1, 1, 0) == 63 + 8192 + 5 and b(8192, 1, 1, 0) == 63 + 8193 + 10
    assert b(7, 5, 2, 7) == f(7, 5, 2, 1)                               # is16bit is a truth value
    # refusals
    assert b(0, 5, 3, 0) == 0 and b(5, 0, 3, 0) == 0 and b(-1, 5, 3, 0) == 0 and b(5, 5, 0, 0) == 0 and b(5, 5, 5, 0) == 0
    # (lineBytes + 1) * h must fit a positive int
    assert b(65535, 65535, 1, 0) == 0                                   # 65536 * 65535 > INT_MAX
    assert b(32767, 65535, 1, 0) == f(32767, 65535, 1, 0)               # 32768 * 65535 = 2147450880 <= INT_MAX
    assert b(32767, 65536, 1, 0) == 0                                   # 2^31
    assert b(1 << 20, 1 << 10, 4, 1) == 0
    assert b(2147483646, 1, 1, 0) == f(2147483646, 1, 1, 0) and b(2147483647, 1, 1, 0) == 0


def test_argument_validation_without_device():
    L = _capi.lib()
    f = L.gamut_hip_png_encode_batch_device
    assert f(None, None, None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK                 # empty batch
    assert f(None, None, None, None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert f(None, None, None, None, None, None, None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    src = (C.c_void_p * 1)(0x1000); pitch = (C.c_int64 * 1)(8); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(0)
    two = (C.c_int * 1)(2); three = (C.c_int * 1)(3); zero = (C.c_int * 1)(0)
    assert f(src, pitch, two, two, three, zero, None, None, 1, off, None, ln, None, None) == _capi.ERR_INVALID_ARG           # no output
    assert f(src, pitch, two, two, three, zero, None, None, 1, off, 0x2000, None, None, None) == _capi.ERR_INVALID_ARG       # no lengths
    assert f(src, pitch, None, two, three, zero, None, None, 1, off, 0x2000, ln, None, None) == _capi.ERR_INVALID_ARG        # no widths
    assert f(src, pitch, two, two, three, None, None, None, 1, off, 0x2000, ln, None, None) == _capi.ERR_INVALID_ARG         # no is16bit
    assert b"bad arguments" in L.gamut_hip_last_error()
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    w = L.gamut_hip_png_write_to_mem
    assert not w(None, 6, 2, 2, 3, C.byref(n), 0, -1, 5)
    assert not w(px.ctypes.data, 6, 2, 2, 3, None, 0, -1, 5)
    assert not w(px.ctypes.data, 6, 2, 2, 5, C.byref(n), 0, -1, 5) and not w(px.ctypes.data, 6, 2, 2, 0, C.byref(n), 0, -1, 5)
    assert not w(px.ctypes.data, 6, 0, 2, 3, C.byref(n), 0, -1, 5) and not w(px.ctypes.data, 6, 2, -1, 3, C.byref(n), 0, -1, 5)
    assert not w(px.ctypes.data, 6, 2, 2, 3, C.byref(n), 0, -1, 11) and not w(px.ctypes.data, 6, 2, 2, 3, C.byref(n), 0, -1, -1)
    assert not w(px.ctypes.data, 6, 65535, 65535, 1, C.byref(n), 0, -1, 5)
    assert b"invalid arguments" in L.gamut_hip_last_error() and n.value == -1


def test_no_device_is_a_loud_failure():
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_png_write_to_mem(px.ctypes.data, 6, 2, 2, 3, C.byref(n), 0, -1, 5)
    assert b"no HIP device" in L.gamut_hip_last_error() and n.value == -1
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(6); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1)
    w = (C.c_int * 1)(2); comp = (C.c_int * 1)(3); zero = (C.c_int * 1)(0)
    out = np.full(4096, 0xA5, np.uint8); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_png_encode_batch_device(src, pitch, w, w, comp, zero, None, None, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    assert (out == 0xA5).all()
    for type_, bpp in ((0, 1), (9, 3), (12, 4), (13, 8)):
        img = gi.Image()
        assert img.createView(np.zeros((2, 2 * bpp), np.uint8), 2, 2, type_, 2 * bpp)
        assert img.save_png_to_memory() is None
        assert img.isValid and img.errorMessage is None


def test_image_refusals_and_generic_entry():
    img = gi.Image()
    assert img.save_png_to_memory() is None                              # errored ("Uninitialized image")
    assert not img.savePNGToFile("/nonexistent-dir/x.png")
    for type_, bpp in ((2, 4), (5, 8), (6, 2), (11, 12), (14, 16), (15, 4), (17, 16)):      # fp32 and premultiplied types
        img = gi.Image()
        assert img.createView(np.zeros((3, 3 * bpp), np.uint8), 3, 3, type_, 3 * bpp)
        assert img.save_png_to_memory() is None
        assert img.isValid and img.errorMessage is None
    img = gi.Image()
    assert img.createView(np.zeros((3, 12), np.uint8), 3, 3, 12, 12)
    for flags in (12, 13, 14, 15, 12 | 16, 15 | 16):                    # level = (flags & 15) - 1 above 10
        assert img.save_png_to_memory(flags) is None and img.isValid
    assert img.save_to_memory(gi.FORMAT_PNG) is None                    # not dispatched from the generic entry in this change
    assert img.isValid and img.errorMessage is None
