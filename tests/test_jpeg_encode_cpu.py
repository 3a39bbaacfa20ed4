"""JPEG encode without a device: the worst-case bound and its refusals, argument checks of the C ABI, the loud failure when there is
no GPU, the Image mirror's refusals, and the two restatements of the reference's writer (tests/c/jpeg_write_ref.c and
tests/jpeg_encode_ref.py) pinned to each other, to the project's own decoders and to Pillow."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_encode_ref as R
import jpeg_write_ref_c as JW
import oracle_lib as O
from gamut_amd import _capi
from gamut_amd import image as gi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_encode_bound():
    L = _capi.lib()
    b = L.gamut_hip_jpeg_encode_bound
    blocks420 = lambda w, h: 6 * (-(-w // 16)) * (-(-h // 16))
    blocks444 = lambda w, h: 3 * (-(-w // 8)) * (-(-h // 8))
    f = lambda n: 607 + 2 * ((n * 1660 + 7) // 8) + 2
    assert b(1, 1, 3, 90) == f(6) == 607 + 2 * 1245 + 2
    assert b(1, 1, 3, 95) == f(3)
    assert b(1920, 1080, 3, 90) == f(blocks420(1920, 1080)) and blocks420(1920, 1080) == 48960
    assert b(1920, 1080, 4, 100) == f(blocks444(1920, 1080))
    assert b(65535, 65535, 1, 95) == f(blocks444(65535, 65535)) > 2 ** 32                  # int64
    # refusals: sizes, comp
    assert b(0, 5, 3, 90) == 0 and b(5, 0, 3, 90) == 0 and b(-1, 5, 3, 90) == 0
    assert b(5, 5, 0, 90) == 0 and b(5, 5, 5, 90) == 0
    assert b(65536, 1, 3, 90) == 0 and b(1, 65536, 3, 90) == 0 and b(65535, 1, 3, 90) == f(blocks420(65535, 1))
    # quality: 0 means 90; 4:2:0 decided before the clamp (<= 90), so -5 is 4:2:0 and 150 is 4:4:4
    w, h = 40, 24
    assert b(w, h, 3, 0) == b(w, h, 3, 90) == f(blocks420(w, h))
    assert b(w, h, 3, 91) == f(blocks444(w, h))
    assert b(w, h, 3, -5) == f(blocks420(w, h))
    assert b(w, h, 3, 150) == f(blocks444(w, h))
    assert blocks420(w, h) != blocks444(w, h)


def test_argument_validation_without_device():
    L = _capi.lib()
    f = L.gamut_hip_jpeg_encode_batch_device
    assert f(None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK                  # empty batch
    assert f(None, None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert f(None, None, None, None, None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    src = (C.c_void_p * 1)(0x1000); pitch = (C.c_int64 * 1)(8); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(0)
    one = (C.c_int * 1)(2); three = (C.c_int * 1)(3)
    assert f(src, pitch, one, one, three, None, 1, off, None, ln, None, None) == _capi.ERR_INVALID_ARG           # no output
    assert f(src, pitch, one, one, three, None, 1, off, 0x2000, None, None, None) == _capi.ERR_INVALID_ARG       # no lengths
    assert f(src, pitch, None, one, three, None, 1, off, 0x2000, ln, None, None) == _capi.ERR_INVALID_ARG        # no widths
    assert f(src, pitch, one, one, None, None, 1, off, 0x2000, ln, None, None) == _capi.ERR_INVALID_ARG          # no comps
    assert b"bad arguments" in L.gamut_hip_last_error()
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_jpeg_encode(None, 2, 2, 3, 6, 90, C.byref(n))
    assert not L.gamut_hip_jpeg_encode(px.ctypes.data, 2, 2, 3, 6, 90, None)
    assert not L.gamut_hip_jpeg_encode(px.ctypes.data, 2, 2, 5, 6, 90, C.byref(n))
    assert not L.gamut_hip_jpeg_encode(px.ctypes.data, 0, 2, 3, 6, 90, C.byref(n))
    assert not L.gamut_hip_jpeg_encode(px.ctypes.data, 65536, 1, 1, 65536, 90, C.byref(n))
    assert b"invalid arguments" in L.gamut_hip_last_error() and n.value == -1
    calls = []
    cb = _capi.JPEG_WRITE_FUNC(lambda ctx, data, size: calls.append(size))
    assert L.gamut_hip_jpeg_write_to_func(C.cast(cb, C.c_void_p), None, 2, 2, 0, px.ctypes.data, 6, 90) == 0
    assert L.gamut_hip_jpeg_write_to_func(C.cast(cb, C.c_void_p), None, 2, 2, 3, None, 6, 90) == 0
    assert L.gamut_hip_jpeg_write_to_func(None, None, 2, 2, 3, px.ctypes.data, 6, 90) == 0
    assert calls == []


def test_no_device_is_a_loud_failure():
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_jpeg_encode(px.ctypes.data, 2, 2, 3, 6, 90, C.byref(n))
    assert b"no HIP device" in L.gamut_hip_last_error() and n.value == -1
    calls = []
    cb = _capi.JPEG_WRITE_FUNC(lambda ctx, data, size: calls.append(size))
    assert L.gamut_hip_jpeg_write_to_func(C.cast(cb, C.c_void_p), None, 2, 2, 3, px.ctypes.data, 6, 90) == 0
    assert b"no HIP device" in L.gamut_hip_last_error() and calls == []
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(6); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1)
    w = (C.c_int * 1)(2); comp = (C.c_int * 1)(3)
    out = np.full(4096, 0xA5, np.uint8); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_jpeg_encode_batch_device(src, pitch, w, w, comp, None, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    assert (out == 0xA5).all()
    for t, ch in ((gi.Image, 1), (gi.Image, 3)):
        img = t()
        assert img.createView(np.zeros((2, 8), np.uint8), 2, 2, 0 if ch == 1 else 9, 8)      # l8 / rgb8
        assert img.save_to_memory(gi.FORMAT_JPEG) is None
        assert img.isValid and img.errorMessage is None


def test_image_save_refusals():
    img = gi.Image()
    assert img.save_to_memory(gi.FORMAT_JPEG) is None                # errored ("Uninitialized image")
    for type_, bpp in ((12, 4), (3, 2), (13, 8)):                     # rgba8 (saveJPEG refuses: stb would drop alpha), la8, rgba16
        img = gi.Image()
        assert img.createView(np.zeros((3, 3 * bpp), np.uint8), 3, 3, type_, 3 * bpp)
        assert img.save_to_memory(gi.FORMAT_JPEG) is None
        assert img.isValid and img.errorMessage is None


def _content(rng, kind, h, w, comp):
    if kind == "flat":
        return np.full((h, w, comp), rng.integers(0, 256), np.uint8)
    if kind == "palette":
        pal = rng.integers(0, 256, (4, comp), dtype=np.uint8)
        return pal[rng.integers(0, 4, (h, w))]
    return rng.integers(0, 256, (h, w, comp), dtype=np.uint8)


def test_two_restatements_agree():
    """~300 small random images: every comp, the quality corners, sizes 1..40 (odd, not multiples of 8 or 16), flat / noise /
    palette content -- C and numpy readings byte for byte"""
    rng = np.random.default_rng(20261016)
    qualities = [0, 1, 10, 49, 50, 75, 90, 91, 100]
    for t in range(300):
        h, w = (int(x) for x in rng.integers(1, 41, 2))
        comp = t % 4 + 1
        q = qualities[t % len(qualities)]
        img = _content(rng, ("noise", "flat", "palette")[t % 3], h, w, comp)
        assert JW.encode(img, q) == R.encode(img, q), (t, w, h, comp, q)


def test_c_restatement_pinned_to_the_decoders():
    """streams of the C reading go through the project's host decoder and the oracle decoder; the header tables are Annex K's at the
    right quality; the coefficients read back (de-quantised, natural order) are the numpy reading's quantised values times DQT"""
    L = _capi.lib()
    rng = np.random.default_rng(7)
    base = (rng.integers(0, 256, (37, 45, 3)) // 3 + 60).astype(np.uint8)
    for q, comp in ((50, 3), (75, 1), (90, 4), (95, 3), (100, 2)):
        img = base[:, :, :comp] if comp >= 3 else base[:, :, :1].repeat(comp, 2)
        data = JW.encode(img, q)
        sub, (qy, quv), blks = R.blocks(img, q)
        # header: DQT both tables, SOF0 geometry and sampling, DHT Annex K tables
        assert data[:2] == b"\xFF\xD8" and data[-2:] == b"\xFF\xD9"
        assert data[20:25] == b"\xFF\xDB\x00\x84\x00" and data[25:89] == bytes(int(x) for x in qy)
        assert data[89] == 1 and data[90:154] == bytes(int(x) for x in quv)
        assert data[154:163] == bytes([0xFF, 0xC0, 0, 0x11, 8, 0, 37, 0, 45])
        assert data[165] == (0x22 if q <= 90 else 0x11)
        assert data[173:177] == b"\xFF\xC4\x01\xA2" and data[177] == 0 and data[178:194] == bytes(R.DC_BITS[0])
        assert data[593:607] == b"\xFF\xDA\x00\x0C\x03\x01\x00\x02\x11\x03\x11\x00\x3F\x00"
        buf = np.frombuffer(data, np.uint8)
        fr = _capi.JpegFrame()
        _capi.check(L.gamut_hip_jpeg_decode_coeffs(buf.ctypes.data, buf.size, C.byref(fr)))
        n = fr.mcus_per_row * fr.mcus_per_col * fr.blocks_per_mcu
        assert (fr.width, fr.height, fr.comps, fr.blocks_per_mcu, n) == (45, 37, 3, 6 if sub else 3, len(blks))
        assert (fr.pixel_aspect_ratio, fr.dpi_y) == (1.0, -1.0)                      # JFIF, no units, 1:1
        got = np.ctypeslib.as_array(fr.coeffs, (n, 64)).copy()
        L.gamut_hip_jpeg_frame_free(C.byref(fr))
        exp = np.array([b * (qy if c == 0 else quv) for c, b in blks])[:, R.ZIGZAG]
        assert np.abs(exp).max() < 32768
        assert np.array_equal(got, exp)
        pix, actual, par, dpi = O.decompress_jpeg(data, 3)
        assert pix.shape == (37, 45 * 3) and actual == 3 and (par, dpi) == (1.0, -1.0)


def test_pillow_reads_the_restatement():
    from PIL import Image
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:64, 0:96]
    img = np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], -1).astype(np.uint8)
    img = np.clip(img.astype(int) + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)
    for q in (75, 90, 95):
        im = Image.open(io.BytesIO(JW.encode(img, q)))
        assert im.size == (96, 64) and im.mode == "RGB" and im.info.get("jfif_density") == (1, 1)
        a = np.asarray(im.convert("RGB"), np.float64)
        psnr = 10 * np.log10(255 ** 2 / np.mean((a - img) ** 2))
        assert psnr > 28, (q, psnr)


def test_c99_write_func_consumer(tmp_path):
    """a strict C99 program uses gamut_hip_jpeg_write_func and the three encode entry points"""
    exe = str(tmp_path / "jpeg_write_consumer")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "c", "jpeg_write_consumer.c"), "-o", exe, "-L", lib_dir, "-lgamut_hip",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.startswith("bound=") and "refused=0 calls=0" in out.stdout
