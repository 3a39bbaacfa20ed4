"""The TGA encoder's oracle and host-side rules, no GPU: the two restatements of TGAEncoder (tests/c/tga_write_ref.c walks a cursor
as the reference does, tests/tga_encode_ref.py reads positions as the kernel does) agree byte for byte; the known packet rows; every
file decodes to its converted source through three decoders; the size bound; refusals, argument validation and the no-device rule."""
import ctypes as C
import io

import numpy as np
import pytest

import tga_encode_cases as cases
import tga_encode_ref as ref
import tga_ref
import tga_ref_c
import tga_write_ref_c
from gamut_amd import _capi


@pytest.fixture(scope="module")
def corpus():
    """(name, image, run-length file, raw file) of every named case and of 300 random images, encoded once by the C restatement"""
    items = cases.matrix_images((511, 512, 513, 1025)) + cases.random_images(300, 1, 399)
    return [(n, im, tga_write_ref_c.encode(im, True), tga_write_ref_c.encode(im, False)) for n, im in items]


def test_the_two_restatements_agree_byte_for_byte(corpus):
    assert len(corpus) > 600
    for name, im, f_rle, f_raw in corpus:
        assert ref.encode(im, True) == f_rle, name
        assert ref.encode(im, False) == f_raw, name


def test_known_answers():
    for name, row, packets in cases.KNOWN_ROWS:
        assert ref.packets(row) == packets, name
        f = tga_write_ref_c.encode(np.asarray(row, np.uint8).reshape(1, -1, 1), True)
        got, p = [], 18
        while p < len(f):
            op = f[p]
            got.append(("R" if op & 0x80 else "raw") + str((op & 127) + 1))
            p += 1 + 3 * (1 if op & 0x80 else (op & 127) + 1)
        assert p == len(f) and got == packets, name


def test_header_bytes():
    for comp, bits in ((1, 24), (2, 32), (3, 24), (4, 32)):
        for rle in (True, False):
            f = tga_write_ref_c.encode(np.zeros((258, 770, comp), np.uint8), rle)
            want = bytearray(18)
            want[2] = 10 if rle else 2
            want[12:16] = bytes([770 & 255, 770 >> 8, 258 & 255, 258 >> 8])
            want[16] = bits
            assert f[:18] == bytes(want)
            if not rle:
                assert len(f) == 18 + 258 * 770 * bits // 8                 # no footer


def test_every_file_decodes_to_the_converted_source(corpus):
    from PIL import Image
    L = _capi.lib()
    for k, (name, im, f_rle, f_raw) in enumerate(corpus):
        want = ref.converted_source(im)
        for f, rle in ((f_rle, 1), (f_raw, 0)):
            got, info = tga_ref_c.load(f)
            assert np.array_equal(got, want) and info["rle"] == rle and info["bottom_up"] == 1, name
            buf = np.frombuffer(f, np.uint8)
            hd = _capi.TgaInfo()
            assert L.gamut_hip_tga_read_header(buf.ctypes.data, buf.size, C.byref(hd)) == _capi.OK and hd.detected == 1, name
            assert (hd.width, hd.height, hd.channels_in_file, hd.rle, hd.data_offset) == (im.shape[1], im.shape[0], want.shape[2], rle, 18), name
            if k % 4 == 0:                                                  # the slow readers on every fourth image
                assert np.array_equal(tga_ref.decode(f)[0], want), name
                pil = Image.open(io.BytesIO(f)); pil.load()
                assert np.array_equal(np.asarray(pil.convert("RGBA" if want.shape[2] == 4 else "RGB")), want), name


def test_one_pixel_raw_packets_and_the_size_bound(corpus):
    L = _capi.lib()
    for name, im, f_rle, _ in corpus:
        h, w, comp = im.shape
        fc = ref.file_channels(comp)
        bound = L.gamut_hip_tga_encode_bound(w, h, comp)
        assert bound == 18 + w * h * (fc + 1) == ref.bound(w, h, comp)
        assert len(f_rle) <= bound and (len(f_rle) == bound) == (w == 1), name
        p, x = 18, 0                                                        # a one-pixel raw packet only at the last pixel of a row
        while p < len(f_rle):
            op = f_rle[p]
            n = (op & 127) + 1
            if op == 0:
                assert x + 1 == w, name
            x = (x + n) % w
            p += 1 + fc * (1 if op & 0x80 else n)


def test_bound_refusals():
    L = _capi.lib()
    for w, h, comp in ((0, 5, 3), (5, 0, 3), (-1, 5, 3), (65536, 5, 3), (5, 65536, 4), (5, 5, 0), (5, 5, 5), (65535, 65535, 3), (65535, 8193, 3), (32768, 16384, 1)):
        assert L.gamut_hip_tga_encode_bound(w, h, comp) == 0 == ref.bound(w, h, comp), (w, h, comp)
    assert L.gamut_hip_tga_encode_bound(65535, 8192, 3) == 18 + 65535 * 8192 * 4 < 2 ** 31      # the largest height at that width
    assert L.gamut_hip_tga_encode_bound(65535, 1, 4) == 18 + 65535 * 5 and L.gamut_hip_tga_encode_bound(1, 65535, 1) == 18 + 65535 * 4
    assert L.gamut_hip_tga_encode_window() % 64 == 0 and L.gamut_hip_tga_encode_window() >= 128


def _batch_args(src, w, h, comp, out):
    a = lambda t, v: (t * 1)(v)
    return dict(src=a(C.c_void_p, src), pitch=a(C.c_int64, w * comp), w=a(C.c_int32, w), h=a(C.c_int32, h), c=a(C.c_int32, comp),
                off=a(C.c_int64, 0), out=out, n=a(C.c_int64, -77), st=a(C.c_int, -77))


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    enc = L.gamut_hip_tga_encode_batch_device
    assert enc(None, None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert enc(None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK
    px = np.arange(4 * 3 * 4, dtype=np.uint8)
    out = np.full(256, 0xA5, np.uint8)
    a = _batch_args(px.ctypes.data, 4, 3, 4, out.ctypes.data)
    full = [a["src"], a["pitch"], a["w"], a["h"], a["c"], None, 1, a["off"], a["out"], a["n"], a["st"], None]
    for missing in (0, 1, 2, 3, 4, 7, 8, 9):                                # every required pointer in turn; rle and status may be NULL
        args = list(full)
        args[missing] = None
        assert enc(*args) == _capi.ERR_INVALID_ARG, missing
        assert b"bad arguments" in L.gamut_hip_last_error()
    assert (out == 0xA5).all() and a["n"][0] == -77 and a["st"][0] == -77
    n = C.c_int(-77)
    for args in ((None, 16, 4, 3, 4, 1), (px.ctypes.data, 16, 0, 3, 4, 1), (px.ctypes.data, 16, 4, 0, 4, 1), (px.ctypes.data, 16, 4, 3, 5, 1),
                 (px.ctypes.data, 16, 65536, 3, 4, 1), (px.ctypes.data, 16, 4, 3, 0, 0)):
        assert not L.gamut_hip_tga_write_to_mem(*args, C.byref(n)) and n.value == -77
        assert b"invalid arguments" in L.gamut_hip_last_error()
    assert not L.gamut_hip_tga_write_to_mem(px.ctypes.data, 16, 4, 3, 4, 1, None)
    assert L.gamut_hip_tga_last_encode_stage_ms(3) == -1.0 and L.gamut_hip_tga_last_encode_stage_ms(-1) == -1.0


def test_every_new_entry_reports_no_device_and_touches_nothing():
    """ERR_NO_DEVICE (NULL from the host drop-in and the Image entries), the message, and every output -- file buffer, per-image
    status, length -- exactly as the caller left it"""
    from gamut_amd import image as gi
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = (np.arange(4 * 3 * 4) % 251).astype(np.uint8)
    px0 = px.copy()
    out = np.full(4096, 0xA5, np.uint8)                                     # stands for the device output: never dereferenced without a device
    a = _batch_args(px.ctypes.data, 4, 3, 4, out.ctypes.data)
    n = C.c_int(-77)
    im = gi.Image()
    assert im.createView(px, 4, 3, 12, 16)
    calls = [("tga_encode_batch_device", lambda: L.gamut_hip_tga_encode_batch_device(a["src"], a["pitch"], a["w"], a["h"], a["c"], None, 1, a["off"], a["out"],
                                                                                     a["n"], a["st"], None), _capi.ERR_NO_DEVICE),
             ("tga_write_to_mem", lambda: L.gamut_hip_tga_write_to_mem(px.ctypes.data, 16, 4, 3, 4, 1, C.byref(n)), None),
             ("tga_write_to_mem raw", lambda: L.gamut_hip_tga_write_to_mem(px.ctypes.data, 16, 4, 3, 4, 0, C.byref(n)), None),
             ("image_save_tga_to_memory", lambda: im.save_tga_to_memory(), None)]
    for name, call, want in calls:
        L.gamut_hip_scanlines_convert_device(-1, out.ctypes.data, 4, 0, 12, out.ctypes.data, 4, 0, 1, 1, 1, None)      # leaves another message behind
        assert b"no HIP device" not in L.gamut_hip_last_error()
        rc = call()
        assert (rc == want) if want is not None else not rc, name
        assert b"no HIP device" in L.gamut_hip_last_error(), name
        assert (out == 0xA5).all() and a["n"][0] == -77 and a["st"][0] == -77 and n.value == -77, name
        assert np.array_equal(px, px0) and im.isValid and im.errorMessage is None, name
    assert L.gamut_hip_tga_last_encode_kernel_ms() == -1.0


def test_image_entries_refuse_other_types_and_errored_images(tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    for t in ("rgb16", "rgbaf32", "l16", "la16", "rgba16", "lf32"):
        im = gi.Image()
        assert im.create(5, 4, O.PT[t])
        assert im.save_tga_to_memory() is None and not im.saveTGAToFile(tmp_path / "x.tga")
        assert im.isValid and im.errorMessage is None and not (tmp_path / "x.tga").exists()
    fresh = gi.Image()                                                      # "Uninitialized image": an error state
    assert fresh.isError and fresh.save_tga_to_memory() is None and not fresh.saveTGAToFile(tmp_path / "y.tga")
    nodata = gi.Image()
    assert nodata.createWithNoData(5, 4, O.PT["rgba8"]) and nodata.save_tga_to_memory() is None
    L = gi.lib()
    n = C.c_size_t(55)
    assert not L.gamut_image_save_tga_to_memory(None, 0, C.byref(n)) and n.value == 0
    ok = gi.Image()
    assert ok.create(5, 4, O.PT["rgba8"])
    assert not L.gamut_image_save_tga_to_memory(ok.h, 0, None) and not L.gamut_image_save_tga_to_file(ok.h, None, 0)
    assert ok.save_to_memory(gi.FORMAT_TGA) is None                         # the generic entry does not dispatch TGA
