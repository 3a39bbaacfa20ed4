"""QOIX encode without a device.  The serial C restatement (tests/c/qoix_write_ref.c), which is the oracle of the GPU tests, is checked
against things that are not itself: both existing decoders, the LZ4 inflater, op streams derived by hand; then the bound and its
refusals, the loud failure when there is no GPU, the Image mirror's refusals, the boundary cases of the container choice and the
coverage of the GPU suite's images, and the struct layout."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import qoix_encode_cases as cases
import qoix_gen
import qoix_ref
import qoix_ref_c
import qoix_write_ref_c as ref
from gamut_amd import _capi
from gamut_amd import image as gi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def suite_images():
    return cases.matrix_images((1, 2, 3, 63, 64, 65)) + cases.run_images() + cases.op_images() + [(n, im) for n, im, _ in cases.boundary_images()]


def test_every_case_file_decodes_to_its_source_through_both_decoders():
    big = cases.content("noise", 160, 140, 3, 5)
    packed = 0
    for name, im in suite_images() + [("noise 160x140", big), ("flat 160x140", qoix_gen.flat_image(160, 140, 3, 4))]:
        for mode in (0, 1):
            f = ref.encode(im, mode, par=1.5, dpi=300.0)
            assert f[:4] == b"qoix" and f[16] in ((0, 1) if mode == 0 else (0,)) and f[17:25] == struct.pack(">ff", 1.5, 300.0), name
            packed += f[16]
            got = qoix_ref_c.load(f)
            assert got is not None and np.array_equal(got[0], im), name
            if im.shape[0] * im.shape[1] <= 4096:                           # (the Python reading is slow)
                got = qoix_ref.decode(f)
                assert got is not None and np.array_equal(got[0], im), name
    assert packed >= 20                                                     # the LZ4 path of both decoders was taken


def test_every_lz4_block_inflates_to_its_input_and_is_consumed_whole():
    for name, s in cases.lz4_strings() + [(f"mixed {k}", s) for k, s in enumerate(cases.lz4_mixed(100))]:
        block = ref.lz4_compress(s)
        assert len(block) <= ref.lz4_bound(len(s)) == len(s) + len(s) // 255 + 16, name
        if len(s) == 0:
            assert block == b"\x00"
            continue
        assert qoix_ref.lz4_block(block, len(s)) == s, name
        with pytest.raises(qoix_ref.Refused):                               # not a byte too many: a shorter block cannot give the string
            qoix_ref.lz4_block(block[:-1], len(s))
    # the distance test of byU32: 65535 back is taken, 65536 is not
    sizes = {n: len(ref.lz4_compress(s)) for n, s in cases.lz4_strings() if n.startswith("recurs")}
    assert sizes["recurs 65535 later"] < 140000 < sizes["recurs 65536 later"] == sizes["recurs 70000 later"]


def test_known_streams():
    for name, im, stream in cases.KNOWN_STREAMS:
        for mode in (0, 1):
            f = ref.encode(im, mode)
            assert f[16] == 0 and f[25:].hex() == stream, name              # an LZ4 block of so few bytes is a byte longer: stored
            assert f[:25] == qoix_gen.header(im.shape[1], im.shape[0], im.shape[2]), name


def desc(w, h, ch=3, cs=0, mode=0):
    return _capi.QoixDesc(w, h, ch, cs, mode, 1.0, 96.0)


def formula(w, h, ch):
    datalen_max = w * h * (ch + 1) + 4
    return 29 + datalen_max + datalen_max // 255 + 16


def test_encode_bound_and_refusals():
    L = _capi.lib()
    b = lambda *a: L.gamut_hip_qoix_encode_bound(C.byref(desc(*a)))
    for w, h, ch in ((1, 1, 3), (3, 7, 4), (1920, 1080, 4), (1920, 1080, 3), (65, 2, 3)):
        assert b(w, h, ch) == formula(w, h, ch) == ref.bound(w, h, ch)
    assert b(7, 3, 4, 2) == formula(7, 3, 4) and b(7, 3, 4, 1, 1) == formula(7, 3, 4)
    assert b(0, 5) == -1 and b(5, 0) == -1 and b(-1, 5) == -1 and b(5, -1) == -1
    assert b(5, 5, 2) == -1 and b(5, 5, 5) == -1 and b(5, 5, 1) == -1
    assert b(5, 5, 4, 3) == -1 and b(5, 5, 4, -1) == -1
    assert b(5, 5, 4, 0, 2) == -1                                           # a mode that does not exist
    w = 20000                                                               # height >= 400000000 / width
    assert b(w, 400000000 // w, 3) == -1 and ref.bound(w, 400000000 // w, 3) == -1
    assert b(w, 400000000 // w - 1, 3) == formula(w, 400000000 // w - 1, 3)
    assert b(7, 57142857, 3) == -1 and b(7, 57142856, 3) == formula(7, 57142856, 3)
    assert formula(1, 399999999, 4) < 2 ** 31 - 1 and b(1, 399999999, 4) == formula(1, 399999999, 4)
    assert b(20000, 19999, 4) == formula(20000, 19999, 4) < 2 ** 31                # the largest accepted shapes stay below 2^31 - 1 (deviation 2 is a guard)
    assert L.gamut_hip_qoix_encode_bound(None) == -1
    assert L.gamut_hip_lz4_compress_bound(0) == 16 and L.gamut_hip_lz4_compress_bound(255) == 272 and L.gamut_hip_lz4_compress_bound(-1) == 0
    assert L.gamut_hip_lz4_compress_bound(0x7E000000) == 0x7E000000 + 0x7E000000 // 255 + 16 and L.gamut_hip_lz4_compress_bound(0x7E000001) == 0
    assert L.gamut_hip_qoix_encode_window() == 64


def test_argument_validation_without_device():
    L = _capi.lib()
    assert L.gamut_hip_qoix_encode_batch_device(None, None, None, 0, None, None, None, None, None) == _capi.OK
    assert L.gamut_hip_qoix_encode_batch_device(None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_qoix_encode_batch_device(None, None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert b"bad arguments" in L.gamut_hip_last_error()
    assert L.gamut_hip_lz4_compress_batch_device(None, None, 0, None, None, None, None, None) == _capi.OK
    assert L.gamut_hip_lz4_compress_batch_device(None, None, 2, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoix_write_to_mem(None, 12, C.byref(desc(4, 4)), C.byref(n))
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 12, None, C.byref(n))
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 12, C.byref(desc(4, 4)), None)
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 8, C.byref(desc(4, 4, 2)), C.byref(n))
    assert b"invalid arguments" in L.gamut_hip_last_error() and n.value == -1
    assert L.gamut_hip_qoix_last_encode_stage_ms(7) == -1.0


def test_no_device_is_a_loud_failure():
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 12, C.byref(desc(4, 4)), C.byref(n)) and n.value == -1
    d = (_capi.QoixDesc * 1)(desc(4, 4))
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(12); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1)
    out = np.full(256, 0xA5, np.uint8); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_qoix_encode_batch_device(src, pitch, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert (out == 0xA5).all() and ln[0] == -1 and st[0] == -7
    slen = (C.c_int32 * 1)(20)
    assert L.gamut_hip_lz4_compress_batch_device(src, slen, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert (out == 0xA5).all()
    img = gi.Image()
    assert img.createView(np.zeros((4, 16), np.uint8), 4, 4, 12, 16)        # rgba8
    assert img.save_qoix_to_memory() is None
    assert img.isValid and img.errorMessage is None


def test_image_save_refusals(tmp_path):
    img = gi.Image()
    assert img.save_qoix_to_memory() is None                                # errored ("Uninitialized image")
    assert img.errorMessage == "Uninitialized image"
    nodata = gi.Image()
    assert nodata.createWithNoData(4, 3, 12) and nodata.save_qoix_to_memory() is None and nodata.isValid
    for type_, bytes_per_px in ((0, 1), (3, 2), (13, 8), (14, 16), (6, 2), (10, 6)):       # l8, la8, rgba16, rgbaf32, lap8, rgb16
        v = gi.Image()
        assert v.createView(np.zeros((3, 4 * bytes_per_px), np.uint8), 4, 3, type_, 4 * bytes_per_px)
        assert v.save_qoix_to_memory() is None and v.saveQOIXToMemory(5) is None
        assert not v.saveQOIXToFile(tmp_path / "no.qoix") and not (tmp_path / "no.qoix").exists()
        assert v.isValid and v.type == type_ and v.width == 4 and v.errorMessage is None        # no side effect on the image
    rgba = gi.Image()
    assert rgba.createView(np.zeros((3, 16), np.uint8), 4, 3, 12, 16)
    assert rgba.save_to_memory(gi.FORMAT_QOIX) is None and gi.FORMAT_QOIX == 3
    L = gi.lib()
    n = C.c_size_t(5)
    assert not L.gamut_image_save_qoix_to_memory(None, 0, C.byref(n)) and n.value == 0
    assert not L.gamut_image_save_qoix_to_memory(rgba.h, 0, None)
    assert not L.gamut_image_save_qoix_to_file(rgba.h, None, 0)
    assert not L.gamut_image_save_to_file(rgba.h, gi.FORMAT_QOIX, str(tmp_path / "x.qoix").encode(), 0)


def test_boundary_cases_are_boundary_cases():
    """lz4Size + 4 - datalen of the committed seeds: -1 packs, 0 and +1 do not"""
    items = cases.boundary_images()
    assert {d for _, _, d in items} >= {-1, 0, 1}
    for name, im, diff in items:
        f, got = ref.encode_ex(im, 0)
        assert got == diff, name
        assert f[16] == (1 if diff < 0 else 0), name
        stored = ref.encode(im, 1)
        assert (len(f) == len(stored) + diff) if diff < 0 else (f == stored), name
    big = ref.encode(cases.content("noise", 160, 140, 3, 5), 1)
    assert len(big) - 25 >= 65547                                           # the GPU suite's byU32 op stream


def test_the_suite_holds_every_op_kind():
    kinds, after_adiff = set(), set()
    for name, im in suite_images():
        ks = cases.parse_ops(ref.encode(im, 1)[25:-4])
        kinds |= set(ks)
        after_adiff |= {b for a, b in zip(ks, ks[1:]) if a == "ADIFF"}
    assert kinds == {"LUMA", "INDEX", "LUMA2", "LUMA3", "ADIFF", "RUN", "RUN2", "GRAY", "RGB", "RGBA"}
    assert after_adiff == {"LUMA", "GRAY", "LUMA2", "LUMA3", "RGB"}          # ADIFF is followed by a colour op, never by anything else
    h1, h2 = cases.equal_hash_pair()
    assert h1 != h2 and cases.color_hash(h1) == cases.color_hash(h2)
    # the recurrence cases: 63 misses later the colour is still indexed, 64 and 65 later it is not
    for gap, hit in ((63, True), (64, False), (65, False)):
        im = dict(cases.op_images())[f"recurs after {gap} misses x3"]
        ks = cases.parse_ops(ref.encode(im, 1)[25:-4])
        assert (ks[gap + 1] == "INDEX") == hit, (gap, ks[gap + 1])
    z = dict(cases.op_images())["zero pixel first and after 64 misses"]
    ks = cases.parse_ops(ref.encode(z, 1)[25:-4])
    assert ref.encode(z, 1)[25] == 0x80 and ks[65] != "INDEX"


def test_qoix_desc_layout_in_the_d_binding(tmp_path):
    """gamut_hip_qoix_desc four ways: the C compiler's layout (tests/c/qoix_encode_abi_layout.c), the static assert in bindings/gamut_hip.d,
    the layout the D declaration yields, and the ctypes mirror"""
    exe = str(tmp_path / "qoix_encode_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "c", "qoix_encode_abi_layout.c"), "-o", exe])
    f = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert f[0] == "gamut_hip_qoix_desc"
    c_size, c_fields = int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    assert list(c_fields) == ["width", "height", "channels", "colorspace", "mode", "pixel_aspect_ratio", "resolution_y"] and c_size == 28
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    m = re.search(r"static assert\((\d+) == gamut_hip_qoix_desc\.sizeof(.*?)\);", dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n: int(v) for v, n in re.findall(r"(\d+) == gamut_hip_qoix_desc\.(\w+)\.offsetof", m.group(2))} == c_fields
    decl = re.search(r"struct gamut_hip_qoix_desc\s*\{(.*?)\}", dsrc, flags=re.S).group(1)
    off, fields = 0, {}
    for part in [x.strip() for x in decl.split(";") if x.strip()]:
        typ, names = part.split(None, 1)
        assert typ in ("int", "float")
        for n in names.split(","):
            fields[n.strip()] = off; off += 4
    assert (off, fields) == (c_size, c_fields)
    assert C.sizeof(_capi.QoixDesc) == c_size and {n: getattr(_capi.QoixDesc, n).offset for n, _ in _capi.QoixDesc._fields_} == c_fields
    assert [t for _, t in _capi.QoixDesc._fields_][5:] == [C.c_float, C.c_float]
