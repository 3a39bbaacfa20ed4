"""SQZ without a GPU: the two restatements of the reference's decoder (tests/c/sqz_ref.c and tests/sqz_ref.py, written separately from the
D text) against each other, the library's host front end against the C restatement coefficient for coefficient, the lossless round trip,
argument checks, the loud no-device failure, identification order, the ABI layout and the golden pins."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sqz_cases
import sqz_ref
import sqz_ref_c as R
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sqz")


@pytest.fixture(scope="module")
def L():
    return _capi.lib()


def host_header(L, f):
    buf = np.zeros(len(f) + 64, np.uint8)                                   # the file at the END of its buffer
    if len(f):
        buf[64:] = np.frombuffer(f, np.uint8)
    info = _capi.SqzInfo()
    rc = L.gamut_hip_sqz_read_header(buf.ctypes.data + 64, len(f), C.byref(info))
    return rc, {k: int(getattr(info, k)) for k in R.INFO_FIELDS}


def host_coeffs(L, f):
    rc, info = host_header(L, f)
    if rc:
        return rc, info, None
    buf = np.zeros(len(f) + 64, np.uint8)
    buf[64:] = np.frombuffer(f, np.uint8)
    n = info["planes"] * info["width"] * info["height"]
    out = np.full(n + 16, 0x5A5A, np.uint16).view(np.int16)
    i2 = _capi.SqzInfo()
    rc = L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data + 64, len(f), out.ctypes.data, n, C.byref(i2))
    assert (out[n:].view(np.uint16) == 0x5A5A).all()                        # nothing behind the capacity
    return rc, info, out[:n]


def test_the_srgb_tables_are_the_reference_tables(L):
    """SHA-256 of SQZ_sRGB_to_linear (little-endian ushorts) and SQZ_linear_to_sRGB as the reference spells them out; both restatements and
    the library generate them from the sRGB transfer functions"""
    s2l, l2s = R.tables()
    assert hashlib.sha256(s2l.astype("<u2").tobytes()).hexdigest() == "fdb7af3c01815a2118db8e50aac3c2304205ccc3f381f8976c588642c1aa60b6"
    assert hashlib.sha256(l2s.tobytes()).hexdigest() == "d256859f24351a0e8f39294df5420e041b15d1b86a95dae6aa6a9fa48dd21905"
    assert sqz_ref.srgb_table() == l2s.tolist()
    t = np.ctypeslib.as_array(C.cast(L.gamut_hip_sqz_linear_to_srgb_table(), C.POINTER(C.c_uint8)), (512,))
    assert np.array_equal(t, l2s)


@pytest.mark.parametrize("order", range(4))
def test_scan_orders_of_the_two_restatements(order):
    """every position once, and the same order, for square, wide, tall, odd and one-tile subbands"""
    for w, h in ((4, 4), (8, 8), (4, 7), (9, 4), (12, 15), (15, 16), (16, 31), (33, 8), (23, 45), (64, 5), (5, 64), (37, 37)):
        c = [tuple(int(v) for v in xy) for xy in R.scan(order, w, h)]
        assert sorted(c) == sorted((x, y) for y in range(h) for x in range(w)), (w, h)
        assert c == list(sqz_ref.SCANS[order](w, h)), (w, h)


def _python_can_afford(f):
    v, info = R.header(f)
    return v != R.OK or info["width"] * info["height"] * info["planes"] <= 6500


def test_the_c_and_python_restatements_agree():
    cases = [(n, f) for n, f, _ in sqz_cases.small_cases() if _python_can_afford(f)]
    grey, oklab = sqz_cases.prefix_files()
    cases += [(f"prefix_grey_{len(f)}", f) for f in sqz_cases.prefixes(grey, 37)] + [(f"prefix_oklab_{len(f)}", f) for f in sqz_cases.prefixes(oklab, 41)]
    assert len(cases) > 90
    for name, f in cases:
        v, info = R.header(f)
        py = sqz_ref.decode(f)
        assert (py is None) == (v != R.OK), name
        if py is None:
            continue
        co, _ = R.coeffs(f)
        assert py[0] == info and py[1] == co.tolist(), name
        assert py[2] == R.pixels(co, info["width"], info["height"], info["color_mode"], info["levels"]).tobytes(), name


def test_python_and_c_pixel_stages_on_extreme_coefficients():
    rng = np.random.default_rng(9)
    for w, h in ((16, 16), (19, 23)):
        for mode in range(4):
            n = (1 if mode == 0 else 3) * w * h
            idx = np.arange(n)
            for co in (np.where(idx & 1, 0xFFFF, 0xFFFE), rng.integers(0, 65536, n) | 0xC000):
                co = co.astype(np.uint16).view(np.int16)
                info = dict(width=w, height=h, levels=1, color_mode=mode, planes=1 if mode == 0 else 3)
                assert sqz_ref.pixels(info, co.tolist()) == R.pixels(co, w, h, mode, 1).tobytes(), (w, h, mode)


def test_the_host_front_end_equals_the_c_restatement(L):
    cases = [(n, f) for n, f, _ in sqz_cases.small_cases()]
    grey, oklab = sqz_cases.prefix_files()
    cases += [(f"prefix_grey_{len(f)}", f) for f in sqz_cases.prefixes(grey)] + [(f"prefix_oklab_{len(f)}", f) for f in sqz_cases.prefixes(oklab)]
    cases += [(f"tiny_{k}", f) for k, f in enumerate(sqz_cases.tiny_files(120))] + [("big", sqz_cases.big_case())]
    accepted = 0
    for name, f in cases:
        v, info = R.header(f)
        rc, hinfo, co = host_coeffs(L, f)
        assert rc == (_capi.OK if v == R.OK else _capi.ERR_DECODE), (name, L.gamut_hip_last_error())
        assert hinfo == info, name
        if v == R.OK:
            assert np.array_equal(co, R.coeffs(f)[0]), name
            accepted += 1
        else:
            assert L.gamut_hip_last_error().startswith(b"sqz: "), name
    assert accepted > 1500


def test_every_prefix_decodes_and_quality_grows():
    """the stream is embedded: every prefix of at least 7 bytes is a file.  (Not every coefficient of a prefix is one of the whole file's: a
    run code cut before its closing 1 bit is taken as closed -- the end of the buffer reads as "not 0" -- and marks an earlier entry.)"""
    for f in sqz_cases.prefix_files():
        assert R.header(f[:6])[0] == R.REFUSED
        whole = R.load(f)[0].astype(np.int32)
        err = []
        for g in sqz_cases.prefixes(f, 5):
            px = R.load(g)
            assert px is not None and px[0].shape == whole.shape
            err.append(float(np.abs(px[0].astype(np.int32) - whole).mean()))
        q = len(err) // 4
        assert np.mean(err[-q:]) < 0.25 * np.mean(err[:q]) and err[0] > 10


@pytest.mark.parametrize("mode", [R.GREY, R.YCOCG])
def test_lossless_round_trip(mode):
    for k, (w, h, lv) in enumerate(((16, 16, 1), (19, 23, 1), (47, 32, 2), (64, 40, 3), (130, 70, 4))):
        px = sqz_cases.picture(w, h, 1 if mode == R.GREY else 3, 50 + k)
        for scan in range(4):
            f = R.encode(px, mode, lv, scan, k & 1)
            got, info = R.load(f)
            assert (info["width"], info["height"], info["levels"], info["scan_order"]) == (w, h, lv, scan)
            assert np.array_equal(got.reshape(px.shape), px), (w, h, scan)


def test_argument_validation_and_no_device_is_a_loud_failure(L):
    assert L.gamut_hip_sqz_read_header(None, 0, None) == _capi.ERR_INVALID_ARG
    f = sqz_cases.small_cases()[-1][1]
    buf = np.frombuffer(f, np.uint8)
    info = _capi.SqzInfo()
    assert L.gamut_hip_sqz_read_header(None, 10, C.byref(info)) == _capi.ERR_DECODE and info.detected == 0
    assert L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, len(f), None, 0, C.byref(info)) == _capi.ERR_INVALID_ARG and info.width == 16      # capacity 0: the sizes
    small = np.full(300, 0x5A5A, np.uint16)
    assert L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, len(f), small.ctypes.data, 255, C.byref(info)) == _capi.ERR_INVALID_ARG and (small == 0x5A5A).all()
    assert L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, len(f), None, 256, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_decode_batch_device(None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_decode_batch_device(None, None, 2, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_decode_batch_device(None, None, 0, None, None, None, None, None) == _capi.OK
    assert L.gamut_hip_sqz_reconstruct_batch_device(None, None, -1, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_reconstruct_batch_device(None, None, 3, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_reconstruct_batch_device(None, None, 0, None, None, None, None) == _capi.OK
    assert L.gamut_hip_sqz_last_decode_stage_ms(7) == -1.0
    if L.gamut_hip_device_count() == 0:                                     # no GPU: a loud failure, outputs untouched
        from gamut_amd import image as gi
        ptrs = (C.c_void_p * 1)(buf.ctypes.data); lens = (C.c_size_t * 1)(len(f)); off = (C.c_int64 * 1)(0)
        out = np.full(512, 0xA5, np.uint8)
        st = (C.c_int * 1)(55)
        hinfo = (_capi.SqzInfo * 1)()
        assert L.gamut_hip_sqz_decode_batch_device(ptrs, lens, 1, off, out.ctypes.data, hinfo, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and hinfo[0].width == 0 and b"no HIP device" in L.gamut_hip_last_error()
        co = np.zeros(256, np.int16)
        d = (_capi.SqzDesc * 1)(); d[0].width = d[0].height = 16; d[0].levels = 1
        assert L.gamut_hip_sqz_reconstruct_batch_device(co.ctypes.data, d, 1, off, out.ctypes.data, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()
        im = gi.Image()
        assert not im.loadFromMemory(f) and not im.isValid and im.errorMessage == "I/O failure while decoding image"


def test_identification_order(L):
    from gamut_amd import image as gi
    gi.lib()

    def ident(b):
        a = np.frombuffer(bytes(b) + b"\0", np.uint8)
        return L.gamut_identify_format_from_memory(a.ctypes.data, len(b))
    tga = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 3, 0, 24, 0x20]) + bytes(36)
    assert ident(tga) == gi.FORMAT_TGA == 5
    a5 = bytes([0xA5]) + tga[1:]                                            # an ID length of 0xA5: a TGA-looking rest behind SQZ's one byte
    assert L.gamut_hip_identify_format(np.frombuffer(a5, np.uint8).ctypes.data, len(a5)) == 5       # the batch surface does not know SQZ
    assert ident(a5) == gi.FORMAT_SQZ == 9
    assert ident(b"\xa5") == 9 and ident(b"") == -1 and ident(b"\xa4" + tga[1:]) == 5
    rest = a5[8:]
    assert ident(b"\xff\xd8" + a5[2:]) == 0 and ident(b"\x89PNG\r\n\x1a\n" + rest) == 1 and ident(b"qoif" + a5[4:]) == 2 and ident(b"qoix" + a5[4:]) == 3
    assert ident(b"GIF89a" + a5[6:]) == 6 and ident(b"GIF87a" + a5[6:]) == 6
    assert ident(b"BM" + a5[2:14] + (40).to_bytes(4, "little") + a5[18:]) == 7
    for name, f, e in sqz_cases.small_cases():
        if len(f) and f[0] == 0xA5:
            assert ident(f) == 9, name                                      # detected, loadable or not
    im = gi.Image()
    assert im.createView(np.zeros((2, 3, 4), np.uint8), 3, 2, 12, 12) and im.save_to_memory(9) is None              # encode is not part of this


def test_sqz_struct_layouts_in_the_d_binding(tmp_path):
    """gamut_hip_sqz_info and gamut_hip_sqz_desc three ways: the C compiler's layout (tests/c/sqz_abi_layout.c), the static asserts in
    bindings/gamut_hip.d and the ctypes mirrors"""
    exe = str(tmp_path / "sqz_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "sqz_abi_layout.c"), "-o", exe])
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(lines) == 2
    for line, mirror in zip(lines, (_capi.SqzInfo, _capi.SqzDesc)):
        f = line.split()
        name, c_size, c_fields = f[0], int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
        m = re.search(r"static assert\((\d+) == %s\.sizeof(.*?)\);" % name, dsrc, flags=re.S)
        assert m and int(m.group(1)) == c_size
        assert {n: int(v) for v, n in re.findall(r"(\d+) == %s\.(\w+)\.offsetof" % name, m.group(2))} == c_fields
        assert C.sizeof(mirror) == c_size and {n: getattr(mirror, n).offset for n, _ in mirror._fields_} == c_fields
    assert list(c_fields) == ["width", "height", "color_mode", "levels", "coeff_offset"]


def test_golden_pins():
    """regression pins of THIS project's restatement (no reference build exists to make them): the files under tests/golden/sqz were written
    by tests/c/sqz_ref.c's encoder, the hashes are of the pixels its decoder gives"""
    pins = json.load(open(os.path.join(GOLDEN, "pins.json")))
    assert len(pins) >= 5
    for name, want in pins.items():
        f = open(os.path.join(GOLDEN, name), "rb").read()
        px, info = R.load(f)
        assert [info["width"], info["height"], info["color_mode"], info["levels"], info["scan_order"], info["subsampling"]] == want["header"], name
        assert hashlib.sha256(px.tobytes()).hexdigest() == want["pixels_sha256"], name
        assert hashlib.sha256(R.coeffs(f)[0].tobytes()).hexdigest() == want["coeffs_sha256"], name
