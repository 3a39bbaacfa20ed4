"""BMP without a GPU: the two readings of the reference's loader (tests/c/bmp_ref.c, a cursor walk; tests/bmp_ref.py, numpy on
positions) against each other and against Pillow where Pillow performs the same transformation; the host header parser
gamut_hip_bmp_read_header against them; detectBMP; the encoder's bound and the argument checks of the batch calls; the Image layer's
refusals."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest

import bmp_gen
import bmp_ref
import bmp_ref_c
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _random_files(n=320, seed=7):
    rng = np.random.default_rng(seed)
    return [bmp_gen.random_file(rng) for _ in range(n)]


FILES = _random_files()
VARIANTS = bmp_gen.variants(13, 3, seed=1) + bmp_gen.variants(5, 2, seed=2)


def _mutations(f, rng, values=(0, 1, 3, 0x80, 0xff)):
    """header mutations: every byte of the first 70 set to a few values; truncation at every length up to the pixel offset + 8"""
    out = []
    for pos in range(min(70, len(f))):
        for v in values + (int(rng.integers(0, 256)),):
            if f[pos] != v:
                out.append(f[:pos] + bytes([v]) + f[pos + 1:])
    off = int.from_bytes(f[10:14], "little")
    for n in range(0, min(len(f), off + 8) + 1):
        out.append(f[:n])
    return out


_BASES = FILES + [v for _, v in VARIANTS[::3]]


def _same(a, b, what):
    assert (a is None) == (b is None), (what, "verdicts differ", a is None, b is None)
    if a is None:
        return
    assert a[1] == b[1], (what, a[1], b[1])
    assert np.array_equal(np.float32(a[2]), np.float32(b[2])), (what, a[2], b[2])
    assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]), what


def test_the_two_readings_agree_on_generated_files():
    n_ok = 0
    for k, f in enumerate(FILES + [v for _, v in VARIANTS]):
        for req in range(5):
            a, b = bmp_ref_c.load(f, req), bmp_ref.decode(f, req)
            _same(a, b, (k, req))
            n_ok += a is not None
    assert n_ok > 5 * 250, n_ok


def test_the_two_readings_agree_on_header_mutations():
    rng = np.random.default_rng(11)
    n = n_ok = n_bad = 0
    for k, f in enumerate(_BASES):
        for m in _mutations(f, rng, (0, 1, 3, 0x80, 0xff) if k < 40 else (0, 0xff)):      # each of the generated files; the full value set on the first 40
            hc, hn = bmp_ref_c.header(m), bmp_ref.parse(m)
            assert (hc is None) == (hn is None), (k, m[:70].hex())
            n += 1
            if hc is None:
                n_bad += 1
                continue
            assert hc[0] == hn[0] and np.array_equal(np.float32(hc[1]), np.float32(hn[1])), (k, m[:70].hex(), hc, hn[:2])
            n_ok += 1
            if hc[0]["width"] * hc[0]["height"] <= 4096:                   # pixels too, on every fourth request, where the picture stayed small
                req = n % 5
                _same(bmp_ref_c.load(m, req), bmp_ref.decode(m, req), (k, req, m[:70].hex()))
    assert n > 80000 and n_ok > n // 4 and n_bad > n // 10, (n, n_ok, n_bad)


def test_pillow_agrees_where_it_performs_the_same_transformation():
    from PIL import Image
    n = 0
    for name, f in bmp_gen.variants(13, 3, seed=3):
        m = re.match(r"h(\d+)_(p\d+|24|32_rgb)", name)
        if not m or "gap" in name or "short" in name or (m.group(1) == "12" and m.group(2).startswith("p")):
            continue                # (16-bit expansion and alpha are Pillow's own; gaps: see bmp_host.hip; the reference takes the palette of
            #                          a 12-byte header to be 4 entries shorter than it is, :2289)
        ref = bmp_ref_c.load(f, 3)
        assert ref is not None, name
        if m.group(1) == "56":
            continue                                                       # (the one header size of the generator that Pillow's BmpImagePlugin does not read)
        im = Image.open(io.BytesIO(f)); im.load()
        got = np.asarray(im.convert("RGB") if im.mode in ("P", "1", "L", "RGB") else im.convert("RGBA"))[..., :3]
        assert np.array_equal(got, ref[0]), name
        n += 1
    assert n >= 12, n


def test_pillow_reads_the_encoder_references_output():
    from PIL import Image
    rng = np.random.default_rng(5)
    for w, h, c in [(1, 1, 3), (5, 3, 3), (7, 2, 4), (33, 5, 3), (64, 2, 4)]:
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        f = bmp_ref_c.write(img, 3780, 3780)
        assert len(f) == bmp_ref_c.bound(w, h, c)
        im = Image.open(io.BytesIO(f)); im.load()
        assert im.size == (w, h)
        got = np.asarray(im.convert("RGBA" if c == 4 else "RGB"))
        assert np.array_equal(got, img), (w, h, c, im.mode)                # rgba: the mask-based file round-trips
        back = bmp_ref_c.load(f, 0)                                        # ... and the loader's reference reads it back
        assert back is not None and np.array_equal(back[0], img) and back[1]["channels_in_file"] == c
        assert back[2] == (3780.0, 3780.0, 1.0)
    assert bmp_ref_c.write(np.zeros((2, 2, 3), np.uint8)) is not None and bmp_ref_c.bound(2, 2, 2) == 0


def _lib_header(f):
    L = _capi.lib()
    buf = np.frombuffer(bytes(f) + b"\0", np.uint8)
    info = _capi.BmpInfo()
    rc = L.gamut_hip_bmp_read_header(buf.ctypes.data, len(f), C.byref(info))
    if rc != _capi.OK:
        assert rc == _capi.ERR_DECODE and L.gamut_hip_last_error().startswith(b"bmp:")
        return None
    return ({k: int(getattr(info, k)) & 0xffffffff for k in bmp_ref_c.INFO_FIELDS},
            (info.pixels_per_meter_x, info.pixels_per_meter_y, info.pixel_aspect_ratio))


def test_read_header_matches_the_c_reference():
    rng = np.random.default_rng(12)
    files = FILES + [v for _, v in VARIANTS]
    for k, f in enumerate(_BASES):
        files += _mutations(f, rng, (0, 1, 3, 0x80, 0xff) if k < 40 else (0, 0xff))
    n_ok = 0
    for f in files:
        a, b = _lib_header(f), bmp_ref_c.header(f)
        assert (a is None) == (b is None), f[:70].hex()
        if a is None:
            continue
        assert a[0] == b[0], (f[:70].hex(), a[0], b[0])
        assert np.array_equal(np.float32(a[1]), np.float32(b[1])), (a[1], b[1])          # unknown is -1, never NaN
        n_ok += 1
    assert n_ok > 20000, n_ok
    L = _capi.lib()
    assert L.gamut_hip_bmp_read_header(None, 0, None) == _capi.ERR_INVALID_ARG
    info = _capi.BmpInfo()
    assert L.gamut_hip_bmp_read_header(None, 100, C.byref(info)) == _capi.ERR_DECODE


def test_identify_format_bmp():
    from gamut_amd import image as gi
    L = _capi.lib()
    gi.lib()

    def ident(data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        a = L.gamut_hip_identify_format(buf.ctypes.data, len(data))
        assert a == L.gamut_identify_format_from_memory(buf.ctypes.data, len(data))
        return a
    f40 = bmp_gen.make(3, 2, 24, 40)
    assert ident(f40) == 7 and ident(bmp_gen.make(3, 2, 8, 12)) == 7
    f52 = f40[:14] + (52).to_bytes(4, "little") + f40[18:]
    assert ident(f52) == 7 and _lib_header(f52) is None and bmp_ref_c.header(f52) is None     # detectBMP says yes, the loader refuses
    assert ident(f40[:14] + (41).to_bytes(4, "little") + f40[18:]) == -1
    assert ident(f40[:17]) == -1 and ident(f40[:18]) == 7
    assert L.gamut_hip_identify_format(None, 100) == -1
    assert ident(b"\xff\xd8BM" + f40[4:]) == 0                             # the three earlier signatures are tested first


def test_encode_bound():
    L = _capi.lib()
    for w, h, c in [(1, 1, 3), (1, 1, 4), (5, 3, 3), (7, 2, 4), (32767, 32767, 4), (1920, 1080, 3)]:
        assert L.gamut_hip_bmp_encode_bound(w, h, c) == 122 + h * ((w * c + 3) & ~3) == bmp_ref_c.bound(w, h, c)
    for w, h, c in [(4, 4, 1), (4, 4, 2), (4, 4, 5), (0, 4, 3), (4, 0, 3), (32768, 4, 3), (4, 32768, 4), (-1, 4, 3)]:
        assert L.gamut_hip_bmp_encode_bound(w, h, c) == 0 == bmp_ref_c.bound(w, h, c)


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    assert L.gamut_hip_bmp_decode_batch_device(None, None, -1, 0, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_decode_batch_device(None, None, 2, 0, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_decode_batch_device(None, None, 0, 0, None, None, None, None, None) == _capi.OK
    f = np.frombuffer(bmp_gen.make(3, 2, 24), np.uint8)
    ptrs = (C.c_void_p * 1)(f.ctypes.data); lens = (C.c_size_t * 1)(f.size); off = (C.c_int64 * 1)(0)
    out = np.full(64, 0xA5, np.uint8)
    assert L.gamut_hip_bmp_decode_batch_device(ptrs, lens, 1, 5, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_decode_batch_device(ptrs, lens, 1, -1, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_encode_batch_device(None, None, None, None, None, None, None, 3, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_encode_batch_device(None, None, None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_bmp_encode_batch_device(None, None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK
    n = C.c_int(77)
    px = np.zeros(48, np.uint8)
    assert not L.gamut_hip_bmp_write_to_mem(None, 12, 4, 4, 3, 0, 0, C.byref(n)) and n.value == 77
    assert not L.gamut_hip_bmp_write_to_mem(px.ctypes.data, 12, 4, 4, 2, 0, 0, C.byref(n)) and n.value == 77
    assert not L.gamut_hip_bmp_write_to_mem(px.ctypes.data, 12, 4, 4, 3, 0, 0, None)
    if L.gamut_hip_device_count() == 0:                                    # no GPU: a loud failure, outputs untouched
        st = (C.c_int * 1)(55)
        assert L.gamut_hip_bmp_decode_batch_device(ptrs, lens, 1, 4, off, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()
        w = (C.c_int32 * 1)(4); c3 = (C.c_int32 * 1)(3); pitch = (C.c_int64 * 1)(12); olen = (C.c_int64 * 1)(99)
        src = (C.c_void_p * 1)(px.ctypes.data)
        assert L.gamut_hip_bmp_encode_batch_device(src, pitch, w, w, c3, None, None, 1, off, out.ctypes.data, olen, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and olen[0] == 99 and st[0] == 55
        assert not L.gamut_hip_bmp_write_to_mem(px.ctypes.data, 12, 4, 4, 3, 0, 0, C.byref(n)) and n.value == 77


def _all_a_files(w, h):
    """32-bit files for the all_a rule (stbdec.d:2137, 2418, 2439-2443): (name, file, expected alpha of decode(req 4))"""
    rng = np.random.default_rng(w * 31 + h)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    zero = px.copy(); zero[..., 3] = 0
    one = zero.copy(); one[h - 1, w - 1, 3] = 9
    easy = (0x00ff0000, 0x0000ff00, 0x000000ff, 0xff000000)
    return [("rgb_all_zero", bmp_gen.make(w, h, 32, 40, body=zero.tobytes()), np.full((h, w), 255, np.uint8)),
            ("rgb_one_set", bmp_gen.make(w, h, 32, 40, body=one.tobytes()), one[::-1, :, 3]),
            ("bitfields_all_zero", bmp_gen.make(w, h, 32, 108, 3, easy, body=zero.tobytes()), np.zeros((h, w), np.uint8)),
            ("v5_rgb_all_zero", bmp_gen.make(w, h, 32, 124, body=zero.tobytes(), top_down=True), np.full((h, w), 255, np.uint8))]


def test_all_a_rule_in_both_references():
    for name, f, alpha in _all_a_files(3, 2):
        for load in (bmp_ref_c.load, bmp_ref.decode):
            r4, r2, r3, r0 = load(f, 4), load(f, 2), load(f, 3), load(f, 0)
            assert np.array_equal(r4[0][..., 3], alpha), name
            assert np.array_equal(r2[0][..., 1], alpha), name                # req_comp 2 decodes to 4 channels first: the rule reaches the la8 alpha
            assert r3[0].shape[2] == 3 and np.array_equal(r3[0], r4[0][..., :3]), name
            assert r0[1]["channels_in_file"] == 4 and np.array_equal(r0[0], r4[0]), name


def test_image_save_bmp_refusals(tmp_path):
    from gamut_amd import image as gi
    a = np.zeros((2, 3, 4 * 8), np.uint8)
    l8, rgba16, layered, blank = gi.Image(), gi.Image(), gi.Image(), gi.Image()
    assert l8.createView(a, 4, 3, 0, 4) and rgba16.createView(a, 4, 3, 13, 32) and layered.createLayeredView(a, 4, 3, 2, 12, 16, 3 * 32)
    path = tmp_path / "never_written.bmp"
    for im, typ in ((l8, 0), (rgba16, 13), (layered, 12), (blank, -1)):
        before = (im.type, im.width, im.height, im.layers, im.isValid, im.errorMessage)
        assert before[0] == typ
        assert im.save_bmp_to_memory() is None and not im.saveBMPToFile(path) and not path.exists()
        assert (im.type, im.width, im.height, im.layers, im.isValid, im.errorMessage) == before      # no side effect on the image
    L = gi.lib()
    n = C.c_size_t(5)
    assert not L.gamut_image_save_bmp_to_memory(l8.h, 0, C.byref(n)) and n.value == 0
    rgba8 = gi.Image()
    assert rgba8.createView(a, 4, 3, 12, 16)
    assert not L.gamut_image_save_bmp_to_file(rgba8.h, None, 0)
    assert rgba8.save_to_memory(gi.FORMAT_BMP) is None and gi.FORMAT_BMP == 7                        # the generic entries do not dispatch BMP


def test_bmp_info_layout_in_the_d_binding(tmp_path):
    """gamut_hip_bmp_info three ways, as test_capi_cpu.py does for the earlier structs: the C compiler's layout (tests/c/bmp_abi_layout.c), the
    static assert in bindings/gamut_hip.d, the layout the D declaration yields, and the ctypes mirror."""
    exe = str(tmp_path / "bmp_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "bmp_abi_layout.c"), "-o", exe])
    f = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert f[0] == "gamut_hip_bmp_info"
    c_size, c_fields = int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    m = re.search(r"static assert\((\d+) == gamut_hip_bmp_info\.sizeof(.*?)\);", dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n: int(v) for v, n in re.findall(r"(\d+) == gamut_hip_bmp_info\.(\w+)\.offsetof", m.group(2))} == c_fields
    decl = re.search(r"struct gamut_hip_bmp_info\s*\{(.*?)\}", dsrc, flags=re.S).group(1)
    off, fields = 0, {}
    for part in [x.strip() for x in decl.split(";") if x.strip()]:
        typ, names = part.split(None, 1)
        assert typ in ("int", "uint", "float")
        for n in names.split(","):
            fields[n.strip()] = off; off += 4
    assert (off, fields) == (c_size, c_fields)
    assert C.sizeof(_capi.BmpInfo) == c_size and {n: getattr(_capi.BmpInfo, n).offset for n, _ in _capi.BmpInfo._fields_} == c_fields
