"""TGA without a GPU: the two readings of the reference's decoder (tests/c/tga_ref.c, a cursor walk; tests/tga_ref.py, numpy on
positions) against each other and against Pillow; the host header parser gamut_hip_tga_read_header against them, each header rule
one at a time; the identification order; the struct layout; the Image layer's refusal of a truncated file."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np

import tga_cases
import tga_gen
import tga_ref
import tga_ref_c
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DETECT_FIELDS = ("width", "height", "bpp", "indexed", "palette_start", "palette_len", "cmap_size", "detected")


def _win():
    return _capi.lib().gamut_hip_tga_rle_window()


def _lib_header(f):
    L = _capi.lib()
    buf = np.frombuffer(bytes(f) + b"\0", np.uint8)
    info = _capi.TgaInfo()
    rc = L.gamut_hip_tga_read_header(buf.ctypes.data, len(f), C.byref(info))
    if rc != _capi.OK:
        assert rc == _capi.ERR_DECODE and L.gamut_hip_last_error().startswith(b"tga:")
    return bool(info.detected), rc == _capi.OK, {k: int(getattr(info, k)) for k in tga_ref_c.INFO_FIELDS}


def _same_header(f, what):
    """the library, the C restatement and the numpy reading: both verdicts, and the fields as far as each verdict reaches"""
    a, b, c = _lib_header(f), tga_ref_c.header(f), tga_ref.parse(f)
    assert a[:2] == b[:2] == c[:2], (what, a[:2], b[:2], c[:2])
    assert a[2] == b[2], (what, a[2], b[2])
    if a[1]:
        assert c[2] == a[2], (what, c[2], a[2])
    elif a[0]:
        assert {k: a[2][k] for k in DETECT_FIELDS} == {k: c[2][k] for k in DETECT_FIELDS}, what
    return a


def test_the_two_readings_agree_on_every_named_case():
    win = _win()
    assert win >= 1024 and win % 4 == 0
    n = 0
    for name, f in tga_cases.variant_files() + tga_cases.rle_edge_cases(win):
        for req in (0, 3, 4):
            a, b = tga_ref_c.load(f, req), tga_ref.decode(f, req)
            assert a is not None and b is not None, (name, req)
            assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]), (name, req)
            n += 1
        assert _same_header(f, name)[:2] == (True, True)
        assert a[1]["channels_in_file"] == {8: 1, 15: 3, 16: 3, 24: 3, 32: 4}[a[1]["cmap_size"] or a[1]["bpp"]] or (a[1]["image_type"], a[1]["bpp"]) == (3, 16)
    assert n > 700
    for name, f in tga_cases.truncations(win):
        assert tga_ref_c.load(f) is None and tga_ref.decode(f) is None, name
        assert _same_header(f, name)[:2] == (True, True), name             # the header is fine: the stream is what ends early


def test_the_window_case_is_what_it_says():
    win = _win()
    f, marks = tga_cases.window_case(win)
    stream = f[18 + 3:]
    assert marks["windows"] >= 4 and marks["cmd_last"] == win - 1 and marks["cmd_last"] % win == win - 1
    assert marks["straddle"] < 2 * win - 1 < 2 * win < marks["straddle"] + 1 + 128 * 4
    pos, starts = 0, set()                                                 # walk the chain: both marks are packet starts
    while pos < len(stream):
        starts.add(pos); cmd = stream[pos]
        pos += 1 + (1 if cmd & 0x80 else (cmd & 127) + 1) * 4
    assert pos == len(stream) and {marks["cmd_last"], marks["straddle"]} <= starts


def test_read_header_each_rule_and_the_short_lengths():
    for name, f, det in tga_cases.header_refusals():
        a = _same_header(f, name)
        assert a[:2] == (det, False), (name, a[:2])
    good = tga_gen.make(3, 2, 2, 24, seed=1)
    assert [_same_header(good[:n], n)[:2] for n in (0, 16, 17, 18)] == [(False, False), (False, False), (True, False), (True, True)]
    with_id = tga_gen.make(3, 2, 10, 32, id_len=9, seed=1)                 # a skip to exactly the end succeeds, one byte less fails
    assert _same_header(with_id[:27], "id")[:2] == (True, True) and _same_header(with_id[:26], "id")[:2] == (True, False)
    assert _lib_header(with_id[:27])[2]["data_offset"] == 27
    L = _capi.lib()
    assert L.gamut_hip_tga_read_header(None, 0, None) == _capi.ERR_INVALID_ARG
    info = _capi.TgaInfo()
    assert L.gamut_hip_tga_read_header(None, 100, C.byref(info)) == _capi.ERR_DECODE and not info.detected


def test_read_header_on_header_mutations():
    """every byte of the first 18 set to a few values, and every length up to 40, on a file of each variant"""
    rng = np.random.default_rng(5)
    n = n_det = n_ok = 0
    for name, typ, bpp, cmap in tga_gen.variants():
        f = tga_gen.make(5, 3, typ, bpp, cmap, id_len=4, pal_start=2 if cmap else 0, seed=3)
        muts = [f[:k] for k in range(0, 41)]
        for pos in range(18):
            for v in (0, 1, 2, 3, 8, 9, 10, 11, 15, 16, 24, 32, 0x20, 0xff, int(rng.integers(0, 256))):
                muts.append(f[:pos] + bytes([v]) + f[pos + 1:])
        for m in muts:
            a = _same_header(m, (name, m[:18].hex(), len(m)))
            n += 1; n_det += a[0]; n_ok += a[1]
            if a[1] and a[2]["width"] * a[2]["height"] <= 4096:
                ra, rb = tga_ref_c.load(m), tga_ref.decode(m)
                assert (ra is None) == (rb is None) and (ra is None or np.array_equal(ra[0], rb[0])), (name, m[:18].hex())
    assert n > 10000 and n_ok > n // 4 and n - n_det > n // 10, (n, n_det, n_ok)


def test_quirks_kept_from_the_reference():
    r = tga_ref_c.load(tga_gen.make(4, 2, 2, 8, seed=1))
    assert r[1]["channels_in_file"] == 1                                    # bpp 8 is one component even for type 2
    f = tga_gen.make(4, 2, 3, 16, seed=1)
    r = tga_ref_c.load(f)
    assert r[1]["channels_in_file"] == 2 and r[0][::-1].tobytes() == f[18:]  # 16-bit grey: two raw bytes, no swap
    f = tga_gen.header(2, 1, 2, 16, top_down=True) + (0x7C00).to_bytes(2, "little") + (0x001F).to_bytes(2, "little")
    assert tga_ref_c.load(f)[0].tolist() == [[[255, 0, 0], [0, 0, 255]]]    # 5-5-5: red is the high field, no swap afterwards
    f = tga_gen.header(1, 1, 1, 8, 16, pal_len=2, top_down=True) + (0x7C00).to_bytes(2, "little") + (0x03E0).to_bytes(2, "little") + b"\x01"
    assert tga_ref_c.load(f)[0].tolist() == [[[0, 255, 0]]]
    f = tga_gen.header(1, 1, 1, 8, 24, pal_start=3, pal_len=2, top_down=True) + b"xyz" + bytes([1, 2, 3, 4, 5, 6]) + b"\x07"
    assert tga_ref_c.load(f)[0].tolist() == [[[3, 2, 1]]]                   # palette_start counts BYTES; an index past the palette reads entry 0
    f = tga_gen.header(2, 2, 2, 32, desc_extra=0x1F) + bytes(range(16))    # alpha bits and x-origin bit ignored; bottom-up
    assert tga_ref_c.load(f)[0][:, :, 0].tolist() == [[10, 14], [2, 6]]


def test_pillow_reads_the_same_pixels():
    from PIL import Image
    n = 0
    for typ, bpp, cmap, mode in [(2, 24, 0, "RGB"), (10, 24, 0, "RGB"), (2, 32, 0, "RGBA"), (10, 32, 0, "RGBA"), (3, 8, 0, "L"), (11, 8, 0, "L"),
                                 (1, 8, 24, "RGB"), (9, 8, 24, "RGB")]:
        for top_down in (False, True):
            for w, h in ((5, 3), (33, 5), (257, 7)):
                f = tga_gen.make(w, h, typ, bpp, cmap, top_down=top_down, seed=w,
                                 pkts=_row_packets(w, h) if typ >= 8 else None, desc_extra=8 if bpp == 32 else 0)
                im = Image.open(io.BytesIO(f)); im.load()
                ref = tga_ref_c.load(f)
                got = np.asarray(im.convert(mode)).reshape(ref[0].shape)
                assert np.array_equal(got, ref[0]) and np.array_equal(tga_ref.decode(f)[0], ref[0]), (typ, bpp, top_down, w, h)
                n += 1
    assert n == 48


def _row_packets(w, h):
    """packets that end with their row (what the TGA specification asks for and Pillow's decoder assumes)"""
    rng = np.random.default_rng(w * h)
    return [p for _ in range(h) for p in tga_gen.packets("mixed", w, rng)]


def test_files_pillow_writes_decode_to_their_source():
    from PIL import Image
    rng = np.random.default_rng(2)
    for mode, c in (("L", 1), ("RGB", 3), ("RGBA", 4)):
        for w, h in ((1, 1), (5, 3), (130, 9)):
            a = np.repeat(rng.integers(0, 256, (h, (w + 3) // 4, c), dtype=np.uint8), 4, axis=1)[:, :w]       # runs of four
            for comp in ("tga_rle", None):
                bio = io.BytesIO(); Image.fromarray(a.squeeze(-1) if c == 1 else a, mode).save(bio, "TGA", compression=comp)
                f = bio.getvalue()
                for ref in (tga_ref_c.load(f), tga_ref.decode(f)):
                    assert ref is not None and ref[1]["rle"] == (comp is not None) and np.array_equal(ref[0], a), (mode, w, h, comp)
                assert _same_header(f, (mode, w, h, comp))[:2] == (True, True)


def test_identify_order():
    from gamut_amd import image as gi
    L = _capi.lib()
    gi.lib()

    def ident(data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        a = L.gamut_hip_identify_format(buf.ctypes.data, len(data))
        assert a == L.gamut_identify_format_from_memory(buf.ctypes.data, len(data))
        return a
    f = tga_gen.make(3, 2, 2, 24, seed=1)
    assert ident(f) == 5 == gi.FORMAT_TGA and ident(tga_gen.make(3, 2, 9, 8, 24, seed=1)) == 5
    assert ident(f[:17]) == 5 and ident(f[:16]) == -1                      # detectTGA looks at 17 bytes; the load needs more
    for name, m, det in tga_cases.header_refusals():
        assert ident(m) == (5 if det else -1), name
    # a header that is ALSO a valid TGA header keeps its earlier format: 'q' 'o' 'i' 'f' cannot be one (byte 1 > 1), so build the
    # prefixes the other way round -- the signature first, whatever follows
    assert ident(b"qoif" + f[4:]) == 2 and ident(b"BM" + f[2:14] + (40).to_bytes(4, "little") + f[18:]) == 7
    assert ident(b"\xff\xd8" + f[2:]) == 0 and ident(b"\x89PNG\r\n\x1a\n" + f[8:]) == 1
    gif = np.frombuffer(b"GIF89a" + f[6:] + b"\0", np.uint8)                # (GIF is known to the Image layer's entry alone)
    assert L.gamut_identify_format_from_memory(gif.ctypes.data, len(f)) == 6 and L.gamut_hip_identify_format(gif.ctypes.data, len(f)) == -1
    bm_tga = b"B\x01\x01" + f[3:]                                          # 'B' then a TGA-looking rest: not BMP, and byte 2 = 1 needs a colour map
    assert ident(bm_tga) == -1
    assert L.gamut_hip_identify_format(None, 100) == -1
    im = gi.Image()
    assert im.createView(np.zeros((2, 3, 4), np.uint8), 3, 2, 12, 12) and im.save_to_memory(5) is None          # encode is not part of this


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    assert L.gamut_hip_tga_decode_batch_device(None, None, -1, 0, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_tga_decode_batch_device(None, None, 2, 0, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_tga_decode_batch_device(None, None, 0, 0, None, None, None, None, None) == _capi.OK
    f = np.frombuffer(tga_gen.make(3, 2, 2, 24), np.uint8)
    ptrs = (C.c_void_p * 1)(f.ctypes.data); lens = (C.c_size_t * 1)(f.size); off = (C.c_int64 * 1)(0)
    out = np.full(64, 0xA5, np.uint8)
    for req in (1, 2, 5, -1):
        assert L.gamut_hip_tga_decode_batch_device(ptrs, lens, 1, req, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    if L.gamut_hip_device_count() == 0:                                    # no GPU: a loud failure, outputs untouched
        st = (C.c_int * 1)(55)
        assert L.gamut_hip_tga_decode_batch_device(ptrs, lens, 1, 4, off, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()


def test_host_image_refuses_a_truncated_rle_file():
    from gamut_amd import image as gi
    name, f = tga_cases.truncations(_win())[0]
    assert name == "rle_cut_at_command_byte"
    im = gi.Image()
    assert not im.loadFromMemory(f) and not im.isValid
    assert im.errorMessage == "Image decoding failed"                      # kStrImageDecodingFailed
    im2 = gi.Image()
    assert not im2.loadFromMemory(f[:17]) and im2.errorMessage == im.errorMessage                 # detected, not loadable: the same message
    im3 = gi.Image()
    assert not im3.loadFromMemory(f[:16]) and im3.errorMessage == "Unidentified image format"     # not even detected


def test_tga_info_layout_in_the_d_binding(tmp_path):
    """gamut_hip_tga_info four ways: the C compiler's layout (tests/c/tga_abi_layout.c), the static assert in bindings/gamut_hip.d, the
    layout the D declaration yields, and the ctypes mirror."""
    exe = str(tmp_path / "tga_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "tga_abi_layout.c"), "-o", exe])
    f = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert f[0] == "gamut_hip_tga_info"
    c_size, c_fields = int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    assert list(c_fields) == list(tga_ref_c.INFO_FIELDS)
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    m = re.search(r"static assert\((\d+) == gamut_hip_tga_info\.sizeof(.*?)\);", dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n: int(v) for v, n in re.findall(r"(\d+) == gamut_hip_tga_info\.(\w+)\.offsetof", m.group(2))} == c_fields
    decl = re.search(r"struct gamut_hip_tga_info\s*\{(.*?)\}", dsrc, flags=re.S).group(1)
    off, fields = 0, {}
    for part in [x.strip() for x in decl.split(";") if x.strip()]:
        typ, names = part.split(None, 1)
        assert typ == "int"
        for n in names.split(","):
            fields[n.strip()] = off; off += 4
    assert (off, fields) == (c_size, c_fields)
    assert C.sizeof(_capi.TgaInfo) == c_size and {n: getattr(_capi.TgaInfo, n).offset for n, _ in _capi.TgaInfo._fields_} == c_fields
