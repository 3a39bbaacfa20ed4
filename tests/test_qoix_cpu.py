"""QOIX without a GPU.  No file written by the reference exists (it ships none and cannot be built here), so the pin is two independent
readings of its text -- tests/c/qoix_ref.c, serial C with the reference's two scanline buffers, and tests/qoix_ref.py, Python on a whole-image
array -- held against each other on every named case, on random op streams and on mutated files, plus round trips of generator-written
images.  Then the library's host side against them: gamut_hip_qoix_read_header, the identification, the struct layout, the Image layer's
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import qoix_cases
import qoix_gen as G
import qoix_ref
import qoix_ref_c
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VERDICT = {"ok": qoix_ref_c.OK, "refused": qoix_ref_c.REFUSED, "unsupported": qoix_ref_c.UNSUPPORTED}


def _cap():
    return _capi.lib().gamut_hip_qoix_row_capacity()


def _agree(name, f, channels=(0, 3, 4)):
    """both readings on one file: header verdict, info, and per channel count the load verdict and the pixels; -> the C reading's load at channels[0]"""
    (va, ia), (vb, ib, _) = qoix_ref_c.header(f), qoix_ref.parse(f)
    assert va == vb, (name, va, vb)
    assert ia == ib, (name, ia, ib)
    first = None
    for k, ch in enumerate(channels):
        a, b = qoix_ref_c.load(f, ch), qoix_ref.decode(f, ch)
        assert (a is None) == (b is None), (name, ch, a is None, b is None)
        if a is not None:
            assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]), (name, ch)
            assert a[1] == b[1] == ia
        if k == 0:
            first = a
    return va, first


def test_the_two_readings_agree_on_every_named_case():
    cap = _cap()
    assert cap >= 256
    cases = qoix_cases.small_cases() + qoix_cases.row_capacity(cap)
    assert len({n for n, _, _ in cases}) == len(cases) > 150
    seen = set()
    for name, f, expect in cases:
        verdict, loaded = _agree(name, f)
        if expect == "ok":
            assert verdict == qoix_ref_c.OK and loaded is not None, name
            seen.add((loaded[1]["channels"], loaded[1]["compression"]))
        elif expect == "unsupported":
            assert verdict == qoix_ref_c.UNSUPPORTED, name
        else:
            assert loaded is None and verdict in (qoix_ref_c.OK, qoix_ref_c.REFUSED), name
            if name.startswith("header_"):
                assert verdict == qoix_ref_c.REFUSED, name
    assert seen == {(3, 0), (3, 1), (4, 0), (4, 1)}


def test_what_some_named_cases_must_decode_to():
    """values worked out by hand from the format, so that the two readings cannot be wrong together on the basics"""
    d = {n: f for n, f, _ in qoix_cases.small_cases()}
    px = lambda name, ch: qoix_ref_c.load(d[name], ch)[0].reshape(-1, ch).tolist()
    assert px("no_ops_at_all_size_29", 4) == [[0, 0, 0, 255]] * 6
    assert px("fifo_slot_never_written_is_0_0_0_0", 4) == [[0, 0, 0, 0]] * 2
    assert px("rgba_op_whose_operands_are_the_last_four_bytes", 4) == [[1, 1, 1, 255], [9, 8, 7, 6]]
    assert px("adiff_chain_into_the_last_four_bytes_then_a_whole_op", 4) == [[5, 5, 5, 0]]
    assert px("adiff_wraps_255_plus_3_and_0_minus_4", 4) == [[9, 9, 9, 2], [1, 1, 1, 0], [2, 2, 2, 252]]
    assert px("index_replaces_the_alpha_an_adiff_just_set", 4) == [[5, 6, 7, 200], [5, 6, 7, 200], [0, 0, 0, 0]]
    assert px("run_repeats_the_alpha_an_adiff_just_set", 4) == [[4, 4, 4, 255]] + [[4, 4, 4, 253]] * 4
    assert px("index_does_not_write_the_fifo", 4) == [[9, 9, 9, 255]] * 3 + [[8, 8, 8, 255]] * 2 + [[0, 0, 0, 0]]
    assert px("fifo_wraps_at_64_writes", 4)[65:69] == [[65, 65, 65, 255], [2, 2, 2, 255], [64, 64, 64, 255], [3, 3, 3, 255]]
    assert px("luma_bias_1_for_a_negative_green_delta_and_2_otherwise", 3) == [[100, 100, 100], [98, 99, 101], [96, 99, 102], [100, 102, 103]]
    assert px("bytes_wrap_250_plus_10_and_2_minus_16", 3)[:4] == [[250, 250, 250], [11, 4, 11], [2, 2, 2], [234, 242, 234]]
    assert px("rgba_and_adiff_ops_in_a_3_channel_file", 4)[:2] == [[1, 2, 3, 4], [1, 3, 3, 6]]
    assert px("rgba_and_adiff_ops_in_a_3_channel_file", 3)[:2] == [[1, 2, 3], [1, 3, 3]]
    # LOCO-I: a = 10, b = 20, c = 30 -> min; a = 20, b = 20, c = 20 -> 20; a = 30, b = 15, c = 30 -> min = 15
    assert px("loco_branches_(10,20,30)_per_channel_rotated", 3)[4] == [10, 20, 15]
    # a = 10, b = 30, c = 20 -> a + b - c; a = 20, b = 20, c = 40 -> min; a = 0, b = 255, c = 128 -> 127
    assert px("loco_branches_(10,30,20)_per_channel_rotated", 3)[4] == [20, 20, 127]
    r = qoix_ref_c.load(d["run_past_the_image_end_is_cut"], 3)[0]
    assert r.shape == (3, 3, 3) and (r == [40, 50, 60]).all()


def test_the_two_readings_agree_on_random_op_streams():
    rng = np.random.default_rng(7)
    firsts = np.array([0x00, 0x35, 0x7f, 0x80, 0x85, 0xbf, 0xc0, 0xdf, 0xe0, 0xe7, 0xe8, 0xeb, 0xef, 0xf0, 0xf3, 0xf7, 0xf8, 0xfb, 0xfc, 0xfd, 0xfe, 0xff], np.uint8)
    n_ok = n_bad = 0
    for k in range(3000):
        w, h = int(rng.integers(1, 10)), int(rng.integers(1, 6))
        n = int(rng.integers(0, 2 * w * h + 4))
        body = rng.integers(0, 256, n, dtype=np.uint8)
        pick = rng.random(n) < 0.5                                           # half the bytes from the range borders; END in every other file; ADIFF closing bytes in every fourth
        body[pick] = rng.choice(firsts[:-1] if k % 2 else firsts, int(pick.sum()))
        f = G.stored(w, h, body.tobytes(), int(rng.integers(3, 5)), pad=(rng.choice(firsts[10:13], 4) if k % 4 == 1 else rng.integers(0, 256, 4, dtype=np.uint8)).tobytes(), colorspace=int(rng.integers(0, 3)))
        if k % 5 == 0:
            f = G.compressed(w, h, body.tobytes(), f[13], pad=f[-4:])
        _, loaded = _agree(("random", k), f, channels=(int(rng.choice([0, 3, 4])),))
        n_ok += loaded is not None
        n_bad += loaded is None
    assert n_ok > 500 and n_bad > 200, (n_ok, n_bad)


def test_the_two_readings_agree_on_mutated_files():
    files = qoix_cases.mutated()
    assert len(files) > 500
    verdicts = [_agree(name, f, channels=(4,))[1] is not None for name, f in files]
    assert 100 < sum(verdicts) < len(files) - 100


def test_generator_written_images_round_trip_through_both_readings():
    for name, f, _, img in qoix_cases.content():
        for ch in (0, 3, 4):
            a, b = qoix_ref_c.load(f, ch), qoix_ref.decode(f, ch)
            want = img if ch in (0, img.shape[2]) else img[..., :3] if ch == 3 else np.dstack([img, np.full(img.shape[:2], 255, np.uint8)])
            assert np.array_equal(a[0], want) and np.array_equal(b[0], want), (name, ch)
    sizes = {n: len(f) for n, f, _, _ in qoix_cases.content()}
    assert sizes["flat_199x151_rgba_lz4"] < sizes["flat_199x151_rgba_stored"]           # the flat image is what LZ4 is for
    rng = np.random.default_rng(3)
    for k in range(40):
        w, h, ch = int(rng.integers(1, 40)), int(rng.integers(1, 12)), int(rng.integers(3, 5))
        img = qoix_cases._noisy(w, h, ch, k) if k % 2 else rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        if k % 4 == 3:
            img[..., :3] //= 64                                              # few colours: INDEX hits and runs
        for lz in (False, True):
            f = G.encode(img, lz4=lz)
            assert np.array_equal(qoix_ref_c.load(f)[0], img) and np.array_equal(qoix_ref.decode(f)[0], img), (k, lz)


def _lib_header(f):
    L = _capi.lib()
    buf = np.frombuffer(bytes(f) + b"\0", np.uint8)
    info = _capi.QoixInfo()
    rc = L.gamut_hip_qoix_read_header(buf.ctypes.data, len(f), C.byref(info))
    if rc != _capi.OK:
        assert L.gamut_hip_last_error().startswith(b"qoix:")
    words = np.frombuffer(bytes(info), np.int32)                             # the floats as their bits
    return {_capi.OK: qoix_ref_c.OK, _capi.ERR_DECODE: qoix_ref_c.REFUSED, _capi.ERR_UNSUPPORTED: qoix_ref_c.UNSUPPORTED}[rc], \
        {k: int(v) for k, v in zip(qoix_ref_c.INFO_FIELDS, words)}


def test_read_header_equals_the_restatement_on_every_case():
    """verdict and every field; where the library's early test of `orig` against 255 * (length - 29) refuses a header that the
    restatement's header part accepts, the restatement's LOAD must refuse the file: the early test never changes a verdict"""
    files = [(n, f) for n, f, _ in qoix_cases.small_cases() + qoix_cases.row_capacity(_cap())] + qoix_cases.mutated()
    early = 0
    for name, f in files:
        (va, ia), (vb, ib) = _lib_header(f), qoix_ref_c.header(f)
        assert ia == ib, (name, ia, ib)
        if vb == qoix_ref_c.OK and ib["compression"] == 1 and ib["orig"] > 255 * (len(f) - 29):
            assert va == qoix_ref_c.REFUSED and qoix_ref_c.load(f) is None and qoix_ref.decode(f) is None, name
            early += 1
        else:
            assert va == vb, (name, va, vb)
    assert early >= 5
    info = _capi.QoixInfo()
    assert _capi.lib().gamut_hip_qoix_read_header(None, 0, None) == _capi.ERR_INVALID_ARG
    assert _capi.lib().gamut_hip_qoix_read_header(None, 100, C.byref(info)) == _capi.ERR_DECODE and info.detected == 0
    d = {n: f for n, f, _ in qoix_cases.small_cases()}
    assert _lib_header(d["colorspace_2_with_4_channels_is_rgbap8"])[1]["pixel_type"] == 15
    hd = _lib_header(d["header_par_and_dpi_bits_are_kept"])[1]
    assert (hd["pixel_aspect_ratio"] & 0xFFFFFFFF, hd["resolution_y"] & 0xFFFFFFFF) == (0x7fc01234, 0x80000000)


def test_identification():
    from gamut_amd import image as gi
    L = _capi.lib()
    gi.lib()

    def ident(data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return L.gamut_identify_format_from_memory(buf.ctypes.data, len(data)), L.gamut_hip_identify_format(buf.ctypes.data, len(data))
    f = qoix_cases.BASE
    assert gi.FORMAT_QOIX == 3
    assert ident(f) == (3, -1) and ident(b"qoix") == (3, -1) and ident(b"qoi") == (-1, -1)        # the batch-level test keeps treating it as unknown
    assert ident(b"qoif" + f[4:]) == (2, 2) and ident(b"qoiy" + f[4:]) == (-1, -1)
    assert ident(b"qoix" + b"\0" * 40) == (3, -1)                           # 'o' is no TGA colour-map type: the TGA test cannot claim the signature


def test_qoix_info_layout_in_the_d_binding(tmp_path):
    """gamut_hip_qoix_info four ways: the C compiler's layout (tests/c/qoix_abi_layout.c), the static assert in bindings/gamut_hip.d, the
    layout the D declaration yields, and the ctypes mirror.  (`version` is a D keyword: the binding's field is version_.)"""
    exe = str(tmp_path / "qoix_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "qoix_abi_layout.c"), "-o", exe])
    f = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert f[0] == "gamut_hip_qoix_info"
    c_size, c_fields = int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    assert list(c_fields) == list(qoix_ref_c.INFO_FIELDS) and c_size == 48
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    m = re.search(r"static assert\((\d+) == gamut_hip_qoix_info\.sizeof(.*?)\);", dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n.rstrip("_"): int(v) for v, n in re.findall(r"(\d+) == gamut_hip_qoix_info\.(\w+)\.offsetof", m.group(2))} == c_fields
    decl = re.search(r"struct gamut_hip_qoix_info\s*\{(.*?)\}", dsrc, flags=re.S).group(1)
    off, fields = 0, {}
    for part in [x.strip() for x in decl.split(";") if x.strip()]:
        typ, names = part.split(None, 1)
        assert typ in ("int", "float")
        for n in names.split(","):
            fields[n.strip().rstrip("_")] = off; off += 4
    assert (off, fields) == (c_size, c_fields)
    assert C.sizeof(_capi.QoixInfo) == c_size and {n: getattr(_capi.QoixInfo, n).offset for n, _ in _capi.QoixInfo._fields_} == c_fields
    assert [t for _, t in _capi.QoixInfo._fields_][7:9] == [C.c_float, C.c_float]


def test_bad_arguments_and_no_device():
    L = _capi.lib()
    f = np.frombuffer(qoix_cases.BASE, np.uint8)
    out = np.full(64, 0xA5, np.uint8)
    ptrs, lens, off = (C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), (C.c_int64 * 1)(0)
    for ch in (1, 2, 5, -1):
        assert L.gamut_hip_qoix_decode_batch_device(ptrs, lens, 1, ch, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_qoix_decode_batch_device(ptrs, lens, -1, 0, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_qoix_decode_batch_device(None, None, 0, 0, None, None, None, None, None) == _capi.OK
    assert L.gamut_hip_qoix_last_decode_stage_ms(2) == -1.0
    if L.gamut_hip_device_count() == 0:                                      # no GPU: a loud failure, outputs untouched
        st = (C.c_int * 1)(55)
        assert L.gamut_hip_qoix_decode_batch_device(ptrs, lens, 1, 4, off, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()
        typ = C.c_int(99)
        assert L.gamut_hip_qoix_lz4_decode(f.ctypes.data, f.size, None, 0, C.byref(typ)) is None and typ.value == -1


def test_host_image_refuses_malformed_headers_without_a_gpu():
    from gamut_amd import image as gi
    d = {n: f for n, f, _ in qoix_cases.small_cases()}
    for name in ("header_width_0", "header_channels_5", "header_size_25", "header_compression_2", "unsupported_10bit_3ch", "unsupported_8bit_1ch",
                 "lz4_orig_0x80000000", "header_lz4_size_28"):
        im = gi.Image()
        assert not im.loadFromMemory(d[name]) and not im.isValid, name
        assert im.errorMessage == "Image decoding failed", (name, im.errorMessage)     # kStrImageDecodingFailed
    im = gi.Image()
    assert not im.loadFromMemory(d["header_bad_signature"][:3]) and im.errorMessage == "Unidentified image format"
    im = gi.Image()
    assert not im.loadFromMemory(qoix_cases.BASE, gi.LOAD_RGB | gi.LOAD_GREYSCALE) and im.errorMessage == "Invalid image decoding flags"
    if _capi.lib().gamut_hip_device_count() == 0:
        im = gi.Image()
        assert not im.loadFromMemory(qoix_cases.BASE) and im.errorMessage == "Image decoding failed"
