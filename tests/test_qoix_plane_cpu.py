"""QOI-Plane (QOIX grey files) without a GPU.  As for the colour codec, no file written by the reference exists, so the pin is two
independent readings of its text -- tests/c/qoiplane_ref.c, serial C with the reference's scanline structure, and tests/qoiplane_ref.py,
Python on whole-image arrays -- held against each other on every named case, on values worked out by hand, on random nibble streams and
on mutated files, plus round trips of generator-written images.  Then the library's host side with gamut_hip_qoix_set_plane: the header,
the setter, the exports, and what the entries answer without a device.  The switch is process-wide: every test that turns it on does so
through a fixture that restores the value it found."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qoiplane_cases as K
import qoiplane_gen as P
import qoiplane_ref
import qoiplane_ref_c
import qoix_gen as G
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture
def plane_on():
    L = _capi.lib()
    prev = L.gamut_hip_qoix_set_plane(1)
    yield L
    L.gamut_hip_qoix_set_plane(prev)


def _cap():
    return _capi.lib().gamut_hip_qoix_plane_row_capacity()


def _agree(name, f, channels=(0, 1, 2)):
    """both readings on one file: header verdict, info, and per channel count the load verdict and the pixels; -> (verdict, the C reading's load at channels[0])"""
    (va, ia), (vb, ib, _) = qoiplane_ref_c.header(f), qoiplane_ref.parse(f)
    assert va == vb, (name, va, vb)
    assert ia == ib, (name, ia, ib)
    first = None
    for k, ch in enumerate(channels):
        a, b = qoiplane_ref_c.load(f, ch), qoiplane_ref.decode(f, ch)
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
    cases = K.small_cases() + K.row_capacity(cap)
    assert len({n for n, _, _ in cases}) == len(cases) > 120
    seen = set()
    for name, f, expect in cases:
        verdict, loaded = _agree(name, f)
        assert expect in ("ok", "refused")
        if expect == "ok":
            assert verdict == qoiplane_ref_c.OK and loaded is not None, name
            seen.add((loaded[1]["channels"], loaded[1]["compression"]))
        else:
            assert loaded is None, name
            if name.startswith(("header_", "colorspace_2")):
                assert verdict == qoiplane_ref_c.REFUSED, name
            if name.startswith("deviation_p1"):
                assert verdict == qoiplane_ref_c.OK, name
    assert seen == {(1, 0), (1, 1), (2, 0), (2, 1)}


def test_values_worked_out_by_hand():
    """so that the two readings cannot be wrong together on the basics"""
    cases = K.hand_worked()
    assert len(cases) == 10
    for name, f, expect, ch, pixels in cases:
        a, b = qoiplane_ref_c.load(f, ch), qoiplane_ref.decode(f, ch)
        if expect == "refused":
            assert a is None and b is None and qoiplane_ref_c.header(f)[0] == qoiplane_ref_c.OK, name       # deviation P1, not the header
        else:
            assert a[0].reshape(-1).tolist() == pixels and b[0].reshape(-1).tolist() == pixels, (name, a[0].reshape(-1).tolist())
    d = {n: f for n, f, _, _, _ in cases}
    assert len(d["no_body_29_bytes_4x2_2ch"]) == 29
    assert d["closing_bytes_are_decoded_5x2"][-4:] == b"\x44" * 4 == d["deviation_p1_closing_bytes_run_out_5x4"][-4:]
    d = {n: f for n, f, _ in K.small_cases()}
    px = lambda name, ch: qoiplane_ref_c.load(d[name], ch)[0].reshape(-1, ch).tolist()
    assert px("adiff_in_front_of_a_repeat_gives_the_run_the_new_alpha", 2)[:10] == [[9, 100]] + [[9, 105]] * 6 + [[9, 103]] * 3
    assert px("adiff_then_la_the_la_wins", 2) == [[1, 50], [2, 60]]
    assert px("adiff_wraps_255_plus_3_and_0_minus_4", 2) == [[9, 2], [1, 0], [1, 252]]
    assert px("direct_in_a_2_channel_file_sets_luminance_only", 2) == [[5, 40], [200, 40], [201, 40]]
    assert px("direct_in_a_2_channel_file_sets_luminance_only", 1) == [[5], [200], [201]]
    assert px("repeat_as_the_first_op_repeats_0_255", 2) == [[0, 255]] * 3 + [[7, 255]] * 5 + [[7, 255]] * 2
    assert px("surplus_ops_are_ignored", 1) == [[1], [2]]
    assert px("an_op_that_ends_with_the_files_last_nibble", 1)[-1] == [77]
    r = qoiplane_ref_c.load(d["run_past_the_image_end_is_cut"], 1)[0]
    assert r.shape == (3, 3, 1) and (r == 40).all()


def test_the_two_readings_agree_on_random_nibble_streams():
    rng = np.random.default_rng(5)
    n_ok = n_bad = 0
    for k in range(3000):
        w, h, ch = int(rng.integers(1, 10)), int(rng.integers(1, 6)), int(rng.integers(1, 3))
        body = rng.integers(0, 256, int(rng.integers(0, w * h * ch + 3)), dtype=np.uint8)
        if k % 3:                                                           # two thirds of the bodies without any f nibble ...
            body[(body >> 4) == 15] &= 0x7f
            body[(body & 15) == 15] &= 0xf7
            if k % 9 in (1, 2):                                             # ... and a third of those cut to a third of their length
                body = body[:len(body) // 3]
        closing = b"\xff" * 4 if k % 2 == 0 else rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        f = G.header(w, h, ch) + body.tobytes() + closing
        _, loaded = _agree(("random", k), f, channels=(int(rng.choice([0, 1, 2])),))
        n_ok += loaded is not None
        n_bad += loaded is None
    print("random nibble streams: accepted", n_ok, "refused", n_bad)
    assert n_ok >= 1500 and n_bad >= 150, (n_ok, n_bad)


def test_the_two_readings_agree_on_mutated_files():
    files = K.mutated()
    assert len(files) > 500
    verdicts = [_agree(name, f, channels=(2,))[1] is not None for name, f in files]
    print("mutated files:", len(files), "accepted", sum(verdicts))
    assert sum(verdicts) > 100 and len(files) - sum(verdicts) > 100


def test_generator_written_images_round_trip_through_both_readings():
    def wanted(img, ch):
        if ch in (0, img.shape[2]):
            return img
        return img[..., :1] if ch == 1 else np.dstack([img, np.full(img.shape[:2], 255, np.uint8)])
    for name, f, _, img in K.content():
        for ch in (0, 1, 2):
            a, b = qoiplane_ref_c.load(f, ch), qoiplane_ref.decode(f, ch)
            assert np.array_equal(a[0], wanted(img, ch)) and np.array_equal(b[0], wanted(img, ch)), (name, ch)
    sizes = {n: len(f) for n, f, _, _ in K.content()}
    assert sizes["flat_199x151_la8_lz4"] < sizes["flat_199x151_la8_stored"]
    rng = np.random.default_rng(3)
    for k in range(48):
        w, h, ch = int(rng.integers(1, 40)), int(rng.integers(1, 12)), 1 + k % 2
        img = (P.noisy(w, h, ch, k), P.flat_image(w, h, ch, k), P.few_levels(w, h, ch, k), P.alpha_ramp(w, h, k, step=1 + k % 11),
               rng.integers(0, 256, (h, w, ch), dtype=np.uint8), P.alpha_ramp(w, h, k, step=37))[k % 6]
        for lz in (False, True):
            f = P.encode(img, lz4=lz)
            assert np.array_equal(qoiplane_ref_c.load(f)[0], img) and np.array_equal(qoiplane_ref.decode(f)[0], img), (k, lz)
    n = P.encode_nibbles(np.full((1, 600, 1), 0, np.uint8))                 # 600 pixels equal to the initial one: runs cut at 258 and at the last pixel
    assert n[:9] == P.REPEAT2(258) * 2 + P.REPEAT2(84) and n[9:] == [15] * 9


def _lib_header(f):
    L = _capi.lib()
    buf = np.frombuffer(bytes(f) + b"\0", np.uint8)
    info = _capi.QoixInfo()
    rc = L.gamut_hip_qoix_read_header(buf.ctypes.data, len(f), C.byref(info))
    words = np.frombuffer(bytes(info), np.int32)
    return {_capi.OK: qoiplane_ref_c.OK, _capi.ERR_DECODE: qoiplane_ref_c.REFUSED, _capi.ERR_UNSUPPORTED: qoiplane_ref_c.UNSUPPORTED}[rc], \
        {k: int(v) for k, v in zip(qoiplane_ref_c.INFO_FIELDS, words)}


def test_read_header_with_the_switch_on_and_off(plane_on):
    L = plane_on
    files = [(n, f) for n, f, _ in K.small_cases() + K.row_capacity(_cap())] + K.mutated()
    grey_ok = 0
    for name, f in files:
        (va, ia), (vb, ib) = _lib_header(f), qoiplane_ref_c.header(f)
        assert ia == ib, (name, ia, ib)
        if vb == qoiplane_ref_c.OK and ib["compression"] == 1 and ib["orig"] > 255 * (len(f) - 29):         # the early refusal never changes a verdict
            assert va == qoiplane_ref_c.REFUSED and qoiplane_ref_c.load(f) is None, name
        else:
            assert va == vb, (name, va, vb)
        grey = vb != qoiplane_ref_c.UNSUPPORTED and ib["pixel_type"] in (0, 3, 6) and ib["compression"] in (0, 1) and (ib["compression"] == 0 or (len(f) >= 29 and ib["orig"] >= 0))
        if grey:                                                            # switch off: the same file is UNSUPPORTED, fields unchanged
            assert L.gamut_hip_qoix_set_plane(0) == 1
            try:
                v0, i0 = _lib_header(f)
            finally:
                assert L.gamut_hip_qoix_set_plane(1) == 0
            assert v0 == qoiplane_ref_c.UNSUPPORTED and i0 == ia, (name, v0)
            grey_ok += vb == qoiplane_ref_c.OK
    assert grey_ok > 300
    d = {n: f for n, f, _ in K.small_cases()}
    v, hd = _lib_header(d["colorspace_2_with_2_channels_is_lap8_and_refused_by_the_sub_codec"])
    assert v == qoiplane_ref_c.REFUSED and hd["pixel_type"] == 6 and b"colorspace" in L.gamut_hip_last_error()
    assert _lib_header(d["geometry_65x3_1ch"])[1]["pixel_type"] == 0 and _lib_header(d["geometry_65x3_2ch"])[1]["pixel_type"] == 3
    assert _lib_header(d["ten_bit_1_channel_is_still_unsupported"])[0] == qoiplane_ref_c.UNSUPPORTED


def test_the_setter():
    L = _capi.lib()
    start = L.gamut_hip_qoix_set_plane(1)
    try:
        assert start in (0, 1)
        assert L.gamut_hip_qoix_set_plane(0) == 1 and L.gamut_hip_qoix_set_plane(0) == 0
        for bad in (2, -1):
            assert L.gamut_hip_qoix_set_plane(bad) == 0 and L.gamut_hip_qoix_set_plane(0) == 0
        assert L.gamut_hip_qoix_set_plane(1) == 0
        for bad in (2, -1):
            assert L.gamut_hip_qoix_set_plane(bad) == 1 and L.gamut_hip_qoix_set_plane(1) == 1
    finally:
        L.gamut_hip_qoix_set_plane(start)
    assert L.gamut_hip_qoix_set_plane(start) == start


def test_a_fresh_process_takes_the_initial_value_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); from gamut_amd import _capi; L = _capi.lib(); v = L.gamut_hip_qoix_set_plane(7); print('value', v)" % ROOT)
    for env, want in (("1", 1), ("0", 0), (None, 0), ("yes", 0)):
        e = {k: v for k, v in os.environ.items() if k != "GAMUT_HIP_QOIX_PLANE"}
        if env is not None:
            e["GAMUT_HIP_QOIX_PLANE"] = env
        out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
        assert "value %d" % want in out, (env, out)


def test_the_new_exports_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "gamut_hip.h")).read()
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    for name in ("gamut_hip_qoix_set_plane", "gamut_hip_qoix_plane_row_capacity", "gamut_hip_qoix_last_plane_kernel_ms"):
        assert name in _capi.SIGNATURES and hasattr(_capi.lib(), name), name
        assert name + "(" in header and name + "(" in dsrc, name
    assert _capi.lib().gamut_hip_qoix_last_plane_kernel_ms() == -1.0 or os.environ.get("GAMUT_HIP_QOIX_TIMING") == "1"


def test_without_a_device_the_entries_fail_loudly(plane_on):
    from gamut_amd import image as gi
    L = plane_on
    f = np.frombuffer(K.small_cases()[0][1], np.uint8)
    out = np.full(64, 0xA5, np.uint8)
    ptrs, lens, off = (C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), (C.c_int64 * 1)(0)
    for ch in (5, -1):
        assert L.gamut_hip_qoix_decode_batch_device(ptrs, lens, 1, ch, off, out.ctypes.data, None, None, None) == _capi.ERR_INVALID_ARG
    im = gi.Image()
    assert not im.loadFromMemory(dict((n, f) for n, f, _ in K.small_cases())["colorspace_2_with_2_channels_is_lap8_and_refused_by_the_sub_codec"])
    assert im.errorMessage == "Image decoding failed"
    if L.gamut_hip_device_count() == 0:
        for ch in (0, 1, 2):
            st = (C.c_int * 1)(55)
            assert L.gamut_hip_qoix_decode_batch_device(ptrs, lens, 1, ch, off, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
            assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()
        typ = C.c_int(99)
        assert L.gamut_hip_qoix_lz4_decode(f.ctypes.data, f.size, None, 0, C.byref(typ)) is None and typ.value == -1
        im = gi.Image()
        assert not im.loadFromMemory(K.small_cases()[0][1]) and im.errorMessage == "Image decoding failed"
