"""The SQZ device writer without a GPU: the scan tables it uploads (gamut_hip_sqz_scan_order) against the C restatement's scanners,
the new entries on bad arguments and without a device, the writer switch, and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sqz_ref_c as R
from gamut_amd import _capi
from gamut_amd import image as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gamut_hip_sqz_write_batch_device", "gamut_hip_sqz_encode_batch_to_device", "gamut_hip_sqz_scan_order", "gamut_hip_sqz_write_chunk",
       "gamut_hip_sqz_last_write_stage_ms", "gamut_hip_sqz_set_writer")


@pytest.fixture(scope="module")
def L():
    return _capi.lib()


def scan_order(L, order, w, h):
    xy = np.full((w * h + 8, 2), 0xBEEF, np.uint16)                          # a guard behind the table
    rc = L.gamut_hip_sqz_scan_order(order, w, h, xy.ctypes.data)
    assert (xy[w * h:] == 0xBEEF).all()
    return rc, xy[:w * h]


@pytest.mark.parametrize("order", range(4))
def test_scan_order_equals_the_reference_scanners(L, order):
    sizes = [(w, h) for w in range(1, 21) for h in range(1, 21)] + [(60, 34), (64, 36), (135, 240), (34, 60), (240, 135)]
    for w, h in sizes:
        rc, got = scan_order(L, order, w, h)
        want = R.scan(order, w, h)
        assert rc == 0 and want.shape == (w * h, 2) and np.array_equal(got, want), (order, w, h)
        if order == 0:
            assert np.array_equal(got[:, 0] + w * got[:, 1].astype(np.int64), np.arange(w * h))
        assert len({(int(x), int(y)) for x, y in got}) == w * h             # a permutation of the band


def test_scan_order_refuses_bad_arguments(L):
    xy = np.full(64, 0xBEEF, np.uint16)
    for order, w, h in ((-1, 4, 4), (4, 4, 4), (0, 0, 4), (1, 4, 0), (2, -3, 4), (3, 4, -1), (1, 65536, 1)):
        assert L.gamut_hip_sqz_scan_order(order, w, h, xy.ctypes.data) == _capi.ERR_INVALID_ARG, (order, w, h)
        assert b"sqz_scan_order" in L.gamut_hip_last_error()
    assert L.gamut_hip_sqz_scan_order(1, 4, 4, None) == _capi.ERR_INVALID_ARG
    assert (xy == 0xBEEF).all()


def one_desc(budget=100):
    d = (_capi.SqzEncodeDesc * 1)()
    d[0].width, d[0].height, d[0].color_mode, d[0].levels, d[0].scan_order, d[0].subsampling, d[0].budget = 16, 16, 0, 1, 1, 0, budget
    return d


def test_the_batch_entries_refuse_bad_arguments(L):
    d = one_desc()
    co = np.zeros(256, np.int16)
    px = np.zeros(256, np.uint8)
    out = np.full(256, 0xA5, np.uint8)
    off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1); st = (C.c_int * 1)(-7)
    w = L.gamut_hip_sqz_write_batch_device
    good = [co.ctypes.data, off, d, 1, off, out.ctypes.data, ln, st, None]
    for k in (0, 1, 2, 4, 5, 6):                                            # every pointer but status_host and the stream
        args = list(good)
        args[k] = None
        assert w(*args) == _capi.ERR_INVALID_ARG and b"sqz_write_batch_device" in L.gamut_hip_last_error(), k
    args = list(good); args[3] = -1
    assert w(*args) == _capi.ERR_INVALID_ARG
    assert w(None, None, None, 0, None, None, None, None, None) == 0        # an empty batch is fine
    e = L.gamut_hip_sqz_encode_batch_to_device
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(16)
    good = [src, pitch, d, 1, off, out.ctypes.data, ln, st, None]
    for k in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert e(*args) == _capi.ERR_INVALID_ARG and b"sqz_encode_batch_to_device" in L.gamut_hip_last_error(), k
    args = list(good); args[3] = -2
    assert e(*args) == _capi.ERR_INVALID_ARG
    assert e(None, None, None, 0, None, None, None, None, None) == 0
    assert (out == 0xA5).all() and ln[0] == -1 and st[0] == -7


def test_without_a_device_the_entries_fail_and_touch_nothing(L):
    if L.gamut_hip_device_count() > 0:
        return                                                              # tests/test_sqz_write_gpu.py is the test then
    d = one_desc()
    co = np.zeros(256, np.int16)
    px = np.zeros(256, np.uint8)
    out = np.full(256, 0xA5, np.uint8)
    off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_sqz_write_batch_device(co.ctypes.data, off, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(16)
    assert L.gamut_hip_sqz_encode_batch_to_device(src, pitch, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    assert (out == 0xA5).all() and ln[0] == -1 and st[0] == -7
    prev = L.gamut_hip_sqz_set_writer(1)                                    # the switched entries say the same with either writer
    try:
        assert L.gamut_hip_sqz_encode_batch_device(src, pitch, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
        n = C.c_int(-1)
        assert not L.gamut_hip_sqz_write_to_mem(px.ctypes.data, 16, d, C.byref(n)) and n.value == 0
    finally:
        L.gamut_hip_sqz_set_writer(prev)
    assert (out == 0xA5).all() and ln[0] == -1 and st[0] == -7
    img = gi.Image()
    assert img.createView(np.zeros((16, 48), np.uint8), 16, 16, 9, 48)
    assert img.save_sqz_to_device() is None and img.isValid and img.errorMessage is None


def test_the_writer_switch(L):
    if os.environ.get("GAMUT_HIP_SQZ_WRITER", "host") == "host":
        assert L.gamut_hip_sqz_set_writer(0) == 0                           # the default is the host writer
    prev = L.gamut_hip_sqz_set_writer(1)
    try:
        assert prev in (0, 1)
        assert L.gamut_hip_sqz_set_writer(0) == 1 and L.gamut_hip_sqz_set_writer(0) == 0
        assert L.gamut_hip_sqz_set_writer(7) == 0 and L.gamut_hip_sqz_set_writer(-1) == 0 and L.gamut_hip_sqz_set_writer(1) == 0      # no such writer: nothing changes
        assert L.gamut_hip_sqz_set_writer(1) == 1
    finally:
        L.gamut_hip_sqz_set_writer(prev)
    assert L.gamut_hip_sqz_set_writer(prev) == prev


def test_chunk_and_stage_timings(L):
    c = L.gamut_hip_sqz_write_chunk()
    assert c >= 64 and c % 64 == 0                                          # whole waves
    assert L.gamut_hip_sqz_last_write_stage_ms(9) == -1 and L.gamut_hip_sqz_last_write_stage_ms(-1) == -1
    assert L.gamut_hip_sqz_last_write_stage_ms(0) == -1 and L.gamut_hip_sqz_last_write_stage_ms(1) == -1      # no call yet on this thread


def test_the_image_entry_refuses_without_an_image():
    Li = gi.lib()
    n = C.c_size_t(5)
    assert not Li.gamut_image_save_sqz_to_device(None, 0, C.byref(n)) and n.value == 0
    img = gi.Image()
    assert not Li.gamut_image_save_sqz_to_device(img.h, 0, None)
    assert img.save_sqz_to_device() is None                                 # "Uninitialized image" stays what it is
    host = gi.Image()
    assert host.createView(np.zeros((16, 48), np.uint8), 16, 16, 9, 48)
    assert host.save_sqz_to_device() is None and host.isValid               # a host-resident image has no file in HBM


def test_the_bindings_list_the_new_entries(L):
    header = open(os.path.join(ROOT, "include", "gamut_hip.h")).read()
    dbind = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, dbind), name
        res, args = _capi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "gamut_image_save_sqz_to_device" in open(os.path.join(ROOT, "include", "gamut_image.h")).read()
    assert gi.lib().gamut_image_save_sqz_to_device.argtypes is not None
