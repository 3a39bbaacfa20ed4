"""The SQZ device reader without a GPU: the new entries on bad arguments and without a device, the reader switch, the bindings, and the
rules the reader is built on -- a position-parallel model in numpy (tests/sqz_read_model.py) against the serial C restatement
(tests/c/sqz_ref.c), coefficient for coefficient."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sqz_cases
import sqz_read_model as M
import sqz_ref_c as R
from gamut_amd import _capi
from gamut_amd import image as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gamut_hip_sqz_read_batch_device", "gamut_hip_sqz_set_reader", "gamut_hip_sqz_read_window", "gamut_hip_sqz_set_read_chunk",
       "gamut_hip_sqz_last_read_stage_ms")


@pytest.fixture(scope="module")
def L():
    return _capi.lib()


def test_the_bindings_list_the_new_entries(L):
    header = open(os.path.join(ROOT, "include", "gamut_hip.h")).read()
    dbind = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, dbind), name
        res, args = _capi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_reader_switch(L):
    if os.environ.get("GAMUT_HIP_SQZ_READER", "host") == "host":
        assert L.gamut_hip_sqz_set_reader(0) == 0                           # the default is the host front end
    prev = L.gamut_hip_sqz_set_reader(1)
    try:
        assert prev in (0, 1)
        assert L.gamut_hip_sqz_set_reader(0) == 1 and L.gamut_hip_sqz_set_reader(0) == 0
        assert L.gamut_hip_sqz_set_reader(7) == 0 and L.gamut_hip_sqz_set_reader(-1) == 0 and L.gamut_hip_sqz_set_reader(2) == 0      # no such reader: nothing changes
        assert L.gamut_hip_sqz_set_reader(1) == 0 and L.gamut_hip_sqz_set_reader(1) == 1
    finally:
        L.gamut_hip_sqz_set_reader(prev)
    assert L.gamut_hip_sqz_set_reader(prev) == prev


@pytest.mark.parametrize("value,want", [(None, 0), ("host", 0), ("device", 1), ("gpu", 0), ("", 0)])
def test_the_environment_sets_the_initial_reader(value, want):
    env = {k: v for k, v in os.environ.items() if k != "GAMUT_HIP_SQZ_READER"}
    if value is not None:
        env["GAMUT_HIP_SQZ_READER"] = value
    code = "from gamut_amd import _capi; L = _capi.lib(); a = L.gamut_hip_sqz_set_reader(5); print(a, L.gamut_hip_sqz_set_reader(1 - a), L.gamut_hip_sqz_set_reader(9))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(want), str(want), str(1 - want)]


def test_window_chunk_and_stage_timings(L):
    w = L.gamut_hip_sqz_read_window()
    assert 2048 <= w <= 65536 and w % 2048 == 0                             # a dword or two per lane, whole waves
    prev = L.gamut_hip_sqz_set_read_chunk(0)                                # below 1: nothing changes
    assert prev >= 1 << 22 and L.gamut_hip_sqz_set_read_chunk(-5) == prev   # the default holds a 2048 x 2048 grey file at the least
    try:
        assert L.gamut_hip_sqz_set_read_chunk(1000) == prev and L.gamut_hip_sqz_set_read_chunk(1 << 40) == 1000
        assert L.gamut_hip_sqz_set_read_chunk(0) == 1 << 40
    finally:
        L.gamut_hip_sqz_set_read_chunk(prev)
    assert L.gamut_hip_sqz_set_read_chunk(0) == prev
    assert L.gamut_hip_sqz_last_read_stage_ms(9) == -1 and L.gamut_hip_sqz_last_read_stage_ms(-1) == -1
    assert L.gamut_hip_sqz_last_read_stage_ms(0) == -1 and L.gamut_hip_sqz_last_read_stage_ms(1) == -1      # no call yet on this thread


def one_file():
    f = np.frombuffer(sqz_cases.make(16, 16, R.GREY, 1), np.uint8).copy()
    return f, (C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size)


def test_the_batch_entry_refuses_bad_arguments(L):
    f, ptrs, lens = one_file()
    co = np.full(256, 0x5A5A, np.int16)
    off = (C.c_int64 * 1)(0); st = (C.c_int * 1)(-7); info = (_capi.SqzInfo * 1)()
    r = L.gamut_hip_sqz_read_batch_device
    good = [ptrs, lens, 1, co.ctypes.data, off, info, st, None]
    for k in (0, 1, 3, 4):                                                  # every pointer but info, status_host and the stream
        args = list(good)
        args[k] = None
        assert r(*args) == _capi.ERR_INVALID_ARG and b"sqz_read_batch_device" in L.gamut_hip_last_error(), k
    args = list(good); args[2] = -1
    assert r(*args) == _capi.ERR_INVALID_ARG
    assert r(None, None, 0, None, None, None, None, None) == 0              # an empty batch is fine
    assert (co == 0x5A5A).all() and st[0] == -7 and info[0].width == 0


def test_without_a_device_the_entries_fail_and_touch_nothing(L):
    if L.gamut_hip_device_count() > 0:
        return                                                              # tests/test_sqz_read_gpu.py is the test then
    f, ptrs, lens = one_file()
    co = np.full(256, 0x5A5A, np.int16)
    out = np.full(256, 0xA5, np.uint8)
    off = (C.c_int64 * 1)(0); st = (C.c_int * 1)(-7)
    assert L.gamut_hip_sqz_read_batch_device(ptrs, lens, 1, co.ctypes.data, off, None, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    prev = L.gamut_hip_sqz_set_reader(1)                                    # the switched entries say the same with either reader
    try:
        assert L.gamut_hip_sqz_decode_batch_device(ptrs, lens, 1, off, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
        img = gi.Image()
        assert not img.loadFromMemory(f.tobytes())
    finally:
        L.gamut_hip_sqz_set_reader(prev)
    assert (co == 0x5A5A).all() and (out == 0xA5).all() and st[0] == -7


# ---- the rules by position: the model against the C restatement ----
def same(f):
    got, want = M.coeffs(f), R.coeffs(f)
    if want is None:
        return got is None
    return got[1] == want[1] and np.array_equal(got[0], want[0])


def test_model_on_the_named_cases():
    n = 0
    for name, f, e in sqz_cases.small_cases():
        hd = R.header(f)[1]
        if hd["width"] * hd["height"] > 128 * 72:
            continue
        assert same(f), name
        n += 1
    assert n >= 90


@pytest.mark.parametrize("which", [0, 1])
def test_model_on_every_prefix(which):
    for f in sqz_cases.prefixes(sqz_cases.prefix_files()[which]):
        assert same(f), len(f)


def test_model_on_1500_mutations():
    for k, f in enumerate(M.mutations(1500)):
        assert same(f), k


def test_model_sorting_pass_ends():
    """the three ends of a stream inside a sorting pass, bit by bit: at a flag position the pending record closes, at a sign or a data
    position nothing does"""
    bits = lambda s: np.array([int(c) for c in s], np.uint8)
    t, sg, pos, closed = M.sorting_pass(bits("1" + "0001" + "11" + "000"), 1, 64)          # ends where a flag is due: run (1 0) = 2 closes
    assert t.tolist() == [1, 2, 4] and sg.tolist() == [0, 1, 0] and not closed and pos == 10
    t, sg, pos, closed = M.sorting_pass(bits("1" + "0001" + "11"), 1, 64)                  # ends at a sign position
    assert t.tolist() == [1, 2] and sg.tolist() == [0, 1] and not closed
    t, sg, pos, closed = M.sorting_pass(bits("1" + "0001" + "11" + "00"), 1, 64)           # ends at a data position
    assert t.tolist() == [1, 2] and not closed
    t, sg, pos, closed = M.sorting_pass(bits("1" + "0001" + "11" + "000"), 1, 3)           # the closed-by-the-end record overshoots
    assert t.tolist() == [1, 2] and closed and pos == 11
