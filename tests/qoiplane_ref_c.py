"""ctypes binding of tests/c/qoiplane_ref.c (the grey slice of qoix_lz4_decode and qoiplane_decode restated serially, deviation P1
included; colour files go to the restatement of tests/c/qoix_ref.c), compiled once per process into a temporary directory.  This is the
library with gamut_hip_qoix_set_plane(1).  header() gives the header verdict and fields, load() the pixels."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from qoix_ref_c import INFO_FIELDS, OK, REFUSED, UNSUPPORTED               # noqa: F401 (re-exported)

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "qoiplane_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="qoiplane_ref_")
    so = os.path.join(d, "libqoiplane_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.planeref_load.restype = C.c_long
    L.planeref_load.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    return L


def _buf(data):
    return np.frombuffer(bytes(data) + b"\0", np.uint8)


def header(data):
    """-> (verdict: OK / REFUSED / UNSUPPORTED, dict of INFO_FIELDS as far as the header was read)"""
    buf = _buf(data)
    info = np.zeros(12, np.int32)
    v = lib().planeref_load(buf.ctypes.data, len(data), 0, None, 0, info.ctypes.data)
    return v & 3, {k: int(x) for k, x in zip(INFO_FIELDS, info)}


def load(data, channels=0):
    """-> None when the load fails (header, LZ4 block, op stream, or a channel count of the other family), else (pixels (h, w, channels) uint8, info dict)"""
    rc, info = header(data)
    if rc != OK:
        return None
    ch = channels or info["channels"]
    buf = _buf(data)
    out = np.zeros((info["height"], info["width"], ch), np.uint8)
    i2 = np.zeros(12, np.int32)
    v = lib().planeref_load(buf.ctypes.data, len(data), channels, out.ctypes.data, out.size, i2.ctypes.data)
    return (out, info) if v & 32 else None
