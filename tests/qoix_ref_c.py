"""ctypes binding of tests/c/qoix_ref.c (qoix_lz4_decode, LZ4_decompress_fast and qoix_decode restated serially, the four deliberate
deviations included), compiled once per process into a temporary directory.  header() gives the header verdict and fields, load() the
pixels."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "qoix_ref.c")
INFO_FIELDS = ("width", "height", "version", "channels", "bitdepth", "colorspace", "compression", "pixel_aspect_ratio", "resolution_y",
               "orig", "pixel_type", "detected")                            # the two floats as their bits
OK, REFUSED, UNSUPPORTED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="qoix_ref_")
    so = os.path.join(d, "libqoix_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.qoixref_load.restype = C.c_long
    L.qoixref_load.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    return L


def _buf(data):
    return np.frombuffer(bytes(data) + b"\0", np.uint8)


def header(data):
    """-> (verdict: OK / REFUSED / UNSUPPORTED, dict of INFO_FIELDS as far as the header was read)"""
    buf = _buf(data)
    info = np.zeros(12, np.int32)
    v = lib().qoixref_load(buf.ctypes.data, len(data), 0, None, 0, info.ctypes.data)
    return v & 3, {k: int(x) for k, x in zip(INFO_FIELDS, info)}


def load(data, channels=0):
    """-> None when the load fails (header, LZ4 block or op stream), else (pixels (h, w, channels) uint8, info dict)"""
    rc, info = header(data)
    if rc != OK:
        return None
    ch = channels or info["channels"]
    buf = _buf(data)
    out = np.zeros((info["height"], info["width"], ch), np.uint8)
    i2 = np.zeros(12, np.int32)
    v = lib().qoixref_load(buf.ctypes.data, len(data), channels, out.ctypes.data, out.size, i2.ctypes.data)
    return (out, info) if v & 32 else None
