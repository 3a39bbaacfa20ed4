"""ctypes binding of tests/c/qoiplane_write_ref.c (qoiplane_encode restated serially: header, ops, closing nibbles, bound), compiled
once per process into a temporary directory.  encode() gives the file qoix_lz4_encode writes for an (h, w, 1 | 2) uint8 image: the LZ4
block and the rule that the smaller file wins come from tests/qoix_write_ref_c.py (lz4_compress), used as it is."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import qoix_write_ref_c as W

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "qoiplane_write_ref.c")
HEADER = 25
bits = W.bits


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="qoiplane_write_ref_")
    so = os.path.join(d, "libqoiplane_write_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    for name in ("qoipwref_datalen_max", "qoipwref_reference_alloc"):
        getattr(L, name).restype = C.c_longlong
        getattr(L, name).argtypes = [C.c_int] * 3
    L.qoipwref_bound.restype = C.c_longlong
    L.qoipwref_bound.argtypes = [C.c_int] * 4
    L.qoipwref_encode.restype = C.c_long
    L.qoipwref_encode.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_long]
    return L


def bound(w, h, channels, colorspace=0):
    return lib().qoipwref_bound(w, h, channels, colorspace)


def datalen_max(w, h, channels):
    return lib().qoipwref_datalen_max(w, h, channels)


def reference_alloc(w, h, channels):
    return lib().qoipwref_reference_alloc(w, h, channels)


def stored(img, colorspace=0, par=1.0, dpi=96.0):
    """img: (h, w, 1 | 2) uint8 -> the uncompressed file"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, ch = img.shape
    cap = HEADER + datalen_max(w, h, ch)
    out = np.zeros(cap, np.uint8)
    n = lib().qoipwref_encode(img.ctypes.data, w * ch, w, h, ch, colorspace, bits(par), bits(dpi), out.ctypes.data, cap)
    if n < 0:
        raise ValueError(f"qoipwref_encode: {n}")
    return out[:n].tobytes()


def encode_ex(img, mode=0, **kw):
    """-> (the file, lz4Size + 4 - datalen); mode 1: stored only (plugins/qoix.d:319-338 for mode 0)"""
    f = stored(img, **kw)
    block = W.lz4_compress(f[HEADER:])
    datalen = len(f) - HEADER
    diff = len(block) + 4 - datalen
    if mode == 0 and diff < 0:
        f = f[:16] + b"\x01" + f[17:HEADER] + struct.pack(">i", datalen) + block
    return f, diff


def encode(img, mode=0, **kw):
    return encode_ex(img, mode, **kw)[0]
