"""ctypes binding of tests/c/qoix_write_ref.c (qoix_encode, LZ4_compress and qoix_lz4_encode restated serially), compiled once per
process into a temporary directory.  encode() gives the file the reference writes for an (h, w, 3 | 4) uint8 image."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "qoix_write_ref.c")
HEADER = 25


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="qoix_write_ref_")
    so = os.path.join(d, "libqoix_write_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.qoixwref_lz4_bound.restype = C.c_long
    L.qoixwref_lz4_bound.argtypes = [C.c_long]
    L.qoixwref_lz4_compress.restype = C.c_long
    L.qoixwref_lz4_compress.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.qoixwref_bound.restype = C.c_longlong
    L.qoixwref_bound.argtypes = [C.c_int] * 4
    L.qoixwref_encode.restype = C.c_long
    L.qoixwref_encode.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_long,
                                  C.POINTER(C.c_long)]
    return L


def bits(f):
    """a float (or 4 big-endian bytes) -> the header's bit pattern"""
    return struct.unpack(">I", f if isinstance(f, bytes) else struct.pack(">f", f))[0]


def bound(w, h, channels, colorspace=0):
    return lib().qoixwref_bound(w, h, channels, colorspace)


def lz4_bound(n):
    return lib().qoixwref_lz4_bound(n)


def lz4_compress(data):
    src = np.frombuffer(bytes(data), np.uint8)
    src = np.concatenate([src, np.zeros(1, np.uint8)])                      # (never read: keeps the pointer valid at length 0)
    out = np.zeros(lz4_bound(len(data)), np.uint8)
    n = lib().qoixwref_lz4_compress(src.ctypes.data, len(data), out.ctypes.data, out.size)
    if n < 0:
        raise ValueError(f"qoixwref_lz4_compress: {n}")
    return out[:n].tobytes()


def encode_ex(img, mode=0, colorspace=0, par=1.0, dpi=96.0):
    """img: (h, w, 3 | 4) uint8 -> (the file, lz4Size + 4 - datalen)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, ch = img.shape
    b = bound(w, h, ch, colorspace)
    if b < 0:
        raise ValueError("qoixwref: refused")
    out = np.zeros(b, np.uint8)
    diff = C.c_long(0)
    n = lib().qoixwref_encode(img.ctypes.data, w * ch, w, h, ch, colorspace, bits(par), bits(dpi), mode, out.ctypes.data, out.size, C.byref(diff))
    if n < 0:
        raise ValueError(f"qoixwref_encode refused: {n}")
    return out[:n].tobytes(), diff.value


def encode(img, mode=0, **kw):
    return encode_ex(img, mode, **kw)[0]
