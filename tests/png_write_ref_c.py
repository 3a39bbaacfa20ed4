"""ctypes binding of tests/c/png_write_ref.c (the reference's PNG writer around its compressor, restated serially), compiled once per
process into a temporary directory.  filt() is the buffer the reference hands to its compressor, file_around() the complete file it
writes around a given zlib payload, split() takes a file apart again."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "png_write_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="png_write_ref_")
    so = os.path.join(d, "libpng_write_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.pwr_filt.restype = C.c_long
    L.pwr_filt.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.pwr_file.restype = C.c_long
    L.pwr_file.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    return L


def geometry(img):
    """img: (h, w, comp) uint8 or uint16 -> (h, w, comp, is16)"""
    h, w, comp = img.shape
    return h, w, comp, int(img.dtype.itemsize == 2)


def filt(img, force_filter=-1):
    """img: (h, w, comp) uint8 / uint16 (native byte order), rows contiguous -> the filtered stream as bytes"""
    img = np.ascontiguousarray(img)
    h, w, comp, is16 = geometry(img)
    lb = w * comp * (2 if is16 else 1)
    out = np.empty((lb + 1) * h, np.uint8)
    n = lib().pwr_filt(img.ctypes.data, lb, w, h, comp, is16, force_filter, out.ctypes.data)
    assert n == out.size, n
    return out.tobytes()


def file_around(w, h, comp, is16, payload):
    """the complete PNG file the reference writes around the zlib stream `payload`"""
    buf = np.frombuffer(bytes(payload), np.uint8)
    out = np.empty(57 + buf.size, np.uint8)
    n = lib().pwr_file(w, h, comp, is16, buf.ctypes.data, buf.size, out.ctypes.data)
    assert n == out.size, n
    return out.tobytes()


def encode(img, force_filter=-1, level=6):
    h, w, comp, is16 = geometry(img)
    return file_around(w, h, comp, is16, zlib.compress(filt(img, force_filter), level))


def split(data):
    """a file of the reference's shape (signature, IHDR, one IDAT, IEND) -> the IDAT payload; asserts the shape"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[37:41] == b"IDAT", data[:48]
    (zlen,) = struct.unpack(">I", data[33:37])
    assert len(data) == 57 + zlen, (len(data), zlen)
    return data[41:41 + zlen]


BLOCK = 8192


def bound(w, h, comp, is16):
    """include/gamut_hip.h: container 57 + zlib 6 + the filtered stream in stored blocks of 8192"""
    L = (w * comp * (2 if is16 else 1) + 1) * h
    return 57 + 6 + L + 5 * (-(-L // BLOCK))
