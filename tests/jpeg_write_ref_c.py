"""ctypes binding of tests/c/jpeg_write_ref.c, compiled once per process into a temporary directory with
gcc -O2 -ffp-contract=off -fno-fast-math (every float operation rounded on its own, x86-64 SSE)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "jpeg_write_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="jpeg_write_ref_")
    so = os.path.join(d, "libjpeg_write_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC",
                           SRC, "-o", so])
    L = C.CDLL(so)
    L.jwr_encode.restype = C.c_long
    L.jwr_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_long]
    return L


def bound(w, h, quality):
    q = quality or 90
    blocks = 6 * (-(-w // 16)) * (-(-h // 16)) if q <= 90 else 3 * (-(-w // 8)) * (-(-h // 8))
    return 607 + 2 * ((blocks * 1660 + 7) // 8) + 2


def encode(img, quality=90, comp=None):
    """img: (h, w) or (h, w, comp) uint8 (any strides: rows are passed with their own pitch) -> the stream as bytes"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    comp = comp or c
    if img.strides[1] != comp or img.strides[2] != 1:
        img = np.ascontiguousarray(img)
    out = np.empty(bound(w, h, quality), np.uint8)
    n = lib().jwr_encode(img.ctypes.data, w, h, comp, img.strides[0], quality, out.ctypes.data, out.size)
    assert n > 0, n
    return out[:n].tobytes()
