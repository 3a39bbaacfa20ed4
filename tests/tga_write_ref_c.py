"""ctypes binding of tests/c/tga_write_ref.c (TGAEncoder as saveTGA drives it, restated serially), compiled once per process into a
temporary directory.  encode() gives the file the reference writes for an (h, w, comp) uint8 image."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "tga_write_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="tga_write_ref_")
    so = os.path.join(d, "libtga_write_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.tgawref_encode.restype = C.c_long
    L.tgawref_encode.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return L


def encode(img, rle=True):
    """img: (h, w, comp) uint8, comp 1..4 -> the file's bytes (raises when the reference refuses)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, comp = img.shape
    fc = 3 if comp in (1, 3) else 4
    out = np.zeros(18 + w * h * (fc + 1), np.uint8)
    n = lib().tgawref_encode(img.ctypes.data, w * comp, w, h, comp, int(rle), out.ctypes.data, out.size)
    if n < 0:
        raise ValueError(f"tgawref_encode refused: {n}")
    return out[:n].tobytes()
