"""ctypes binding of tests/c/sqz_ref_fwd.c (the forward steps of tests/c/sqz_ref.c's encoder on their own), compiled once per process
into a temporary directory, as tests/sqz_ref_c.py binds the original.  analyze() is colour transform + DWT + sign-magnitude from
pixels, forward() the same from int16 planes."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "sqz_ref_fwd.c")
GREY = 0


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="sqz_ref_fwd_")
    so = os.path.join(d, "libsqz_ref_fwd.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.sqzref_analyze.restype = C.c_long
    L.sqzref_analyze.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.sqzref_forward.restype = C.c_long
    L.sqzref_forward.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    assert L.sqzref_selftest() == 1
    return L


def clamp_levels(w, h, levels):
    return min(levels, min(int(min(w, h)).bit_length() - 3, 8))


def analyze(px, mode, levels):
    """px: (h, w) or (h, w, 3) uint8 -> planes * h * w sign-magnitude int16; levels is clamped as SQZ_validate_input clamps it"""
    px = np.ascontiguousarray(px, np.uint8)
    h, w = px.shape[:2]
    planes = 1 if mode == GREY else 3
    assert px.size == h * w * planes
    out = np.zeros(planes * h * w, np.int16)
    assert lib().sqzref_analyze(px.ctypes.data, w, h, mode, clamp_levels(w, h, levels), out.ctypes.data) == 0
    return out


def forward(planes_in, w, h, levels):
    """two's-complement int16 planes in raster order -> sign-magnitude coefficients"""
    p = np.ascontiguousarray(planes_in, np.int16).reshape(-1)
    assert p.size % (w * h) == 0
    out = np.zeros(p.size, np.int16)
    assert lib().sqzref_forward(p.ctypes.data, w, h, p.size // (w * h), clamp_levels(w, h, levels), out.ctypes.data) == 0
    return out
