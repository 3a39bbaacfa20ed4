"""ctypes binding of tests/c/sqz_ref.c (SQZ_decode restated serially in two callable steps, and SQZ_encode to make test files), compiled
once per process into a temporary directory.  header() gives the verdict and the fields, coeffs() the coefficient stage, pixels() the
pixel stage, load() both, encode() a file."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "sqz_ref.c")
INFO_FIELDS = ("width", "height", "planes", "color_mode", "levels", "scan_order", "subsampling", "pixel_type", "detected")
OK, REFUSED = 0, 1
GREY, YCOCG, OKLAB, LOGL1 = range(4)
RASTER, SNAKE, MORTON, HILBERT = range(4)


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="sqz_ref_")
    so = os.path.join(d, "libsqz_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.sqzref_header.restype = C.c_long
    L.sqzref_header.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    L.sqzref_coeffs.restype = C.c_long
    L.sqzref_coeffs.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.sqzref_pixels.restype = C.c_long
    L.sqzref_pixels.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.sqzref_encode.restype = C.c_long
    L.sqzref_encode.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    L.sqzref_scan.restype = C.c_long
    L.sqzref_scan.argtypes = [C.c_int, C.c_long, C.c_long, C.c_void_p]
    L.sqzref_tables.argtypes = [C.c_void_p, C.c_void_p]
    assert L.sqzref_selftest() == 1
    return L


def _buf(data):
    return np.frombuffer(bytes(data) + b"\0", np.uint8)


def header(data):
    """-> (verdict: OK / REFUSED, dict of INFO_FIELDS; all zero but `detected` when refused)"""
    buf = _buf(data)
    info = np.zeros(9, np.int32)
    v = lib().sqzref_header(buf.ctypes.data, len(data), info.ctypes.data)
    return int(v), {k: int(x) for k, x in zip(INFO_FIELDS, info)}


def coeffs(data):
    """-> None when the file is refused, else (int16 array of planes * h * w sign-magnitude coefficients, info)"""
    rc, info = header(data)
    if rc != OK:
        return None
    buf = _buf(data)
    out = np.zeros(info["planes"] * info["height"] * info["width"], np.int16)
    assert lib().sqzref_coeffs(buf.ctypes.data, len(data), out.ctypes.data, out.size) == 0
    return out, info


def pixels(co, w, h, mode, levels):
    """coefficient planes (left unchanged) -> (h, w, planes) uint8"""
    co = np.ascontiguousarray(co, np.int16)
    planes = 1 if mode == GREY else 3
    assert co.size == planes * w * h
    out = np.zeros((h, w, planes), np.uint8)
    assert lib().sqzref_pixels(co.ctypes.data, w, h, mode, levels, out.ctypes.data) == 0
    return out


def load(data):
    """-> None when the file is refused, else (pixels (h, w, planes) uint8, info)"""
    c = coeffs(data)
    if c is None:
        return None
    co, info = c
    return pixels(co, info["width"], info["height"], info["color_mode"], info["levels"]), info


def encode(px, mode, levels, scan=SNAKE, subsampling=0, budget=None):
    """px: (h, w) or (h, w, 3) uint8 -> the file as bytes, cut at `budget` bytes (default: enough for a lossless stream)"""
    px = np.ascontiguousarray(px, np.uint8)
    h, w = px.shape[:2]
    assert px.size == h * w * (1 if mode == GREY else 3)
    if budget is None:
        budget = 64 + px.size * 3
    dst = np.zeros(budget + 1, np.uint8)
    n = lib().sqzref_encode(px.ctypes.data, w, h, mode, levels, scan, subsampling, dst.ctypes.data, budget)
    assert n >= 0, "sqzref_encode refused"
    return dst[:n].tobytes()


def scan(order, w, h):
    """the LIP order of a w x h subband -> (w * h, 2) array of x, y"""
    xy = np.zeros((w * h, 2), np.uint16)
    n = lib().sqzref_scan(order, w, h, xy.ctypes.data)
    return xy[:n]


def tables():
    a, b = np.zeros(256, np.uint16), np.zeros(512, np.uint8)
    lib().sqzref_tables(a.ctypes.data, b.ctypes.data)
    return a, b
