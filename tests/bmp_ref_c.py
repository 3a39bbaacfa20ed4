"""ctypes binding of tests/c/bmp_ref.c (stbi__bmp_load and write_bmp restated serially), compiled once per process into a temporary
directory.  load() gives the reference's verdict, header fields and pixels; write() the file write_bmp produces."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "bmp_ref.c")
INFO_FIELDS = ("width", "height", "bpp", "header_size", "compression", "channels_in_file", "top_down", "pixel_offset", "palette_size",
               "mask_r", "mask_g", "mask_b", "mask_a")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="bmp_ref_")
    so = os.path.join(d, "libbmp_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.bmpref_load.restype = C.c_int
    L.bmpref_load.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.bmpref_write.restype = C.c_long
    L.bmpref_write.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def header(data, req_comp=0):
    """-> None when refused (for that req_comp: the size test is on the decoder's target), else (dict of INFO_FIELDS, (ppm_x, ppm_y, ratio))"""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    info = np.zeros(16, np.uint32); dens = np.zeros(3, np.float32)
    if not lib().bmpref_load(buf.ctypes.data, len(data), req_comp, None, 0, info.ctypes.data, dens.ctypes.data):
        return None
    return {k: int(v) for k, v in zip(INFO_FIELDS, info)}, tuple(float(x) for x in dens)


def load(data, req_comp=0):
    """-> None when refused, else (pixels (h, w, comps) uint8, info dict, densities)"""
    hd = header(data, req_comp)
    if hd is None:
        return None
    info, dens = hd
    comps = req_comp or info["channels_in_file"]
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    out = np.zeros((info["height"], info["width"], comps), np.uint8)
    i2 = np.zeros(16, np.uint32); d2 = np.zeros(3, np.float32)
    ok = lib().bmpref_load(buf.ctypes.data, len(data), req_comp, out.ctypes.data, out.size, i2.ctypes.data, d2.ctypes.data)
    assert ok
    return out, info, dens


def write(img, ppm_x=0, ppm_y=0):
    """img: (h, w, 3 | 4) uint8 -> the file as bytes, or None when saveBMP refuses the shape"""
    img = np.ascontiguousarray(img)
    h, w, comp = img.shape
    out = np.zeros(122 + h * ((w * comp + 3) & ~3) + 16, np.uint8)
    n = lib().bmpref_write(img.ctypes.data, w * comp, w, h, comp, ppm_x, ppm_y, out.ctypes.data)
    return out[:n].tobytes() if n else None


def bound(w, h, comp):
    if comp not in (3, 4) or not (1 <= w <= 32767 and 1 <= h <= 32767):
        return 0
    return 122 + h * ((w * comp + 3) & ~3)
