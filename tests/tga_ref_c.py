"""ctypes binding of tests/c/tga_ref.c (TGADecoder.getImageInfo / decodeImage restated serially), compiled once per process into a
temporary directory.  header() gives the reference's two verdicts and its header fields, load() the pixels."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "tga_ref.c")
INFO_FIELDS = ("width", "height", "bpp", "image_type", "rle", "indexed", "rgb16", "channels_in_file", "bottom_up", "palette_start",
               "palette_len", "cmap_size", "data_offset", "detected")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="tga_ref_")
    so = os.path.join(d, "libtga_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.tgaref_load.restype = C.c_int
    L.tgaref_load.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    return L


def header(data):
    """-> (detected, loadable, dict of INFO_FIELDS as far as the header was read)"""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    info = np.zeros(16, np.int32)
    v = lib().tgaref_load(buf.ctypes.data, len(data), 0, None, 0, info.ctypes.data)
    return bool(v & 1), bool(v & 2), {k: int(x) for k, x in zip(INFO_FIELDS, info)}


def load(data, req_comp=0):
    """-> None when the load is refused (header or stream), else (pixels (h, w, comps) uint8, info dict)"""
    det, ok, info = header(data)
    if not ok:
        return None
    comps = req_comp or info["channels_in_file"]
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    out = np.zeros((info["height"], info["width"], comps), np.uint8)
    i2 = np.zeros(16, np.int32)
    v = lib().tgaref_load(buf.ctypes.data, len(data), req_comp, out.ctypes.data, out.size, i2.ctypes.data)
    return (out, info) if v & 4 else None
