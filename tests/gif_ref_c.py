"""ctypes binding of tests/c/gif_ref.c (GIFDecoder + loadGIF restated serially), compiled once per process into a temporary directory.
header() gives the verdict of GIFDecoder.open and its fields, load() the composited rgba8 layers as well."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "gif_ref.c")
INFO_FIELDS = ("width", "height", "layers", "is_gif89")


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="gif_ref_")
    so = os.path.join(d, "libgif_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.gifref_load.restype = C.c_int
    L.gifref_load.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    return L


def header(data):
    """-> None when refused, else (dict of INFO_FIELDS, (pixel aspect ratio, fps) as float32)"""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    info = np.zeros(4, np.int32); f = np.zeros(2, np.float32)
    if not lib().gifref_load(buf.ctypes.data, len(data), None, 0, info.ctypes.data, f.ctypes.data):
        return None
    return {k: int(v) for k, v in zip(INFO_FIELDS, info)}, (np.float32(f[0]), np.float32(f[1]))


def load(data):
    """-> None when refused, else (pixels (layers, h, w, 4) uint8, info dict, (aspect, fps))"""
    hd = header(data)
    if hd is None:
        return None
    info, f = hd
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    out = np.zeros((info["layers"], info["height"], info["width"], 4), np.uint8)
    i2 = np.zeros(4, np.int32); f2 = np.zeros(2, np.float32)
    ok = lib().gifref_load(buf.ctypes.data, len(data), out.ctypes.data if out.size else np.zeros(1, np.uint8).ctypes.data, out.size, i2.ctypes.data, f2.ctypes.data)
    assert ok
    return out, info, f
