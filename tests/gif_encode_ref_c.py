"""ctypes binding of tests/c/gif_encode_ref.c (saveGIF over msf_gif restated serially), compiled once per process into a temporary
directory.  encode() gives the file and, per frame, a report of what the encoder did."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "gif_encode_ref.c")
REPORT_FIELDS = ("depth", "count", "table_bits", "resets", "sub_blocks", "last_kind", "has_transparent", "compatible")
LAST_PARTIAL, LAST_NONE_AFTER_ROLLOVER, LAST_EXACTLY_FULL = 1, 2, 3


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="gif_encode_ref_")
    so = os.path.join(d, "libgif_encode_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.gifencref_encode.restype = C.c_long
    L.gifencref_encode.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.gifencref_cook_both.restype = None
    L.gifencref_cook_both.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def bound(w, h, frames):
    return 32 + frames * (32 + 768 + w * h * 3 // 2 + 256) + 1


def encode(frames, centiseconds=7, max_bit_depth=16, alpha_threshold=10):
    """frames: (n, h, w, 4) uint8 -> (file bytes, [report dict per frame])"""
    px = np.ascontiguousarray(frames, np.uint8)
    n, h, w, c = px.shape
    assert c == 4
    out = np.zeros(bound(w, h, n) + 512, np.uint8)
    rep = np.zeros((n, 8), np.int32)
    length = lib().gifencref_encode(px.ctypes.data, w * 4, w * h * 4, w, h, n, centiseconds, max_bit_depth, alpha_threshold, out.ctypes.data, rep.ctypes.data)
    assert length > 0
    return out[:length].tobytes(), [dict(zip(REPORT_FIELDS, map(int, r))) for r in rep]


def cook_both(px, x, y, depth, alpha_threshold):
    """-> (value by the 4-pixel body's arithmetic, value by the scalar tail's)"""
    p = np.ascontiguousarray(px, np.uint8)
    v = np.zeros(2, np.uint32)
    lib().gifencref_cook_both(p.ctypes.data, x, y, depth, alpha_threshold, v.ctypes.data, v.ctypes.data + 4)
    return int(v[0]), int(v[1])
