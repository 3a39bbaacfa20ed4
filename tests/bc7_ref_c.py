"""ctypes binding of tests/c/bc7_ref.c (saveDDS and the live part of bc7enc16 restated serially), compiled once per process into a
temporary directory.  blocks() gives the BC7 blocks of (n, 16, 4) uint8 tiles and their traces, write_dds() the file the reference
writes for an (h, w) / (h, w, comp) uint8 image."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "bc7_ref.c")
HEADER = 148
FLAGS = ("alpha", "mode1_tried", "mode1_won", "single_colour", "degenerate_fixed", "ls_improved", "early_zero", "mean_colour_won")


class Trace(C.Structure):                                         # bc7ref_trace
    _fields_ = [("mode", C.c_int32), ("partition", C.c_int32), ("partition_iter", C.c_int32),
                ("lo", C.c_int32 * 4 * 2), ("hi", C.c_int32 * 4 * 2), ("pbits", C.c_int32 * 2 * 2), ("sel", C.c_int32 * 16),
                ("error", C.c_uint64)] + [(f, C.c_int32) for f in FLAGS]


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="bc7_ref_")
    so = os.path.join(d, "libbc7_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.bc7ref_block.restype = None
    L.bc7ref_block.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Trace)]
    L.bc7ref_blocks.restype = None
    L.bc7ref_blocks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bc7ref_dds_size.restype = C.c_int64
    L.bc7ref_dds_size.argtypes = [C.c_int, C.c_int]
    L.bc7ref_write_dds.restype = None
    L.bc7ref_write_dds.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.bc7ref_table.restype = None
    L.bc7ref_table.argtypes = [C.c_void_p]
    L.bc7ref_weight_tables.restype = None
    L.bc7ref_weight_tables.argtypes = [C.c_void_p, C.c_void_p]
    return L


def block(tile):
    """16 rgba pixels -> (the 16 bytes, the Trace)"""
    tile = np.ascontiguousarray(tile, np.uint8).reshape(64)
    out = np.zeros(16, np.uint8)
    t = Trace()
    lib().bc7ref_block(tile.ctypes.data, out.ctypes.data, C.byref(t))
    return out.tobytes(), t


def blocks(tiles):
    """(n, 16, 4) uint8 -> ((n, 16) uint8, a ctypes array of n Trace)"""
    tiles = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 64)
    n = tiles.shape[0]
    out = np.zeros((n, 16), np.uint8)
    traces = (Trace * max(n, 1))()
    lib().bc7ref_blocks(tiles.ctypes.data, n, out.ctypes.data, C.addressof(traces))
    return out, traces


def dds_size(w, h):
    return int(lib().bc7ref_dds_size(w, h))


def write_dds(img):
    """(h, w) or (h, w, comp) uint8, rows of any (also negative) stride -> the file as bytes"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, comp = img.shape
    assert (comp == 1 or img.strides[2] == 1) and (w == 1 or img.strides[1] == comp)
    out = np.zeros(dds_size(w, h), np.uint8)
    lib().bc7ref_write_dds(img.ctypes.data, img.strides[0], w, h, comp, out.ctypes.data)
    return out.tobytes()


def table():
    """the computed g_bc7_mode_1_optimal_endpoints as (256, 2, 3) int32: err, lo, hi"""
    t = np.zeros((256, 2, 3), np.int32)
    lib().bc7ref_table(t.ctypes.data)
    return t


def weight_tables():
    wx3, wx4 = np.zeros((8, 4), np.float32), np.zeros((16, 4), np.float32)
    lib().bc7ref_weight_tables(wx3.ctypes.data, wx4.ctypes.data)
    return wx3, wx4
