"""GPU parity of every QOI stream of tests/qoi_cases.py -- the 82 constructed ones, each named for the boundary it crosses, and the 40 arbitrary
ones -- on every QOI decode kernel (qoi.hip): k_qoi_decode<1> (one wave per stream: launches of at least Q.WIDE_BELOW resident streams),
k_qoi_decode<4> and k_qoi_pipe (smaller launches, GAMUT_HIP_QOI_PIPE = 0 / 1), at output channels 0, 3 and 4, through the entry points the
library has.  The launches are laid out by tests/qoi_batch.py (streams at every alignment with hostile bytes between them, outputs at every
residue mod 16 with gaps between them); every test compares the WHOLE output allocation with the layout's expected_allocation(): the oracle's
pixels, and 0x5A in every gap and behind the last image.  A failure names the case, not an index."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import qoi_batch as B
import qoi_cases as Q
from gamut_amd import _capi

pytestmark = pytest.mark.gpu

resident_layout = functools.lru_cache(maxsize=None)(B.resident)
threshold_layout = functools.lru_cache(maxsize=None)(B.threshold)


@contextlib.contextmanager
def forced(kernel):
    """GAMUT_HIP_QOI_PIPE for the launches inside ("pipeline": 1, "phases": 0, "one_wave": left alone -- the stream count decides), put back afterwards"""
    old = os.environ.get("GAMUT_HIP_QOI_PIPE")
    if kernel != "one_wave":
        os.environ["GAMUT_HIP_QOI_PIPE"] = "1" if kernel == "pipeline" else "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GAMUT_HIP_QOI_PIPE", None)
        else:
            os.environ["GAMUT_HIP_QOI_PIPE"] = old


@pytest.fixture(params=["pipeline", "phases"])
def small_batch_kernel(request):
    """k_qoi_pipe or k_qoi_decode<4> for launches below Q.WIDE_BELOW streams (as in test_qoi_gpu.py)"""
    with forced(request.param):
        yield request.param


def the_kernel_is(kernel, n):
    """which kernel a launch of n streams runs is decided by n and GAMUT_HIP_QOI_PIPE (gamut_hip_qoi_decode_resident_device): a changed threshold fails here"""
    assert (n >= Q.WIDE_BELOW) == (kernel == "one_wave"), (kernel, n, Q.WIDE_BELOW)


def device_buffer(hip, nbytes):
    p = hip.gamut_hip_device_malloc(nbytes)
    assert p, hip.gamut_hip_last_error()
    return p


def poison(hip, L, out_d):
    _capi.check(hip.gamut_hip_memcpy_h2d(out_d, B.pointer(L, "poison", C.c_uint8), L.out_len, None))
    _capi.check(hip.gamut_hip_stream_synchronize(None))


def download(hip, L, out_d):
    got = np.empty(L.out_len, np.uint8)
    _capi.check(hip.gamut_hip_memcpy_d2h(got.ctypes.data, out_d, got.nbytes, None))
    _capi.check(hip.gamut_hip_stream_synchronize(None))
    return got


def same(L, got, what=""):
    d = L.first_difference(got)
    assert d is None, f"{what}: {d.text}"


class Resident:
    """a ResidentLayout's blob and output allocation on the device, for as many launches as the test wants"""

    def __init__(self, hip, L):
        self.hip, self.L = hip, L
        L.fill_descs(hip.gamut_hip_qoi_read_header, _capi.QoiDesc)
        self.blob_d, self.out_d = device_buffer(hip, L.blob_len), device_buffer(hip, L.out_len)
        _capi.check(hip.gamut_hip_memcpy_h2d(self.blob_d, B.pointer(L, "blob", C.c_uint8), L.blob_len, None))
        _capi.check(hip.gamut_hip_stream_synchronize(None))
        poison(hip, L, self.out_d)

    def decode(self):
        L = self.L
        _capi.check(self.hip.gamut_hip_qoi_decode_resident_device(self.blob_d, L.blob_len, B.pointer(L, "begin", C.c_int64), B.pointer(L, "size", C.c_int),
                                                                  B.pointer(L, "descs_read", _capi.QoiDesc), L.n, L.channels, B.pointer(L, "out_offset", C.c_int64), self.out_d, None))
        return download(self.hip, L, self.out_d)

    def free(self):
        self.hip.gamut_hip_device_free(self.blob_d); self.hip.gamut_hip_device_free(self.out_d)


def decode_resident(hip, L, what):
    r = Resident(hip, L)
    try:
        same(L, r.decode(), what)
    finally:
        r.free()


def decode_from_host(hip, L, what):
    out_d = device_buffer(hip, L.out_len)
    try:
        poison(hip, L, out_d)
        rc = hip.gamut_hip_qoi_decode_batch_device(B.pointer(L, "ptrs", C.c_void_p), B.pointer(L, "size", C.c_int), L.n, L.channels, B.pointer(L, "out_offset", C.c_int64), out_d,
                                                   B.pointer(L, "descs_read", _capi.QoiDesc), B.pointer(L, "status", C.c_int), None)
        assert rc == 0, hip.gamut_hip_last_error()
        assert not L.status.any(), [L.streams[i].case.name for i in np.flatnonzero(L.status)]
        for i, s in enumerate(L.streams):
            assert (L.descs_read[i]["width"], L.descs_read[i]["height"], L.descs_read[i]["channels"]) == Q.header(s.case.data), s.case.name
        same(L, download(hip, L, out_d), what)
    finally:
        hip.gamut_hip_device_free(out_d)


@pytest.mark.parametrize("channels", (0, 3, 4))
@pytest.mark.parametrize("kernel", ("one_wave", "phases", "pipeline"))
def test_every_case_resident(hip, kernel, channels):
    """all 122 cases in ONE launch of each kernel: seven copies of the list for the one-wave kernel (854 streams), one copy for the other two"""
    L = resident_layout("one_wave" if kernel == "one_wave" else "phases", channels)          # (the two small-batch kernels get the same layout)
    assert L.n == (854 if kernel == "one_wave" else 122) and {s.case.name for s in L.streams} == set(Q.BY_NAME)
    the_kernel_is(kernel, L.n)
    with forced(kernel):
        decode_resident(hip, L, f"{kernel}, channels {channels}")


def test_both_sides_of_the_wide_threshold(hip):
    """Q.WIDE_BELOW - 1 streams are the largest launch of the small-batch kernels -- more workgroups than the part has compute units, two or more to
    a compute unit -- and Q.WIDE_BELOW the smallest of the one-wave kernel"""
    for channels in (4, 3):
        below, at = threshold_layout(Q.WIDE_BELOW - 1, channels), threshold_layout(Q.WIDE_BELOW, channels)
        assert (below.n, at.n) == (Q.WIDE_BELOW - 1, Q.WIDE_BELOW) and below.streams == at.streams[:-1]
        for kernel in ("pipeline", "phases"):
            the_kernel_is(kernel, below.n)
            with forced(kernel):
                decode_resident(hip, below, f"{below.n} streams, {kernel}, channels {channels}")
        the_kernel_is("one_wave", at.n)
        for kernel in ("pipeline", "phases"):                  # (whatever the variable says: from Q.WIDE_BELOW streams on it is not asked)
            with forced(kernel):
                decode_resident(hip, at, f"{at.n} streams, GAMUT_HIP_QOI_PIPE as for {kernel}, channels {channels}")


def test_constructed_cases_from_host_memory(hip, small_batch_kernel):
    """gamut_hip_qoi_decode_batch_device: every case in one call -- at most Q.HOST_GROUP streams, one launch -- and three times every case: two
    launches, each behind its own upload"""
    for channels in (0, 3):
        one, three = B.host(1, channels), B.host(3, channels)
        assert one.n == len(Q.CASES) <= Q.HOST_GROUP < three.n <= 2 * Q.HOST_GROUP < 2 * Q.WIDE_BELOW
        decode_from_host(hip, one, f"{one.n} files, {small_batch_kernel}, channels {channels}")
        decode_from_host(hip, three, f"{three.n} files, {small_batch_kernel}, channels {channels}")


def test_each_constructed_case_alone(hip, small_batch_kernel):
    """a launch of one workgroup has no neighbour to hide behind: every constructed case as a batch of one (rgba out), and one case of each family
    through the drop-in gamut_hip_qoi_decode at every channel count"""
    for c in Q.CONSTRUCTED:
        decode_from_host(hip, B.alone(c), f"alone, {small_batch_kernel}")
    for c in B.drop_in_cases():
        data = np.frombuffer(c.data, np.uint8)
        for channels in (0, 3, 4):
            exp = Q.expected(c.name, channels)
            d = _capi.QoiDesc()
            p = hip.gamut_hip_qoi_decode(data.ctypes.data, data.size, C.byref(d), channels)
            assert p, (c.name, hip.gamut_hip_last_error())
            got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (exp.size,)).copy()
            O._libc.free(C.c_void_p(p))
            assert (d.width, d.height, d.channels) == Q.header(c.data), c.name
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"{c.name}, drop-in, {small_batch_kernel}, channels {channels}: {bad.size} bytes differ, the first at {int(bad[0])} of {exp.size}"


def test_the_same_streams_give_the_same_pixels_twice(hip):
    """the one-wave launch twice into the same allocation, then once more into a poisoned one: the LDS pixel buffer and the item table's per-thread
    slots (four, taken in turn: the third call is on its third) carry nothing from one call to the next"""
    L = resident_layout("one_wave", 3)
    the_kernel_is("one_wave", L.n)
    r = Resident(hip, L)
    try:
        same(L, r.decode(), "first call")
        same(L, r.decode(), "second call, over the first one's pixels")
        poison(hip, L, r.out_d)
        same(L, r.decode(), "third call")
    finally:
        r.free()
