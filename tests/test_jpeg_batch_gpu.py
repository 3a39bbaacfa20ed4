"""GPU parity of the BATCHED JPEG reconstruction launches: every kernel instantiation the two launchers of gamut_amd/csrc/jpeg.hip can start
(tests/jpeg_batch_cases.py, checked for completeness in test_jpeg_batch_cases_cpu.py), each with 17 distinct images -- two full groups of eight,
then one image and seven guarded slots -- against the CPU oracle.  Bar: the WHOLE output allocation, bit for bit: pixels, row gaps, the gaps
between images, the spare image slots behind the batch and a guard on either side."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_batch_cases as B
import oracle_lib as O
from gamut_amd import _capi

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


class _DeviceBuffer:
    """one device allocation reused by the cases of a test: every case uploads its whole image of it"""

    def __init__(self, L, nbytes):
        self.L, self.nbytes = L, nbytes
        self.ptr = L.gamut_hip_device_malloc(nbytes)
        assert self.ptr, _capi.last_error()

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _capi.check(self.L.gamut_hip_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes, None))
        _capi.check(self.L.gamut_hip_stream_synchronize(None))

    def download(self, nbytes):
        assert nbytes <= self.nbytes
        host = np.empty(nbytes, np.uint8)
        _capi.check(self.L.gamut_hip_memcpy_d2h(host.ctypes.data, self.ptr, nbytes, None))
        _capi.check(self.L.gamut_hip_stream_synchronize(None))
        return host

    def free(self):
        self.L.gamut_hip_device_free(self.ptr)


def _sizes(c):
    n = B.nblk(c)
    s = B.slots(c.count)
    return n, n * 64 + 8, n + 3, s                    # blocks, coefficient stride (int16 units: not tight, a multiple of 8), max_zag stride, image slots


@pytest.mark.parametrize("scan_type", [4, 1, 2, 3, 0])
def test_dense_batches_every_variant(hip, scan_type):
    """gamut_hip_jpeg_reconstruct_batch_device.  Per case: coefficients `nblk * 64 + 8` apart and max_zag `nblk + 3` apart, both for 8 * ceil(count / 8) image
    slots whose spare ones (and every gap, and a 4096-byte guard on both sides) hold non-zero noise; the output the same number of slots, 0xA5 all
    over.  A wrong tail guard or image index then shows as a changed byte inside the allocation.  Expected: the oracle's images placed by pitch sign
    and stride into an allocation of 0xA5, compared whole; a difference is reported as case, variant, image, row and column."""
    cases = [c for c in B.CASES if c.scan_type == scan_type]
    G = B.GUARD
    d_co = _DeviceBuffer(hip, max(G + _sizes(c)[3] * _sizes(c)[1] * 2 + G for c in cases))
    d_zz = _DeviceBuffer(hip, max(G + _sizes(c)[3] * _sizes(c)[2] + G for c in cases))
    d_out = _DeviceBuffer(hip, max(2 * G + _sizes(c)[3] * B.geometry(c)[1] for c in cases))
    rng = np.random.default_rng(900 + scan_type)
    failures, ran = [], set()
    try:
        assert d_out.ptr % 128 == 0 and d_co.ptr % 16 == 0, "the mirror assumes allocations that start on a 128-byte line"
        for c in cases:
            n, cstride, zstride, s = _sizes(c)
            pitch, stride = B.geometry(c)
            name = B.case_variant(c, d_out.ptr)
            assert name == B.case_variant(c)
            co, mz = B.inputs(c)
            hco = (rng.integers(1, 32768, G + s * cstride, dtype=np.int16) * rng.choice(np.array([-1, 1], np.int16), G + s * cstride)).astype(np.int16)
            hco[G // 2:G // 2 + s * cstride].reshape(s, cstride)[:c.count, :n * 64] = co.reshape(c.count, -1)
            d_co.upload(hco)
            if mz is not None:
                hzz = rng.integers(1, 65, 2 * G + s * zstride, dtype=np.uint8)
                hzz[G:G + s * zstride].reshape(s, zstride)[:c.count, :n] = mz
                d_zz.upload(hzz)
            total = 2 * G + s * stride
            d_out.upload(np.full(total, 0xA5, np.uint8))
            out = d_out.ptr + G + ((B.HEIGHT - 1) * pitch if c.flip else 0)          # bottom-up: the pointer is that of row 0, the image's last row in memory
            with _env("GAMUT_HIP_JPEG_COLS", c.cols_env):
                _capi.check(hip.gamut_hip_jpeg_reconstruct_batch_device(d_co.ptr + G, cstride, d_zz.ptr + G if mz is not None else None, zstride, out,
                                                                         -pitch if c.flip else pitch, stride, c.w, B.HEIGHT, scan_type, c.out_comps, c.count, None))
            _capi.check(hip.gamut_hip_stream_synchronize(None))
            got = d_out.download(total)
            bad = B.describe_difference(c, got, B.expected_allocation(c))
            if bad:
                failures.append(bad)
            ran.add(name)
    finally:
        for d in (d_co, d_zz, d_out):
            d.free()
    assert not failures, f"{len(failures)} of {len(cases)} cases differ:\n" + "\n".join(failures[:8])
    assert ran == {B.case_variant(c) for c in cases}


@pytest.fixture(params=["tokens", "dense"])
def handoff(request):
    """GAMUT_HIP_JPEG_HANDOFF: what the entropy kernels hand to the reconstruction inside gamut_hip_jpeg_decode_batch_device"""
    with _env("GAMUT_HIP_JPEG_HANDOFF", request.param):
        yield request.param


def test_file_batches_every_token_variant(hip, handoff):
    """gamut_hip_jpeg_decode_batch_device on 17 distinct Pillow-written 4:2:0 files of 128x40 and of 133x40 (quality 90; noisy content, so that each scan is
    longer than the 4096 bytes below which a file keeps the dense blocks even when tokens are asked for -- checked on the CPU in
    test_jpeg_batch_cases_cpu.py: 128x40 is large enough), rgba8 / rgb8 / l8, out_offset in equal steps on the 128-byte lines, in equal steps 4 bytes
    off them, and in steps that change from file to file (launches of two and a last one of one: jpeg_batch_cases.token_launches).  Every file ==
    O.decompress_jpeg, and the whole allocation (gaps between the images, a 4096-byte guard on both sides) == the expected one."""
    G = B.GUARD
    failures = []
    for (w, h) in B.TOKEN_SIZES:
        blobs = B.token_files(w, h)
        n = len(blobs)
        bufs = [np.frombuffer(b, np.uint8) for b in blobs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_size_t * n)(*[len(b) for b in blobs])
        for comps in (4, 3, 1):
            want = [O.decompress_jpeg(b, comps)[0] for b in blobs]
            size = w * h * comps
            for form in B.TOKEN_OFFSETS:
                offs, total = B.token_offsets(w, h, comps, form)
                d_out = _DeviceBuffer(hip, 2 * G + total)
                try:
                    assert d_out.ptr % 128 == 0
                    d_out.upload(np.full(2 * G + total, 0xA5, np.uint8))
                    info = (_capi.JpegFrame * n)(); hst = (C.c_int * n)()
                    rc = hip.gamut_hip_jpeg_decode_batch_device(ptrs, lens, n, comps, offs.ctypes.data_as(C.POINTER(C.c_int64)), d_out.ptr + G, info, hst, None, None)
                    assert rc == 0 and not any(hst), (rc, list(hst), hip.gamut_hip_last_error())
                    _capi.check(hip.gamut_hip_stream_synchronize(None))
                    got = d_out.download(2 * G + total)
                finally:
                    d_out.free()
                exp = np.full(2 * G + total, 0xA5, np.uint8)
                where = f"{handoff} {w}x{h} comps{comps} offsets {form} {B.token_variants(w, h, comps, form, handoff == 'tokens')}"
                for i in range(n):
                    assert (info[i].width, info[i].height) == (w, h)
                    exp[G + offs[i]:G + offs[i] + size] = want[i].reshape(-1)
                    mine = got[G + offs[i]:G + offs[i] + size]
                    if not np.array_equal(mine, exp[G + offs[i]:G + offs[i] + size]):
                        k = int(np.flatnonzero(mine != want[i].reshape(-1))[0])
                        failures.append(f"{where}: image {i} row {k // (w * comps)} column {k % (w * comps) // comps}")
                if not np.array_equal(got, exp):
                    k = int(np.flatnonzero(got != exp)[0])
                    failures.append(f"{where}: allocation byte {k - G} (image slots start at {offs[:4].tolist()} ...): got {got[k:k + 8].tolist()} want {exp[k:k + 8].tolist()}")
    assert not failures, f"{len(failures)} differences:\n" + "\n".join(failures[:8])
