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


def _dc_category_16(blob):
    """the file with the value 11 of its first DC table -- a category only a DC difference of 1024 or more uses: none in smooth content -- replaced by 16: the
    same image, but a table the kernels are not given (the host feeder decodes the file behind the device pass)"""
    out = bytearray(blob)
    p = 2
    while out[p + 1] != 0xDA:
        n = (out[p + 2] << 8) | out[p + 3]
        if out[p + 1] == 0xC4:
            q = p + 4
            while q < p + 2 + n:
                count = sum(out[q + 1:q + 17])
                if out[q] >> 4 == 0:
                    k = out.index(11, q + 17, q + 17 + count)
                    out[k] = 16
                    return bytes(out)
                q += 17 + count
        p += 2 + n
    raise AssertionError("no DC table")


def _stage_files():
    """one small file of every class the batch call tells apart -> [(name, bytes)]; the classes are checked below through gamut_hip_jpeg_scan_layout"""
    import io
    from PIL import Image
    import gen
    rng = np.random.default_rng(77)

    def jpeg(px, **kw):
        bio = io.BytesIO(); Image.fromarray(px).save(bio, "JPEG", **kw)
        return bio.getvalue()
    smooth = gen.synth_rgb(96, 64, 5)
    return [("420 long", B.token_files(128, 40)[0]),
            ("444 long", jpeg(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), quality=95, subsampling=0)),
            ("restart short", jpeg(smooth, quality=90, subsampling=2, restart_marker_blocks=2)),
            ("restart long", jpeg(rng.integers(0, 256, (64, 128, 3), dtype=np.uint8), quality=95, subsampling=2, restart_marker_rows=1)),
            ("dc category 16", _dc_category_16(jpeg(smooth, quality=90, subsampling=0))),
            ("progressive", jpeg(gen.synth_rgb(67, 45, 6), quality=85, subsampling=2, progressive=True)),
            ("broken header", jpeg(smooth, quality=90)[:150])]


def test_one_batch_of_every_class_across_two_groups(hip):
    """ONE gamut_hip_jpeg_decode_batch_device call over 133 files -- 19 repeats, interleaved, of the seven files of _stage_files: two groups of files, the second
    on a side stream -- with one file of every class the call tells apart: 4:2:0 with one scan of >= 4096 bytes (tokens), 4:4:4 with one of >= 4096 bytes
    (dense, a workgroup), restart intervals of a few dozen bytes (unstuffed on the host, a lane each), restart intervals of >= 1024 bytes (unstuffed on
    the device), a DC table with category 16 (the host feeder's, behind the device pass), a progressive file, a file that ends in its headers.  Every decodable
    image == the oracle's, status_host and the return code are what the oracle's verdicts give, every byte of the allocation outside the images (gaps, the
    slots of the files that fail, a guard on both sides) is untouched -- and the same call, made again on the same thread right after a smaller batch of
    other files, gives the same bytes (the thread's staging is reused)."""
    kinds = _stage_files()
    layout = {}
    for name, blob in kinds:
        buf = np.frombuffer(blob, np.uint8)
        fr = _capi.JpegFrame(); seg = C.c_int32(); nbytes = C.c_uint64()
        rc = hip.gamut_hip_jpeg_scan_layout(buf.ctypes.data, buf.size, C.byref(fr), C.byref(seg), C.byref(nbytes))
        layout[name] = (rc, seg.value, nbytes.value, fr.scan_type)
    assert layout["420 long"][0] == 0 and layout["420 long"][1] == 1 and layout["420 long"][2] - 64 >= 4096 and layout["420 long"][3] == O.JPGD_YH2V2
    assert layout["444 long"][0] == 0 and layout["444 long"][1] == 1 and layout["444 long"][2] - 64 >= 4096 and layout["444 long"][3] == O.JPGD_YH1V1
    rc, segs, nb, _ = layout["restart short"]
    assert rc == 0 and segs > 1 and len(dict(kinds)["restart short"]) < 1024 * segs
    rc, segs, nb, _ = layout["restart long"]
    assert rc == 0 and segs > 1 and nb - 64 * segs >= 1024 * segs
    assert layout["dc category 16"][0] != 0                   # no segments for the kernels: the header walk leaves the file to the host feeder ...
    want = [O.decompress_jpeg(blob, 4) for _, blob in kinds]
    assert [w is not None for w in want] == [True, True, True, True, True, True, False]           # ... which decodes it, like the oracle

    def call(order):
        """-> (rc, status_host, the whole allocation, the expected allocation)"""
        n = len(order)
        blobs = [kinds[k][1] for k in order]
        bufs = [np.frombuffer(b, np.uint8) for b in blobs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_size_t * n)(*[len(b) for b in blobs])
        size = [want[k][0].size if want[k] is not None else 96 for k in order]              # (a slot for the files that fail too: it stays as it is)
        steps = [(s + 127) // 128 * 128 + 128 * (i % 3) for i, s in enumerate(size)]
        offs = np.concatenate([[0], np.cumsum(steps)[:-1]]).astype(np.int64)
        total = 2 * B.GUARD + int(sum(steps))
        exp = np.full(total, 0xA5, np.uint8)
        for i, k in enumerate(order):
            if want[k] is not None:
                exp[B.GUARD + offs[i]:B.GUARD + offs[i] + size[i]] = want[k][0].reshape(-1)
        d_out = _DeviceBuffer(hip, total)
        try:
            d_out.upload(np.full(total, 0xA5, np.uint8))
            info = (_capi.JpegFrame * n)(); hst = (C.c_int * n)()
            rc = hip.gamut_hip_jpeg_decode_batch_device(ptrs, lens, n, 4, offs.ctypes.data_as(C.POINTER(C.c_int64)), d_out.ptr + B.GUARD, info, hst, None, None)
            _capi.check(hip.gamut_hip_stream_synchronize(None))
            return rc, list(hst), d_out.download(total), exp, offs
        finally:
            d_out.free()

    order = [i % 7 for i in range(133)]
    rc, hst, got, exp, offs = call(order)
    for i, k in enumerate(order):
        assert (hst[i] == 0) == (want[k] is not None), (i, kinds[k][0], hst[i])
    assert rc == hst[6] != 0, (rc, hst[:7])                    # the return code: the verdict of the lowest-numbered file that fails
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0]) - B.GUARD
        i = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError(f"allocation byte {at}: file {i} ({kinds[order[i]][0] if i >= 0 else 'the guard'}) at {int(offs[i])}: got {got[at + B.GUARD:at + B.GUARD + 8].tolist()}")
    small = [5, 3, 0, 2, 6, 1, 4, 3, 2]
    rc_s, hst_s, got_s, exp_s, _ = call(small)
    assert rc_s != 0 and [h == 0 for h in hst_s] == [want[k] is not None for k in small] and np.array_equal(got_s, exp_s)
    rc2, hst2, got2, _, _ = call(order)
    assert (rc2, hst2) == (rc, hst) and np.array_equal(got2, got)
