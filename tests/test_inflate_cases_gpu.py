"""GPU parity of the inflate kernel (gamut_amd/csrc/inflate.hip) on the constructed streams of tests/inflate_cases.py -- what RFC 1951 allows and
zlib's encoder never writes: == zlib, byte for byte and verdict for verdict, with zlib asked at test time.  Good and corrupt streams share a batch; every
good stream again at capacities that end in it; the long ones again through the sliced entry; the batch again, and reversed; four of them as the IDAT of PNG
files through the file batch.  tests/test_inflate_cases_cpu.py shows, without a GPU, which line of the kernel each case reaches."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
from inflate_corpus import _inflate_device, zlib_inflate as _zlib

pytestmark = pytest.mark.gpu


def _batch():
    """every case, good and corrupt ones in turn as far as they go -> (cases, what zlib makes of each)"""
    good = [c for c in IC.cases() if c.status is None]
    bad = [c for c in IC.cases() if c.status is not None]
    order = []
    for k in range(max(len(good), len(bad))):
        order += good[k:k + 1] + bad[k % len(bad):k % len(bad) + 1]          # (the corrupt ones come round again: a corrupt neighbour for every good stream)
    return order, [_zlib(c.data) for c in order]


def _check(cases, want, caps, outs, st, where=""):
    failures = []
    for c, exp, cap, got, s in zip(cases, want, caps, outs, st):
        if exp is None:
            assert c.status is not None, c.name
            if s == 0 or (c.status != IC.ANY and s != c.status):
                failures.append(f"{c.name}{where}: zlib turns it away, status {s}, expected {'non-zero' if c.status == IC.ANY else c.status}")
        else:
            assert c.status is None, c.name
            if s != 0:
                failures.append(f"{c.name}{where}: status {s} on a good stream (capacity {cap} of {len(exp)})")
            elif got != exp[:cap]:
                diff = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), None)
                failures.append(f"{c.name}{where}: {len(got)} bytes, expected {min(cap, len(exp))}; first difference at {diff} (capacity {cap})")
    assert not failures, f"{len(failures)} of {len(cases)} streams:\n" + "\n".join(failures[:12])


def _caps(cases, want):
    return [len(e) + 7 if e is not None else 4096 for e in want]


def test_every_case_in_one_batch_good_and_corrupt_side_by_side(hip):
    cases, want = _batch()
    caps = _caps(cases, want)
    rc, outs, st = _inflate_device(hip, [c.data for c in cases], caps)
    assert rc == 0, hip.gamut_hip_last_error()
    _check(cases, want, caps, outs, st)


def test_every_good_case_at_capacities_that_end_inside_it(hip):
    """the whole stream, one byte less, one byte, none -- and for streams of more than a tile a capacity inside a tile: status 0, the prefix, the guard behind it
    untouched (_inflate_device checks the 0xA5 bytes behind every capacity)"""
    cases, want, caps = [], [], []
    for c in IC.cases():
        if c.status is not None:
            continue
        exp = _zlib(c.data)
        assert exp is not None, c.name
        n = len(exp)
        for cap in [n, max(n - 1, 0), 1, 0] + ([IC.TILE_BYTES + n % 9973 % IC.TILE_BYTES] if n > 2 * IC.TILE_BYTES else []):
            cases.append(c); want.append(exp); caps.append(cap)
    rc, outs, st = _inflate_device(hip, [c.data for c in cases], caps)
    assert rc == 0, hip.gamut_hip_last_error()
    _check(cases, want, caps, outs, st)


def test_long_cases_in_slices_equal_one_launch(hip):
    """gamut_hip_inflate_batch_device_sliced on every case that is long enough to suspend: slices just above the smallest span that lets a stream stop
    (kRoundBytes + 64), a little more, and two rounds -- the block of 1-15 bit codes resumes from InfState.lens, a stream waits in front of a 65 535-byte stored
    block, the streams that never resynchronise stop between their rounds"""
    cases = [c for c in IC.cases() if len(c.data) > IC.SLICE_MIN]
    assert any(c.name.startswith("long codes, three rounds") for c in cases) and len(cases) > 30
    want = [_zlib(c.data) for c in cases]
    caps = _caps(cases, want)
    streams = [c.data for c in cases]
    rc, outs0, st0 = _inflate_device(hip, streams, caps)
    assert rc == 0, hip.gamut_hip_last_error()
    _check(cases, want, caps, outs0, st0)
    for slice_bytes in (33_000, 40_000, 70_000):
        rc, outs, st = _inflate_device(hip, streams, caps, slice_bytes)
        assert rc == 0, hip.gamut_hip_last_error()
        _check(cases, want, caps, outs, st, f" in slices of {slice_bytes}")
        assert [int(s) for s in st] == [int(s) for s in st0]


def test_the_batch_again_and_reversed(hip):
    """the token lists and their busy flags are reused from call to call: the same batch twice, then back to front"""
    cases, want = _batch()
    caps = _caps(cases, want)
    for turn in range(2):
        rc, outs, st = _inflate_device(hip, [c.data for c in cases], caps)
        assert rc == 0, hip.gamut_hip_last_error()
        _check(cases, want, caps, outs, st, f" (call {turn + 1})")
    cases, want, caps = cases[::-1], want[::-1], caps[::-1]
    rc, outs, st = _inflate_device(hip, [c.data for c in cases], caps)
    assert rc == 0, hip.gamut_hip_last_error()
    _check(cases, want, caps, outs, st, " (reversed)")


def _png(stream, raw):
    """a one-row 8-bit grey PNG whose IDAT is `stream` behind a zlib header: `raw` = filter byte 0 and the row"""
    assert raw[0] == 0

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))
    idat = b"\x78\x01" + stream + struct.pack(">I", zlib.adler32(raw))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", len(raw) - 1, 1, 8, 0, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def test_constructed_streams_as_png_files(hip):
    """the long codes, the 2 212-bit code-length stream and a stream that never resynchronises (two phases: one of them is out of step with every lane) as the IDAT of
    valid PNG files: the file batch with the inflate on the device == the file batch with zlib on the host == the row itself"""
    from gamut_amd import _capi
    names = ("long codes", "code lengths: 2 212 bits, all single", "never resynchronises: 2-bit codes, phase 0", "never resynchronises: 2-bit codes, phase 1")
    raws = [IC.by_name(n).expect for n in names]
    files = [_png(IC.by_name(n).data, raw) for n, raw in zip(names, raws)]
    n = len(files)
    offs = np.zeros(n, np.int64)
    for i in range(1, n):
        offs[i] = (offs[i - 1] + len(raws[i - 1]) - 1 + 255) // 256 * 256
    span = int(offs[-1]) + len(raws[-1]) - 1
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
    got = {}
    old = os.environ.get("GAMUT_HIP_PNG_INFLATE")
    try:
        for mode in ("host", "device"):
            os.environ["GAMUT_HIP_PNG_INFLATE"] = mode
            d_out = hip.gamut_hip_device_malloc(span + 256)
            assert d_out
            try:
                poison = np.full(span + 256, 0xA5, np.uint8)
                _capi.check(hip.gamut_hip_memcpy_h2d(d_out, poison.ctypes.data, poison.size, None))
                _capi.check(hip.gamut_hip_stream_synchronize(None))
                info = (_capi.PngInfo * n)(); st = (C.c_int * n)()
                rc = hip.gamut_hip_png_decode_batch_device(ptrs, lens, n, 1, 8, offs.ctypes.data_as(C.POINTER(C.c_int64)), d_out, info, st, 3, None)
                assert rc == 0 and not any(st), (mode, rc, list(st), hip.gamut_hip_last_error())
                _capi.check(hip.gamut_hip_stream_synchronize(None))
                host = np.empty(span + 256, np.uint8)
                _capi.check(hip.gamut_hip_memcpy_d2h(host.ctypes.data, d_out, host.size, None))
                _capi.check(hip.gamut_hip_stream_synchronize(None))
                got[mode] = host
                for i in range(n):
                    assert (info[i].width, info[i].height, info[i].channels, info[i].bits) == (len(raws[i]) - 1, 1, 1, 8)
            finally:
                hip.gamut_hip_device_free(d_out)
    finally:
        if old is None:
            os.environ.pop("GAMUT_HIP_PNG_INFLATE", None)
        else:
            os.environ["GAMUT_HIP_PNG_INFLATE"] = old
    for i, raw in enumerate(raws):
        row = np.frombuffer(raw, np.uint8)[1:]
        at = int(offs[i])
        assert np.array_equal(got["host"][at:at + row.size], row), f"{names[i]}: the host path"
        assert np.array_equal(got["device"][at:at + row.size], row), f"{names[i]}: inflate on the device, first difference at {int(np.flatnonzero(got['device'][at:at + row.size] != row)[0])}"
    assert np.array_equal(got["host"], got["device"])
