"""The hand-built baseline scans of tests/jpeg_scan_cases.py through the device decoders: k_jpeg_unstuff, k_jpeg_entropy (a lane per short
segment) and k_jpeg_entropy_sync (up to 512 self-synchronising lanes per long one), tables in LDS and in global memory, dense and token
hand-off.  Coefficients and max_zag are compared bit for bit with the oracle; a file the reference refuses (or has no defined result for) has
to come back refused, its neighbours intact.  tests/test_jpeg_scan_cases_cpu.py proves on the CPU that every case stands on what its name says."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_scan_cases as S
import jpeg_scan_ref as R
import oracle_lib as O
from gamut_amd import _capi
from test_jpeg_gpu import _decode_batch_device, dev_upload, handoff, unstuff_site      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

CASES = S.corpus()
IMAGES = [c for c in CASES if c.verdict == "image"]
G = S.geometry()
TAIL = 4                                                       # poisoned blocks behind the last file


@pytest.fixture(scope="module")
def expected():
    """the oracle's reading of every case, made once: (coefficients, max_zag) or None"""
    out = {}
    for c in CASES:
        try:
            d = O.DecodedJpeg(c.data)
            out[c.name] = (d.coeffs, d.max_zag)
        except ValueError:
            out[c.name] = None
    assert all((out[c.name] is not None) == (c.verdict == "image") for c in CASES)
    return out


def entropy_decode(L, blobs):
    """gamut_hip_jpeg_entropy_decode_device into poisoned buffers -> (rc, host status, device status, [(coeffs, max_zag) or None]); what lies behind
    the last file's blocks has to be as it was"""
    n = len(blobs)
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    hdr = (_capi.JpegFrame * n)()
    nblk = []
    for i in range(n):
        rc = L.gamut_hip_jpeg_read_header(ptrs[i], lens[i], C.byref(hdr[i]))
        nblk.append(hdr[i].mcus_per_row * hdr[i].mcus_per_col * hdr[i].blocks_per_mcu if rc == 0 else 0)
    off = np.concatenate([[0], np.cumsum(nblk)[:-1]]).astype(np.int64)
    co_off = off * 64
    total = max(1, sum(nblk))
    dco = dev_upload(L, np.full((total + TAIL) * 64, 0x5A5A, np.uint16))
    dzz = dev_upload(L, np.full(total + TAIL, 0xEE, np.uint8))
    dst = dev_upload(L, np.full(n + 1, 0xFFFFFFFF, np.uint32))
    info = (_capi.JpegFrame * n)()
    hst = (C.c_int * n)()
    rc = L.gamut_hip_jpeg_entropy_decode_device(ptrs, lens, n, co_off.ctypes.data_as(C.POINTER(C.c_int64)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                dco, dzz, dst, info, hst, None)
    co = np.empty((total + TAIL) * 64, np.uint16); zz = np.empty(total + TAIL, np.uint8); st = np.empty(n + 1, np.uint32)
    _capi.check(L.gamut_hip_memcpy_d2h(co.ctypes.data, dco, co.nbytes, None))
    _capi.check(L.gamut_hip_memcpy_d2h(zz.ctypes.data, dzz, zz.nbytes, None))
    _capi.check(L.gamut_hip_memcpy_d2h(st.ctypes.data, dst, st.nbytes, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    for p in (dco, dzz, dst):
        L.gamut_hip_device_free(p)
    assert (co[total * 64:] == 0x5A5A).all() and (zz[total:] == 0xEE).all() and st[n] == 0xFFFFFFFF, "wrote behind the last file"
    co = co.view(np.int16)
    res = [None if hst[i] else (co[co_off[i]:co_off[i] + nblk[i] * 64].reshape(-1, 64), zz[off[i]:off[i] + nblk[i]]) for i in range(n)]
    return rc, list(hst), st[:n], res


def judge(cases, hst, st, res, expected, where):
    """as _expect_like_oracle of test_jpeg_gpu.py: the verdict is the reference's (a refused file has a non-zero status), the numbers are its numbers"""
    for i, c in enumerate(cases):
        exp = expected[c.name]
        assert (hst[i] == 0 and st[i] == 0) == (exp is not None), (where, c.name, hst[i], int(st[i]))
        if exp is not None:
            assert np.array_equal(res[i][0], exp[0]), (where, c.name, np.argwhere(res[i][0] != exp[0])[:4].tolist())
            assert np.array_equal(res[i][1], exp[1]), (where, c.name, np.flatnonzero(res[i][1] != exp[1])[:8].tolist())


_READ = {}


def read(c):
    """the plain decoder's reading of a well-formed case (its tables and census), made once"""
    if c.name not in _READ:
        _READ[c.name] = R.decode(c.data)
    return _READ[c.name]


def tables_of(cases):
    """distinct Huffman / quantisation tables the scans of these (well-formed) files use, as the batch call counts them"""
    huff, quant = set(), set()
    for c in cases:
        d = read(c)
        for key in d.census.tables_used:
            huff.add((tuple(d.huff[key].bits), tuple(d.huff[key].vals)))
        for comp in d.frame["comp"]:
            quant.add(tuple(d.quant[comp["tq"]]))
    return len(huff), len(quant)


def test_every_case_in_one_batch_tables_in_global_memory(hip, unstuff_site, expected):
    """the whole corpus in one call: far more distinct hand-built tables than a workgroup keeps in LDS, so all three kernels read them from global
    memory; long and short segments, refused files between good ones"""
    nh, nq = tables_of([c for c in CASES if c.wellformed and c.verdict == "image"])
    assert nh > G["lds_huff"] and nq > G["lds_huff"]
    rc, hst, st, res = entropy_decode(hip, [c.data for c in CASES])
    judge(CASES, hst, st, res, expected, unstuff_site)
    assert (rc != 0) == any(hst)


def test_each_image_case_alone_tables_in_lds(hip, unstuff_site, expected):
    """every file the reference decodes, a call of its own: its few tables live in LDS (the four-table build of the kernels)"""
    for c in IMAGES:
        rc, hst, st, res = entropy_decode(hip, [c.data])
        assert rc == 0, (c.name, hip.gamut_hip_last_error())
        judge([c], hst, st, res, expected, unstuff_site)


@pytest.fixture
def no_host_redo():
    """a file a kernel flags is decoded again by the host feeder behind the device pass -- right, and invisible.  GAMUT_HIP_JPEG_HOST_REDO=0 leaves such
    a file refused: what then comes back OK, the kernels decoded themselves"""
    os.environ["GAMUT_HIP_JPEG_HOST_REDO"] = "0"
    yield
    del os.environ["GAMUT_HIP_JPEG_HOST_REDO"]


def test_the_kernels_decode_every_well_formed_case_themselves(hip, unstuff_site, no_host_redo, expected):
    """with the host feeder's second reading switched off: every stream T.81 defines and the reference decodes comes out of the KERNELS, in one
    batch (tables in global memory) and alone (in LDS); the streams that rest on a habit of the reference are the host feeder's by design
    (an unassigned bit pattern, r/0 and a scan that ends early are what the kernels flag) and stay refused here"""
    own = [c for c in IMAGES if c.wellformed]
    theirs = [c for c in IMAGES if not c.wellformed and not c.name.startswith("symbol_")]        # (r/0 reads as EOB in the kernels as well)
    assert len(own) >= 50 and len(theirs) >= 3
    batch = own + theirs
    rc, hst, st, res = entropy_decode(hip, [c.data for c in batch])
    for c, h in zip(batch, hst):
        assert (h == 0) == c.wellformed, (c.name, h, unstuff_site)
    judge(own, hst, st, res, expected, unstuff_site)
    for c in own:
        rc, hst, st, res = entropy_decode(hip, [c.data])
        assert rc == 0 and hst == [0], (c.name, hip.gamut_hip_last_error())
        judge([c], hst, st, res, expected, unstuff_site)


def test_the_token_kernel_decodes_its_files_itself(hip, no_host_redo):
    """the same for the files -> pixels call: the 4:2:0 files of one long segment hand over tokens and need no second reading"""
    tok = [c for c in IMAGES if c.wellformed and read(c).frame["nb"] == 6 and len(read(c).census.segments) == 1 and read(c).census.segments[0] >= G["sync_min_bytes"]]
    assert len(tok) >= 3
    rc, hst, res = _decode_batch_device(hip, [c.data for c in tok], 4)
    assert rc == 0 and not any(hst), (hst, hip.gamut_hip_last_error())
    for c, got in zip(tok, res):
        assert np.array_equal(got, O.decompress_jpeg(c.data, 4)[0]), c.name


def test_a_batch_of_five_to_eight_tables_in_lds(hip, unstuff_site, expected):
    """more tables than the four-table build holds, no more than kLdsHuff: the other LDS build, on long and short segments"""
    picked, rest = [], [c for c in IMAGES if c.wellformed]
    for c in rest:
        nh, nq = tables_of(picked + [c])
        if nh <= G["lds_huff"] and nq <= G["lds_huff"]:
            picked.append(c)
    nh, nq = tables_of(picked)
    assert 4 < nh <= G["lds_huff"] and nq <= G["lds_huff"] and len(picked) >= 12, (nh, nq, len(picked))
    seg = [max(read(c).census.segments) for c in picked]
    assert max(seg) >= G["sync_min_bytes"] and min(seg) < G["sync_min_bytes"]
    rc, hst, st, res = entropy_decode(hip, [c.data for c in picked])
    assert rc == 0 and not any(hst) and not st.any()
    judge(picked, hst, st, res, expected, unstuff_site)


@pytest.mark.parametrize("checkpoints", [1, 3, 9])
def test_phase_locked_streams_with_close_checkpoints(hip, checkpoints, expected):
    """streams a decoder entered at a lane boundary never falls into step with: the fixed point takes a sweep per lane, and no checkpoint of a
    re-decode ever matches the pass before -- with every number of checkpoints the lane's area holds"""
    phase = [c for c in CASES if c.family == "phase"]
    assert len(phase) == 4
    os.environ["GAMUT_HIP_JPEG_CHECKPOINTS"] = str(checkpoints)
    try:
        rc, hst, st, res = entropy_decode(hip, [c.data for c in phase])
        assert rc == 0
        judge(phase, hst, st, res, expected, checkpoints)
        for c in phase[-2:]:                                    # and alone (tables in LDS)
            rc, hst, st, res = entropy_decode(hip, [c.data])
            judge([c], hst, st, res, expected, checkpoints)
    finally:
        del os.environ["GAMUT_HIP_JPEG_CHECKPOINTS"]


def test_files_to_pixels_tokens_and_dense(hip, handoff):
    """every image case through gamut_hip_jpeg_decode_batch_device: pixels == the oracle's.  The 4:2:0 files of one segment of kSyncMinBytes and
    more hand over tokens (unless the dense hand-off is forced): coded coefficients whose product is 0, complete codes, the comb"""
    tok = [c for c in IMAGES if c.claims.get("scan_type") == 4 or "4_2_0_long" in c.name]
    tok = [c for c in tok if c.wellformed and len(read(c).census.segments) == 1 and read(c).census.segments[0] >= G["sync_min_bytes"]]
    assert len(tok) >= 3, [c.name for c in tok]
    blobs = [c.data for c in IMAGES]
    for comps in (4, 1):
        rc, hst, res = _decode_batch_device(hip, blobs, comps)
        assert rc == 0 and not any(hst), (rc, hst, hip.gamut_hip_last_error())
        for c, got in zip(IMAGES, res):
            exp = O.decompress_jpeg(c.data, comps)
            assert exp is not None and np.array_equal(got, exp[0]), (c.name, comps, handoff)
    rc, hst, res = _decode_batch_device(hip, [c.data for c in tok], 3)        # the token files alone: four tables, in LDS
    assert rc == 0 and not any(hst)
    for c, got in zip(tok, res):
        assert np.array_equal(got, O.decompress_jpeg(c.data, 3)[0]), (c.name, handoff)


def test_refused_files_in_the_files_to_pixels_call(hip, handoff):
    """the files the reference refuses or has no defined result for, between good neighbours: refused, the neighbours' pixels the oracle's"""
    bad = [c for c in CASES if c.verdict != "image"]
    good = IMAGES[:len(bad) + 1]
    mixed = [good[0]]
    for b, g in zip(bad, good[1:]):
        mixed += [b, g]
    rc, hst, res = _decode_batch_device(hip, [c.data for c in mixed], 4)
    assert rc != 0
    for c, h, got in zip(mixed, hst, res):
        exp = O.decompress_jpeg(c.data, 4)
        assert (h == 0) == (c.verdict == "image") == (exp is not None), (c.name, h)
        if exp is not None:
            assert np.array_equal(got, exp[0]), c.name
