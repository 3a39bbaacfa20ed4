"""GPU parity: JPEG block reconstruction (IDCT + 4:2:0 frequency-domain upsample + YCbCr->RGB)
through the C ABI vs the CPU oracle.  Bar: bit-exact, every sampling mode, every output format."""
import ctypes as C
import fixtures
import gen as gen_mod
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from gamut_amd import _capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
JPEGS = fixtures.jpegs()
NB = {0: 1, 1: 3, 2: 4, 3: 4, 4: 6}
MCU = {0: (8, 8), 1: (8, 8), 2: (16, 8), 3: (8, 16), 4: (16, 16)}
ZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
       49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dev_upload(L, arr):
    arr = np.ascontiguousarray(arr)
    p = L.gamut_hip_device_malloc(max(16, arr.nbytes))
    assert p
    _capi.check(L.gamut_hip_memcpy_h2d(p, arr.ctypes.data, arr.nbytes, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    return p


def gpu_reconstruct(L, width, height, scan_type, coeffs, max_zag, out_comps, count=1, pad=0):
    """coeffs: (count, nblk, 64) int16.  Returns (count, height, width*out_comps) uint8."""
    coeffs = np.ascontiguousarray(coeffs, np.int16).reshape(count, -1)
    dco = dev_upload(L, coeffs)
    dzz = dev_upload(L, np.ascontiguousarray(max_zag, np.uint8).reshape(count, -1)) if max_zag is not None else None
    pitch = width * out_comps + pad
    istride = pitch * height + 64
    host = np.full(count * istride, 0xA5, np.uint8)
    dout = dev_upload(L, host)
    nblk = coeffs.shape[1] // 64
    _capi.check(L.gamut_hip_jpeg_reconstruct_batch_device(dco, coeffs.shape[1], dzz, nblk, dout, pitch, istride,
                                                           width, height, scan_type, out_comps, count, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    _capi.check(L.gamut_hip_memcpy_d2h(host.ctypes.data, dout, host.nbytes, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    for p in (dco, dzz, dout):
        if p:
            L.gamut_hip_device_free(p)
    out = np.empty((count, height, width * out_comps), np.uint8)
    for i in range(count):
        img = host[i * istride:(i + 1) * istride]
        rows = img[:pitch * height].reshape(height, pitch)
        out[i] = rows[:, :width * out_comps]
        assert (rows[:, width * out_comps:] == 0xA5).all(), "wrote into the row gap"
        assert (img[pitch * height:] == 0xA5).all(), "wrote past the image"
    return out


def random_coeffs(rng, nblk, kind):
    if kind == "natural":           # DCT-like: decaying magnitudes, mostly zero high frequencies
        scale = 600.0 / (1.0 + np.add.outer(np.arange(8), np.arange(8)) ** 2)
        c = rng.normal(0, 1, (nblk, 8, 8)) * scale
        c[:, 0, 0] = rng.integers(-1000, 1000, nblk)
        c = np.where(rng.random((nblk, 8, 8)) < 0.5, 0, c)
        return np.round(c).astype(np.int16).reshape(nblk, 64)
    if kind == "dense":
        return rng.integers(-256, 257, (nblk, 64)).astype(np.int16)
    return rng.integers(-32768, 32768, (nblk, 64)).astype(np.int16)        # "wild": every int16, wrap-around arithmetic


@pytest.mark.parametrize("path", JPEGS, ids=[os.path.basename(p) for p in JPEGS])
def test_fixture_files(hip, path):
    """product feeder -> GPU kernels == oracle == frozen golden hashes, for out_comps 1, 3, 4."""
    data = open(path, "rb").read()
    name = os.path.basename(path)[:-4]
    buf = np.frombuffer(data, np.uint8)
    fr = _capi.JpegFrame()
    _capi.check(hip.gamut_hip_jpeg_decode_coeffs(buf.ctypes.data, buf.size, C.byref(fr)))
    nblk = fr.mcus_per_row * fr.mcus_per_col * fr.blocks_per_mcu
    co = np.ctypeslib.as_array(fr.coeffs, (nblk, 64)).copy()
    mz = np.ctypeslib.as_array(fr.max_zag, (nblk,)).copy()
    w, h, comps, st = fr.width, fr.height, fr.comps, fr.scan_type
    hip.gamut_hip_jpeg_frame_free(C.byref(fr))
    for rc in (1, 3, 4):
        exp = O.jpeg_reconstruct(w, h, comps, st, co, mz, rc)
        got = gpu_reconstruct(hip, w, h, st, co[None], mz[None], rc)[0]
        assert np.array_equal(got, exp), f"{name} comps{rc}: {np.count_nonzero(got != exp)} bytes differ"
        assert sha(got) == GOLDEN["frozen"][f"{name}:comps{rc}"]
        got_dense = gpu_reconstruct(hip, w, h, st, co[None], None, rc, pad=5)[0]      # max_zag = NULL: identical on real data
        assert np.array_equal(got_dense, exp)


def test_reference_derived_vectors(hip):
    """The HIP kernels against tests/golden/jpeg_h2v2_ref.npz DIRECTLY (not via liboracle.so): whole 4:2:0 frames -> rgba8 / rgb8 /
    l8 with the recorded max_zag (and NULL for the dense frames), and idct() per max_zag class through the grey kernel.  The file
    holds outputs of tools/ref_literal_jpeg.py, whose arithmetic statements are transliterated mechanically from jpegload.d."""
    import test_oracle_pinning as P
    V = P.jpeg_vectors()
    for f in range(int(V["n_frames"])):
        w, h = int(V[f"frame{f}_w"]), int(V[f"frame{f}_h"])
        co = V[f"frame{f}_coeffs"]
        dense = bool(V[f"frame{f}_dense"])
        for comps in (4, 3, 1):
            exp = P.rgba_to(V[f"frame{f}_rgba"], w, comps)
            for mz in ([None, V[f"frame{f}_max_zag"]] if dense else [V[f"frame{f}_max_zag"]]):
                got = gpu_reconstruct(hip, w, h, 4, co[None], None if mz is None else mz[None], comps)[0]
                assert np.array_equal(got, exp), (f, comps, mz is None)
    # idct(block, max_zag): the blocks as a grey image, one block per MCU
    n = len(V["blocks"])
    got = gpu_reconstruct(hip, 8 * n, 8, 0, V["blocks"][None], V["block_max_zag"][None], 1)[0]
    assert np.array_equal(got.reshape(8, n, 8).transpose(1, 0, 2).reshape(n, 64), V["idct"])


@pytest.fixture(params=["cols", "plain"])
def plain_kernels(request):
    """which kernels reconstruct every sampling mode but 4:2:0: k_jpeg_cols / k_jpeg_cols4 (a thread per pixel column keeps its samples in registers,
    round 4) or k_jpeg_plain (samples through an LDS byte buffer, rounds 1-3; GAMUT_HIP_JPEG_COLS=plain)"""
    old = os.environ.get("GAMUT_HIP_JPEG_COLS")
    os.environ["GAMUT_HIP_JPEG_COLS"] = request.param
    yield request.param
    if old is None:
        del os.environ["GAMUT_HIP_JPEG_COLS"]
    else:
        os.environ["GAMUT_HIP_JPEG_COLS"] = old


@pytest.mark.parametrize("scan_type", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["natural", "dense", "wild"])
def test_random_coefficients(hip, scan_type, kind, plain_kernels):
    # (4:2:0 has one kernel whatever GAMUT_HIP_JPEG_COLS says: its "plain" cases check that the setting leaves that kernel's output alone)
    rng = np.random.default_rng(100 * scan_type + len(kind))
    mw, mh = MCU[scan_type]
    # (256 and 1024 wide: rows of 32 / 64 MCUs take the 32-MCU strips of k_jpeg_cols / k_jpeg_cols4, the other sizes the 24-MCU ones)
    for (w, h) in [(1, 1), (17, 9), (130, 33), (16 * 9 + 3, 16 * 2), (257, 65), (256, 24), (1024, 9)]:
        nblk = ((w + mw - 1) // mw) * ((h + mh - 1) // mh) * NB[scan_type]
        co = random_coeffs(rng, nblk, kind)
        comps = 1 if scan_type == 0 else 3
        for rc in (4, 3, 1):
            exp = O.jpeg_reconstruct(w, h, comps, scan_type, co, None, rc)
            got = gpu_reconstruct(hip, w, h, scan_type, co[None], None, rc, pad=(3 if rc != 4 else 8))[0]
            assert np.array_equal(got, exp), f"st={scan_type} {kind} {w}x{h} comps{rc}: {np.count_nonzero(got != exp)} differ"


@pytest.mark.parametrize("scan_type", [0, 1, 2, 3, 4])
def test_sparse_paths_with_max_zag(hip, scan_type, plain_kernels):
    """m_mcu_block_max_zag drives the reference's sparse IDCT variants (jpegload.d:295-376); with full-range int16
    coefficients the Col!(1) shortcut (max_zag <= 2) differs from the dense form by 32-bit wrap-around and must be matched."""
    rng = np.random.default_rng(5 + scan_type)
    mw, mh = MCU[scan_type]
    w, h = 16 * 11 + 5, 16 * 3 + 1
    nblk = ((w + mw - 1) // mw) * ((h + mh - 1) // mh) * NB[scan_type]
    co = random_coeffs(rng, nblk, "wild")
    mz = rng.choice([1, 2, 2, 2, 3, 4, 6, 10, 20, 36, 64], nblk).astype(np.uint8)
    zag = np.array(ZAG)
    for i in range(nblk):
        co[i, zag[mz[i]:]] = 0
    comps = 1 if scan_type == 0 else 3
    exp = O.jpeg_reconstruct(w, h, comps, scan_type, co, mz, 4 if comps == 3 else 1)
    dense = O.jpeg_reconstruct(w, h, comps, scan_type, co, None, 4 if comps == 3 else 1)
    assert not np.array_equal(exp, dense), "test vector does not exercise the Col!1 overflow case"
    got = gpu_reconstruct(hip, w, h, scan_type, co[None], mz[None], 4 if comps == 3 else 1)[0]
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["natural", "wild"])
def test_wave_uniform_sparse_luma_passes(hip, kind):
    """The tuned 4:2:0 kernel takes idct_4x4's Row!4 / Col!4 passes for a wave (2 MCUs = 8 Y blocks) none of whose Y blocks reaches
    zig-zag position 10 (jpegload.d:295-397: the row / column tables of max_zag <= 10 name rows 0-3 and columns 0-3 only).  Regions of
    whole sparse MCU pairs next to dense ones, sparse pairs at the ragged right / bottom edges, Col!1 blocks (max_zag <= 2) inside
    sparse waves, every output format; == the oracle, which follows the reference's per-block table look-ups."""
    rng = np.random.default_rng(77 + len(kind))
    zag = np.array(ZAG)
    for (w, h) in [(16 * 21 + 5, 16 * 4 + 3), (16 * 2, 16), (16 * 8 + 1, 16 * 2 + 9), (16 * 16, 16 * 3)]:
        mx, my = (w + 15) // 16, (h + 15) // 16
        co = random_coeffs(rng, mx * my * 6, kind).reshape(my, mx, 6, 64)
        mz = rng.choice([1, 2, 3, 7, 10, 11, 15, 28, 64], (my, mx, 6)).astype(np.uint8)
        sparse_mcu = rng.random((my, (mx + 1) // 2)) < 0.6                         # by wave: MCU pairs (2k, 2k + 1) of a row
        sparse_mcu = np.repeat(sparse_mcu, 2, axis=1)[:, :mx]
        low = rng.choice([1, 2, 3, 5, 9, 10], (my, mx, 4)).astype(np.uint8)
        mz[:, :, :4] = np.where(sparse_mcu[:, :, None], low, mz[:, :, :4])
        mz[0, -1, :4] = 10; mz[-1, :, :4] = rng.choice([2, 10], (mx, 4))           # the edges take the sparse passes too
        for idx in np.ndindex(my, mx, 6):
            co[idx][zag[mz[idx]:]] = 0
        co = co.reshape(-1, 64); mzf = mz.reshape(-1)
        for rc in (4, 3, 1):
            exp = O.jpeg_reconstruct(w, h, 3, 4, co, mzf, rc)
            got = gpu_reconstruct(hip, w, h, 4, co[None], mzf[None], rc, pad=(3 if rc != 4 else 8))[0]
            assert np.array_equal(got, exp), f"{kind} {w}x{h} comps{rc}: {np.count_nonzero(got != exp)} differ"


def test_batch_strides_and_1080p(hip):
    """uniform batch launch: per-image strides honoured; one full-size 1920x1080 4:2:0 frame (BASELINE.json config 2 geometry)."""
    rng = np.random.default_rng(42)
    w, h, st = 1920, 1080, 4
    nblk = 120 * 68 * 6
    co = np.stack([random_coeffs(rng, nblk, "natural") for _ in range(3)])
    got = gpu_reconstruct(hip, w, h, st, co, None, 4, count=3)
    for i in range(3):
        exp = O.jpeg_reconstruct(w, h, 3, st, co[i], None, 4)
        assert np.array_equal(got[i], exp), f"image {i}"


def test_descriptor_api_mixed_sizes(hip):
    rng = np.random.default_rng(8)
    jobs = [(100, 60, 4, 4), (33, 17, 1, 3), (64, 64, 0, 1), (250, 40, 2, 4)]
    descs = (_capi.JpegDesc * len(jobs))()
    keep, exps, outs = [], [], []
    for i, (w, h, st, rc) in enumerate(jobs):
        mw, mh = MCU[st]
        nblk = ((w + mw - 1) // mw) * ((h + mh - 1) // mh) * NB[st]
        co = random_coeffs(rng, nblk, "natural")
        exps.append(O.jpeg_reconstruct(w, h, 1 if st == 0 else 3, st, co, None, rc))
        dco = dev_upload(hip, co)
        dout = dev_upload(hip, np.zeros(w * h * rc, np.uint8))
        keep += [dco, dout]; outs.append((dout, w * h * rc))
        descs[i].coeffs, descs[i].max_zag, descs[i].out, descs[i].out_pitch = dco, None, dout, w * rc
        descs[i].width, descs[i].height, descs[i].scan_type, descs[i].out_comps = w, h, st, rc
    _capi.check(hip.gamut_hip_jpeg_reconstruct_device(descs, len(jobs), None))
    _capi.check(hip.gamut_hip_stream_synchronize(None))
    for (dout, n), exp in zip(outs, exps):
        got = np.empty(n, np.uint8)
        _capi.check(hip.gamut_hip_memcpy_d2h(got.ctypes.data, dout, n, None))
        _capi.check(hip.gamut_hip_stream_synchronize(None))
        assert np.array_equal(got, exp.reshape(-1))
    for p in keep:
        hip.gamut_hip_device_free(p)


@pytest.mark.parametrize("path", JPEGS, ids=[os.path.basename(p) for p in JPEGS])
def test_host_dropin_decompress(hip, path):
    """gamut_hip_decompress_jpeg_image_from_memory == decompress_jpeg_image_from_stream (jpegload.d:3720-3808)."""
    data = open(path, "rb").read()
    buf = np.frombuffer(data, np.uint8)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for rc in (-1, 1, 3, 4):
        exp = O.decompress_jpeg(data, rc)
        w, h, ac = C.c_int(), C.c_int(), C.c_int()
        par, dpi = C.c_float(), C.c_float()
        p = hip.gamut_hip_decompress_jpeg_image_from_memory(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ac),
                                                            C.byref(par), C.byref(dpi), rc)
        assert p, hip.gamut_hip_last_error()
        comps = ac.value if rc < 0 else rc
        got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h.value, w.value * comps)).copy()
        libc.free(p)
        assert np.array_equal(got, exp[0])
        assert ac.value == exp[1] and O.same_density((par.value, dpi.value), exp[2:])
    # error convention: NULL + message, no exception (jpegload.d:3726-3733)
    assert not hip.gamut_hip_decompress_jpeg_image_from_memory(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ac),
                                                                C.byref(par), C.byref(dpi), 2)
    assert not hip.gamut_hip_decompress_jpeg_image_from_memory(buf.ctypes.data, 0, C.byref(w), C.byref(h), C.byref(ac),
                                                                C.byref(par), C.byref(dpi), 4)
    assert hip.gamut_hip_last_error() != b""


# ------------------------------------------------------------------ entropy decode on the device
def _entropy_decode_device(L, blobs):
    """-> (rc, host_status, dev_status, [(coeffs, max_zag) or None per file])"""
    n = len(blobs)
    bufs = [np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8) for b in blobs]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    hdr = (_capi.JpegFrame * n)()
    nblk = []
    for i in range(n):
        rc = L.gamut_hip_jpeg_read_header(ptrs[i], lens[i], C.byref(hdr[i]))
        nblk.append(hdr[i].mcus_per_row * hdr[i].mcus_per_col * hdr[i].blocks_per_mcu if rc == 0 else 0)
        assert not hdr[i].coeffs and not hdr[i].max_zag
    co_off = np.concatenate([[0], np.cumsum(nblk)[:-1]]).astype(np.int64) * 64
    zz_off = np.concatenate([[0], np.cumsum(nblk)[:-1]]).astype(np.int64)
    total = max(1, sum(nblk))
    dco = dev_upload(L, np.full(total * 64, 0x5A5A, np.uint16))          # poisoned: the call must clear what it owns
    dzz = dev_upload(L, np.full(total, 0xEE, np.uint8))
    dst = dev_upload(L, np.full(n, 0xFFFFFFFF, np.uint32))
    info = (_capi.JpegFrame * n)()
    hst = (C.c_int * n)()
    rc = L.gamut_hip_jpeg_entropy_decode_device(ptrs, lens, n, co_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                zz_off.ctypes.data_as(C.POINTER(C.c_int64)), dco, dzz, dst, info, hst, None)
    co = np.empty(total * 64, np.int16); zz = np.empty(total, np.uint8); st = np.empty(n, np.uint32)
    _capi.check(L.gamut_hip_memcpy_d2h(co.ctypes.data, dco, co.nbytes, None))
    _capi.check(L.gamut_hip_memcpy_d2h(zz.ctypes.data, dzz, zz.nbytes, None))
    _capi.check(L.gamut_hip_memcpy_d2h(st.ctypes.data, dst, st.nbytes, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    for p in (dco, dzz, dst):
        L.gamut_hip_device_free(p)
    res = []
    for i in range(n):
        if hst[i] != 0:
            res.append(None)
        else:
            res.append((co[co_off[i]:co_off[i] + nblk[i] * 64].reshape(-1, 64), zz[zz_off[i]:zz_off[i] + nblk[i]], info[i]))
    return rc, list(hst), st, res


def _decode_batch_device(L, blobs, comps):
    """gamut_hip_jpeg_decode_batch_device -> (rc, host_status, [pixels (h, w * comps) or None per file])"""
    n = len(blobs)
    bufs = [np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8) for b in blobs]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    hdr = (_capi.JpegFrame * n)()
    size = []
    for i in range(n):
        rc = L.gamut_hip_jpeg_read_header(ptrs[i], lens[i], C.byref(hdr[i]))
        size.append(hdr[i].width * hdr[i].height * comps if rc == 0 else 0)
    offs = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    total = max(16, int(sum(size)))
    dout = dev_upload(L, np.full(total + 64, 0xA5, np.uint8))
    info = (_capi.JpegFrame * n)(); hst = (C.c_int * n)()
    rc = L.gamut_hip_jpeg_decode_batch_device(ptrs, lens, n, comps, offs.ctypes.data_as(C.POINTER(C.c_int64)), dout, info, hst, None, None)
    host = np.empty(total + 64, np.uint8)
    _capi.check(L.gamut_hip_memcpy_d2h(host.ctypes.data, dout, host.nbytes, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    L.gamut_hip_device_free(dout)
    assert (host[total:] == 0xA5).all(), "wrote past the last image"
    res = [host[offs[i]:offs[i] + size[i]].reshape(info[i].height, info[i].width * comps) if hst[i] == 0 and size[i] else None for i in range(n)]
    return rc, list(hst), res


@pytest.fixture(params=["tokens", "dense"])
def handoff(request):
    """what the entropy kernels hand to the reconstruction inside gamut_hip_jpeg_decode_batch_device: the token stream (4:2:0 images of one
    long segment; the library's choice) or the dense 128-byte blocks of the coefficient-level entry point"""
    old = os.environ.get("GAMUT_HIP_JPEG_HANDOFF")
    os.environ["GAMUT_HIP_JPEG_HANDOFF"] = request.param
    yield request.param
    if old is None:
        del os.environ["GAMUT_HIP_JPEG_HANDOFF"]
    else:
        os.environ["GAMUT_HIP_JPEG_HANDOFF"] = old


def test_files_to_pixels_token_handoff(hip, handoff):
    """4:2:0 files of one long segment -- the ones that hand over tokens -- of many shapes: widths that end in a partial strip, one MCU
    row, quality 30 .. 100 (3 .. 60 tokens per block), optimised tables, a flat image (a DC token per block and nothing else), noise at
    q 100 (blocks of 64 tokens), mixed with files that keep the dense blocks (4:4:4, grey, restart intervals) and damaged ones: every
    file's pixels == the oracle's, for rgba8 / rgb8 / l8"""
    import io
    from PIL import Image
    import gen
    rng = np.random.default_rng(17)
    blobs = []
    for (w, h, kw) in ((1920, 1080, dict(quality=90)), (1000, 700, dict(quality=30)), (129, 260, dict(quality=75, optimize=True)), (2048, 16, dict(quality=95)),
                       (640, 480, dict(quality=100)), (333, 222, dict(quality=85)), (16, 4000, dict(quality=80))):
        bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(w, h, 40 + w)).save(bio, "JPEG", subsampling=2, **kw); blobs.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(np.full((300, 500, 3), 90, np.uint8)).save(bio, "JPEG", quality=90, subsampling=2); blobs.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(rng.integers(0, 256, (200, 264, 3), dtype=np.uint8)).save(bio, "JPEG", quality=100, subsampling=2); blobs.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(500, 400, 7)).save(bio, "JPEG", quality=90, subsampling=0); blobs.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(500, 400, 8)).convert("L").save(bio, "JPEG", quality=90); blobs.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(800, 600, 9)).save(bio, "JPEG", quality=90, subsampling=2, restart_marker_rows=1); blobs.append(bio.getvalue())
    good = list(range(len(blobs)))
    big = blobs[0]; sos = big.index(b"\xff\xda")
    noisy = bytearray(big)
    for k in rng.integers(sos + 20, len(big) - 2, 200):
        noisy[k] = int(rng.integers(0, 255))
    # damaged scans: what the kernels flag is decoded again by the host feeder -- noise in the scan runs a coefficient past 63 sooner or later (null), a file that
    # ends inside its scan is an image whose rest is flat (jpgd pads the stream with FF D9 and decodes symbol 0 from the 1-bits) -- their neighbours untouched
    blobs += [bytes(noisy), big[:len(big) // 3]]
    for comps in (4, 3, 1):
        rc, hst, res = _decode_batch_device(hip, blobs, comps)
        for i in range(len(blobs)):
            exp = O.decompress_jpeg(blobs[i], comps)
            assert (hst[i] == 0) == (exp is not None), (i, hst[i])
            assert i not in good or exp is not None
            if exp is not None:
                assert np.array_equal(res[i], exp[0]), (i, comps, handoff)
        assert O.decompress_jpeg(blobs[-1], comps) is not None
        assert (rc != 0) == any(h != 0 for h in hst)


def test_files_to_pixels_batch(hip, progressive_mode, handoff):
    """gamut_hip_jpeg_decode_batch_device: every fixture (baseline and progressive, every sampling mode, restart intervals) plus
    damaged files in ONE batch -> the pixels decompress_jpeg_image_from_memory gives (== the oracle), for rgba8 / rgb8 / l8; a bad
    file is reported and does not disturb its neighbours"""
    blobs = [open(p, "rb").read() for p in JPEGS]
    blobs.insert(3, b"not a jpeg at all")
    blobs.insert(9, blobs[0][:200])                                          # truncated in its headers
    for comps in (4, 3, 1):
        rc, hst, res = _decode_batch_device(hip, blobs, comps)
        assert rc != 0 and hst[3] != 0 and hst[9] != 0
        for i, b in enumerate(blobs):
            if i in (3, 9):
                assert res[i] is None
                continue
            exp = O.decompress_jpeg(b, comps)
            assert hst[i] == 0 and np.array_equal(res[i], exp[0]), (i, comps)


def test_files_to_pixels_uniform_batch_in_groups(hip, handoff):
    """a batch large enough for the grouped pipeline (>= 256 files: two groups, each reconstructed behind its own entropy decode,
    runs of equal geometry as one launch): 300 files of three kinds"""
    kinds = [open(os.path.join(HERE, "golden", "jpeg", n), "rb").read() for n in ("cfg1_640x480_420_q90.jpg", "s_131x97_420_rst.jpg", "s_131x97_444.jpg")]
    blobs = [kinds[0]] * 130 + [kinds[1]] * 90 + [kinds[2], kinds[0]] * 40
    rc, hst, res = _decode_batch_device(hip, blobs, 4)
    assert rc == 0 and not any(hst)
    exp = {id(k): O.decompress_jpeg(k, 4)[0] for k in kinds}
    for i, b in enumerate(blobs):
        assert np.array_equal(res[i], exp[id(b)]), i


@pytest.fixture(params=["device", "host"])
def progressive_mode(request):
    """where the progressive files of a batch are entropy-decoded (jpeg_prog.hpp): every scan level on the GPU, or -- what the
    library picks for a few files -- the host feeder on the thread pool plus an upload of the coefficients"""
    old = os.environ.get("GAMUT_HIP_JPEG_PROGRESSIVE")
    os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = request.param
    yield request.param
    if old is None:
        del os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"]
    else:
        os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = old


def test_device_entropy_decode_matches_host_feeder(hip, progressive_mode):
    """every fixture (all sampling modes, optimised tables, restart intervals, baseline AND progressive) in ONE mixed batch: the
    coefficients and max_zag the GPU writes == the oracle's feeder, bit for bit."""
    blobs = [open(p, "rb").read() for p in JPEGS]
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0, hip.gamut_hip_last_error()
    n_prog = 0
    for path, data, h, s, r in zip(JPEGS, blobs, hst, st, res):
        n_prog += b"\xff\xc2" in data[:2000] and os.path.basename(path).startswith("p_")
        assert h == 0 and s == 0, path
        d = O.DecodedJpeg(data)
        co, zz, info = r
        assert (info.width, info.height, info.comps, info.scan_type) == (d.width, d.height, d.comps, d.scan_type)
        assert np.array_equal(co, d.coeffs), path
        assert np.array_equal(zz, d.max_zag), path
    assert n_prog >= 6


def _progressive_files():
    import io
    from PIL import Image
    import gen
    img = Image.fromarray(gen.synth_rgb(1920, 1080, 21))
    small = Image.fromarray(gen.synth_rgb(203, 117, 22))
    blobs = []
    for im, kw in ((img, dict(quality=90, subsampling=2)), (img, dict(quality=75, subsampling=0, optimize=True)),
                   (img, dict(quality=96, subsampling=1)), (img.convert("L"), dict(quality=85)),
                   (small, dict(quality=90, subsampling=2, restart_marker_blocks=5)), (small, dict(quality=50, subsampling=1, restart_marker_rows=1)),
                   (small, dict(quality=100, subsampling=0)), (small.convert("L"), dict(quality=30, restart_marker_blocks=2)),
                   (Image.fromarray(gen.synth_rgb(64, 48, 23)), dict(quality=5, subsampling=2)),
                   (Image.fromarray(np.zeros((40, 56, 3), np.uint8)), dict(quality=90, subsampling=2))):
        bio = io.BytesIO(); im.save(bio, "JPEG", progressive=True, **kw); blobs.append(bio.getvalue())
    return blobs


def test_device_progressive_decode(hip, progressive_mode):
    """progressive files written by libjpeg (its default scan script: DC first, five AC first scans, AC / DC refinements; with and
    without restart intervals, optimised tables, every sampling mode) mixed with baseline ones: == the oracle's feeder"""
    import io
    from PIL import Image
    import gen
    blobs = _progressive_files()
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(333, 222, 24)).save(bio, "JPEG", quality=88, subsampling=2); blobs.insert(3, bio.getvalue())
    assert sum(b"\xff\xc2" in b[:2000] for b in blobs) == len(blobs) - 1
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0 and hst == [0] * len(blobs) and not st.any(), hip.gamut_hip_last_error()
    for k, (data, (co, zz, info)) in enumerate(zip(blobs, res)):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs), (k, np.count_nonzero(co != d.coeffs))
        assert np.array_equal(zz, d.max_zag), k


def _scripted_files(tables="flat"):
    """progressive files with scan scripts libjpeg never writes (tests/jpeg_scripts.py): bands cut four ways under one refinement scan, DC scans
    per component under an interleaved refinement, spectral selection only, three bit planes -- with and without restart intervals.
    tables="comb": the two smaller images under DEEP and FOUR_BANDS, code lengths 1 .. 16 in every table (jpeg_scripts.comb_lengths)
    instead of 8-bit codes throughout -- k_prog_scan's second level and canonical search, which the flat tables never reach"""
    import io
    from PIL import Image
    import gen
    import jpeg_scripts as J
    comb = tables == "comb"
    blobs = []
    for (w, h, kw) in ((203, 117, dict(quality=90, subsampling=2)), (131, 97, dict(quality=75, subsampling=0)), (200, 120, dict(quality=95, subsampling=1)),
                       (640, 360, dict(quality=85, subsampling=2)))[:2 if comb else 4]:
        bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(w, h, 31)).save(bio, "JPEG", **kw)
        for sc in ((J.DEEP, J.FOUR_BANDS) if comb else J.SCRIPTS.values()):
            for ri in (0, 7):
                blobs.append(J.progressive_with_script(bio.getvalue(), sc, ri, tables=tables))
    if comb:
        assert len(blobs) == 8 and all(max(b[b.index(b"\xff\xc4") + 5 + 15], b[b.index(b"\xff\xc4") + 5 + 14]) for b in blobs)     # 15- / 16-bit codes in the first table
        return blobs
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(90, 70, 32)).convert("L").save(bio, "JPEG", quality=80)
    blobs.append(J.progressive_with_script(bio.getvalue(), J.GREY, 0)); blobs.append(J.progressive_with_script(bio.getvalue(), J.GREY, 3))
    return blobs


def test_device_progressive_scan_scripts(hip, progressive_mode):
    """arbitrary scan scripts in one batch: scans that line up (unit u of a scan follows unit u of the scans it stands on, a few dozen units
    behind) next to files whose scans do not (a per-file barrier per level instead): == the oracle's feeder, coefficient for coefficient"""
    blobs = _scripted_files() + _scripted_files("comb")
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0 and hst == [0] * len(blobs) and not st.any(), hip.gamut_hip_last_error()
    for k, (data, (co, zz, info)) in enumerate(zip(blobs, res)):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs), (k, np.count_nonzero(co != d.coeffs))
        assert np.array_equal(zz, d.max_zag), k


def test_device_progressive_comb_tables_come_out_of_the_scan_kernel(hip):
    """a file k_prog_scan flags is decoded again by the host feeder, which would hide a kernel that flags what it should decode: with that second
    reading switched off (GAMUT_HIP_JPEG_HOST_REDO=0) and every scan on the GPU, the comb-table files still come back OK and == the oracle"""
    blobs = _scripted_files("comb")
    os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = "device"; os.environ["GAMUT_HIP_JPEG_HOST_REDO"] = "0"
    try:
        rc, hst, st, res = _entropy_decode_device(hip, blobs)
    finally:
        del os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"]; del os.environ["GAMUT_HIP_JPEG_HOST_REDO"]
    assert rc == 0 and hst == [0] * len(blobs) and not st.any(), (hst, hip.gamut_hip_last_error())
    for k, (data, (co, zz, info)) in enumerate(zip(blobs, res)):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag), k


def test_device_progressive_damaged_scan_that_leaves_its_band(hip, progressive_mode):
    """tests/golden/jpeg_fuzz/prog_refine_mismatch_r04.jpg (found by tools/fuzz_prog_gpu.py in round 4): a damaged `Y 1-5` first scan whose run ends at
    zig-zag position 7, inside the band of the `Y 6-63` scan behind it.  Both decoders accept the file; the reference decodes scan after scan, so
    the later scan's value stands.  On the GPU the two scans used to count as independent (disjoint bands) and ran side by side -- the order of
    two scans is now kept wherever their REACH overlaps (an AC first scan may write up to position 63, a refinement up to Se + 1)."""
    data = open(os.path.join(HERE, "golden", "jpeg_fuzz", "prog_refine_mismatch_r04.jpg"), "rb").read()
    d = O.DecodedJpeg(data)
    rc, hst, st, res = _entropy_decode_device(hip, [data] * 5)
    assert rc == 0 and hst == [0] * 5 and not st.any()
    for co, zz, info in res:
        assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag), np.argwhere(co != d.coeffs)[:4].tolist()


def test_device_progressive_successive_approximation_beyond_the_standard(hip, progressive_mode):
    """tests/golden/jpeg_fuzz/prog_al14_r04.jpg (tools/fuzz_mixed_gpu.py, round 4): an AC scan whose Ah/Al byte was damaged into Al = 14.  The standard
    allows 0 .. 13; read_sos_marker (jpegload.d:1466-1540) takes the nibble as it is and the shifts wrap in jpgd_block_t (16 bits).  The device path used
    to reject the file; now it decodes it like the oracle, as it does hand-made files with Al = 14 / 15 in first and refinement scans of either kind."""
    data = open(os.path.join(HERE, "golden", "jpeg_fuzz", "prog_al14_r04.jpg"), "rb").read()
    blobs = [data]
    files = _progressive_files()
    for good in (files[4], files[6]):                          # 203 x 117: 4:2:0 with restart intervals, 4:4:4 at quality 100
        at = [i for i in range(len(good) - 1) if good[i] == 0xFF and good[i + 1] == 0xDA]
        for sos in at:                                         # every scan of the file in turn: Al = 14 (first scans) / Ah = 15, Al = 14 (refinements); Al = 15
            ns = good[sos + 4]
            j = sos + 5 + 2 * ns + 2
            b = bytearray(good)
            b[j] = 0xFE if good[j] >> 4 else 0x0E
            blobs.append(bytes(b))
            b[j] = 0x0F
            blobs.append(bytes(b))
    expect = []
    for b in blobs:
        try:
            expect.append(O.DecodedJpeg(b))
        except ValueError:
            expect.append(None)
    assert expect[0] is not None and sum(e is not None for e in expect) >= len(blobs) // 2
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    for k, (e, r) in enumerate(zip(expect, res)):
        assert (hst[k] == 0 and st[k] == 0) == (e is not None), (k, hst[k], int(st[k]))
        if e is not None:
            assert np.array_equal(r[0], e.coeffs) and np.array_equal(r[1], e.max_zag), (k, np.argwhere(r[0] != e.coeffs)[:4].tolist())


def test_files_the_fuzzers_found(hip, progressive_mode, unstuff_site):
    """every file of tests/golden/jpeg_fuzz (a GPU decoder and the oracle once disagreed on each: a run leaving its band, octets between a restart
    interval and its marker, an SOS listing a component twice, Al = 14) -- alone and in one batch, through the coefficient-level call and the
    files -> pixels call: verdict, coefficients and pixels == the oracle's"""
    d = os.path.join(HERE, "golden", "jpeg_fuzz")
    blobs = [open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".jpg")]
    expect = []
    for b in blobs:
        try:
            expect.append(O.DecodedJpeg(b))
        except ValueError:
            expect.append(None)
    assert any(e is None for e in expect) and any(e is not None for e in expect)
    for batch in ([[b] for b in blobs] + [blobs]):
        rc, hst, st, res = _entropy_decode_device(hip, batch)
        for k, r in enumerate(res):
            e = expect[blobs.index(batch[k])]
            assert (hst[k] == 0 and st[k] == 0) == (e is not None), (len(batch), k, hst[k], int(st[k]))
            if e is not None:
                assert np.array_equal(r[0], e.coeffs) and np.array_equal(r[1], e.max_zag), (len(batch), k)
                assert O.same_density((r[2].pixel_aspect_ratio, r[2].dpi_y), (e.pixel_aspect_ratio, e.dpi_y)), (len(batch), k)      # find_eoi's segments included
    rc, hst, px = _decode_batch_device(hip, blobs, 4)
    for k, e in enumerate(expect):
        assert (hst[k] == 0) == (e is not None), (k, hst[k])
        if e is not None:
            want = O.decompress_jpeg(blobs[k], 4)[0]
            assert np.array_equal(px[k].reshape(-1), np.ascontiguousarray(want).reshape(-1)), k



def _expect_like_oracle(blobs, hst, st, res, where=""):
    """every file of a coefficient-level device call against the oracle: verdict (a refused file has a non-zero status), coefficients, max_zag"""
    for i, b in enumerate(blobs):
        try:
            d = O.DecodedJpeg(b)
        except ValueError:
            d = None
        assert (hst[i] == 0 and st[i] == 0) == (d is not None), (where, i, hst[i], int(st[i]))
        if d is not None:
            assert np.array_equal(res[i][0], d.coeffs) and np.array_equal(res[i][1], d.max_zag), (where, i)

def test_device_progressive_corrupt_streams(hip):
    """damaged scans of progressive files on the GPU path: no hang, nothing written outside the file's buffers, the damaged
    files flagged (a scan that decodes to the end without an impossible code is not an error for the reference either);
    the intact neighbours are untouched"""
    os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = "device"
    try:
        good = _progressive_files()[0]
        sos = good.index(b"\xff\xda")
        rng = np.random.default_rng(5)
        noisy = bytearray(good)
        for k in rng.integers(sos + 20, len(good) - 2, 400):
            noisy[k] = int(rng.integers(0, 255))
        cut = good[:len(good) // 3]
        blobs = [good, bytes(noisy), cut, good[:100], good]
        rc, hst, st, res = _entropy_decode_device(hip, blobs)
        assert hst[0] == 0 and hst[4] == 0 and st[0] == 0 and st[4] == 0
        assert hst[3] == _capi.ERR_DECODE
        # the damaged ones: whatever k_prog_scan flags is decoded again by the host feeder -- the verdict and the coefficients are the reference's
        _expect_like_oracle(blobs, hst, st, res, "progressive")
    finally:
        del os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"]


def test_device_entropy_decode_large_and_restart_parallel(hip):
    """a 1080p file, and the same pixels with a restart marker every 2 MCU rows (one lane per interval)"""
    import io
    from PIL import Image
    import gen
    img = Image.fromarray(gen.synth_rgb(1920, 1080, 11))
    blobs = []
    for kw in (dict(quality=90, subsampling=2), dict(quality=90, subsampling=2, restart_marker_rows=2),
               dict(quality=50, subsampling=0, optimize=True), dict(quality=95, subsampling=1, restart_marker_blocks=7),
               dict(quality=98, subsampling=1, restart_marker_rows=9), dict(quality=30, subsampling=2)):
        bio = io.BytesIO(); img.save(bio, "JPEG", **kw); blobs.append(bio.getvalue())
    bio = io.BytesIO(); img.convert("L").save(bio, "JPEG", quality=92); blobs.append(bio.getvalue())             # grey: one block per MCU
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(4000, 3000, 12)).save(bio, "JPEG", quality=97, subsampling=0); blobs.append(bio.getvalue())   # a ~5 MB scan
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0 and hst == [0] * len(blobs) and not st.any()
    for data, (co, zz, info) in zip(blobs, res):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag)


def test_device_entropy_decode_corrupt_streams(hip):
    """damaged entropy data must neither hang nor write outside the image's buffers; header damage is a host-side status"""
    good = open(os.path.join(HERE, "golden", "jpeg", "s_131x97_420.jpg"), "rb").read()
    sos = good.index(b"\xff\xda")
    rng = np.random.default_rng(3)
    noisy = bytearray(good)
    for k in rng.integers(sos + 20, len(good) - 2, 40):
        noisy[k] = int(rng.integers(0, 255))
    blobs = [good, good[:sos + 40], bytes(noisy), good[:100], b"", good]
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert hst[0] == 0 and hst[5] == 0 and st[0] == 0 and st[5] == 0
    assert hst[3] == _capi.ERR_DECODE and hst[4] == _capi.ERR_DECODE and rc == _capi.ERR_DECODE
    assert hst[1] == 0                                 # the scan ends after 40 bytes: an image all the same (FF D9 padding, 1-bits, symbol 0)
    _expect_like_oracle(blobs, hst, st, res, "short scans")   # the damaged files as the reference decodes (or refuses) them, their neighbours intact
    # the same for a scan long enough for the multi-lane (self-synchronising) kernel
    import io
    from PIL import Image
    import gen
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(1920, 1080, 13)).save(bio, "JPEG", quality=90, subsampling=2)
    big = bio.getvalue(); sos = big.index(b"\xff\xda")
    noisy = bytearray(big)
    for k in rng.integers(sos + 20, len(big) - 2, 300):
        noisy[k] = int(rng.integers(0, 255))
    blobs = [big, bytes(noisy), big[:len(big) // 2], big[:sos + 5000] + big[-2:], big]
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert hst[0] == 0 and hst[4] == 0 and hst[2] == 0 and hst[3] == 0        # the two truncated scans are images
    _expect_like_oracle(blobs, hst, st, res, "long scans")


@pytest.mark.parametrize("scan_type", [4, 1, 2, 3, 0])
def test_bottom_up_rows_on_the_tuned_kernels(hip, scan_type):
    """a negative out_pitch (rows stored bottom-up: LAYOUT_VERT_FLIPPED, internals/types.d:498-501; Image.loadFromMemory with a flipped
    layout ends here) runs the tuned kernels, not the generic one: same pixels, row y at out + y * pitch with pitch < 0 -- ragged sizes
    (partial MCU rows: the flipped 4:2:0 strip base lies in front of the image), row gaps, every output format, batches"""
    rng = np.random.default_rng(70 + scan_type)
    mw, mh = MCU[scan_type]
    comps = 1 if scan_type == 0 else 3
    for (w, h, n) in ((131, 97, 3), (64, 48, 1), (1920, 33, 2), (17, 200, 2)):
        nblk = ((w + mw - 1) // mw) * ((h + mh - 1) // mh) * NB[scan_type]
        co = np.stack([random_coeffs(rng, nblk, "natural") for _ in range(n)])
        for oc in (4, 3, 1):
            pad = 8 if oc == 4 else 5
            pitch = w * oc + pad
            istride = pitch * h + 64
            host = np.full(n * istride, 0xA5, np.uint8)
            dco = dev_upload(hip, co.reshape(n, -1)); dout = dev_upload(hip, host)
            # row 0 of image i is its LAST row in memory: the pointer handed over is that of row 0, the pitch negative
            _capi.check(hip.gamut_hip_jpeg_reconstruct_batch_device(dco, nblk * 64, None, 0, dout + (h - 1) * pitch, -pitch, istride,
                                                                     w, h, scan_type, oc, n, None))
            _capi.check(hip.gamut_hip_memcpy_d2h(host.ctypes.data, dout, host.nbytes, None)); _capi.check(hip.gamut_hip_stream_synchronize(None))
            hip.gamut_hip_device_free(dco); hip.gamut_hip_device_free(dout)
            for i in range(n):
                img = host[i * istride:(i + 1) * istride]
                rows = img[:pitch * h].reshape(h, pitch)
                exp = O.jpeg_reconstruct(w, h, comps, scan_type, co[i], None, oc)
                assert np.array_equal(rows[::-1, :w * oc], exp), (scan_type, w, h, oc, i)
                assert (rows[:, w * oc:] == 0xA5).all() and (img[pitch * h:] == 0xA5).all(), "wrote outside the rows"


@pytest.fixture(params=["device", "host"])
def unstuff_site(request):
    """where the 0x00 stuffing is dropped and the restart markers are found: k_jpeg_unstuff (the scan uploaded as it is) or host threads"""
    old = os.environ.get("GAMUT_HIP_JPEG_UNSTUFF")
    os.environ["GAMUT_HIP_JPEG_UNSTUFF"] = request.param
    yield request.param
    if old is None:
        del os.environ["GAMUT_HIP_JPEG_UNSTUFF"]
    else:
        os.environ["GAMUT_HIP_JPEG_UNSTUFF"] = old


def _restart_files():
    import io
    from PIL import Image
    import gen
    big = Image.fromarray(gen.synth_rgb(1920, 1080, 31))
    mid = Image.fromarray(gen.synth_rgb(517, 389, 32))
    noisy = Image.fromarray(np.random.default_rng(5).integers(0, 256, (300, 420, 3), dtype=np.uint8))     # many 0xFF bytes in the scan
    blobs = []
    for im, kw in ((big, dict(quality=90, subsampling=2)), (big, dict(quality=95, subsampling=2, restart_marker_rows=1)),
                   (big, dict(quality=85, subsampling=0, restart_marker_rows=4)), (mid, dict(quality=92, subsampling=1, restart_marker_blocks=7)),
                   (mid, dict(quality=75, subsampling=2, restart_marker_blocks=1)), (noisy, dict(quality=100, subsampling=0)),
                   (noisy, dict(quality=98, subsampling=2, restart_marker_rows=2)), (mid.convert("L"), dict(quality=90, restart_marker_rows=3)),
                   (mid, dict(quality=90, subsampling=2, optimize=True, restart_marker_rows=1))):
        bio = io.BytesIO(); im.save(bio, "JPEG", **kw); blobs.append(bio.getvalue())
    return blobs


def test_scan_headers_that_list_components_out_of_order(hip, progressive_mode):
    """the files of tests/test_capi_cpu.py::test_jpeg_feeder_scan_headers_that_list_components_out_of_order through the device decoders: block b of an
    MCU is decoded with the tables and the predictor of the b-th component the SOS lists (DevImage.org), not of the component its position belongs
    to; a repeat that changes the MCU's block count, or any repeat in a progressive interleaved scan, is rejected.  Verdict and coefficients == the
    oracle's; a lane per interval and the multi-lane kernel (a 1080p file)."""
    import io
    from PIL import Image
    import gen
    import test_capi_cpu as T
    files = T._scan_list_files()
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(1920, 1080, 31)).save(bio, "JPEG", quality=90, subsampling=2, optimize=True); files.append(bio.getvalue())
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(1920, 1080, 31)).save(bio, "JPEG", quality=90, subsampling=0, restart_marker_rows=16); files.append(bio.getvalue())
    blobs = [v for f in files for v in gen.sos_component_lists(f)]
    expect = []
    for b in blobs:
        try:
            expect.append(O.DecodedJpeg(b))
        except ValueError:
            expect.append(None)
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    for k, (e, r) in enumerate(zip(expect, res)):
        assert (hst[k] == 0 and st[k] == 0) == (e is not None), (k, hst[k], int(st[k]), "the oracle " + ("decodes it" if e is not None else "rejects it"))
        if e is not None:
            assert np.array_equal(r[0], e.coeffs) and np.array_equal(r[1], e.max_zag), k
    assert sum(e is None for e in expect) >= 10 and sum(e is not None for e in expect) >= 30


_rst_positions = gen_mod.rst_positions
_leftover_variants = gen_mod.leftover_variants


def test_octets_between_a_restart_interval_and_its_marker(hip, unstuff_site, progressive_mode):
    """process_restart (jpegload.d:2335-2402) looks for the marker from where the decoder's INPUT stands (4 + 2 * (bits used / 16) octets into the
    interval, never past the marker): up to 1536 raw bytes to a 0xFF, its fill bytes, then the expected RSTn.  A damaged file may have whole octets
    between an interval's last bit and the marker: skipped if none is 0xFF and all of it fits in the 1536 reads, JPGD_BAD_RESTART_MARKER otherwise.
    The device decodes intervals independently of each other and used to ignore what lies behind an interval's data (found by tools/fuzz_mixed_gpu.py
    against the oracle in round 4); now the kernel that decodes an interval judges its leftover (restart_leftover_bad).  Verdict == the oracle's file
    by file, coefficients too where it decodes: a lane per interval, the multi-lane kernel (long intervals), progressive scans of every kind."""
    import io
    from PIL import Image
    import gen
    import jpeg_scripts as JS
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(160, 96, 32)).save(bio, "JPEG", quality=90, subsampling=2, restart_marker_blocks=3); small = bio.getvalue()
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(1920, 1080, 31)).save(bio, "JPEG", quality=92, subsampling=2, restart_marker_rows=8); big = bio.getvalue()
    prog = JS.progressive_with_script(small, JS.LIBJPEG_DEFAULT, restart=4)
    n_prog = len(_rst_positions(prog))
    blobs = _leftover_variants(small, 2) + _leftover_variants(small, len(_rst_positions(small)) - 1) + _leftover_variants(big, 1)
    for which in range(0, n_prog, max(1, n_prog // 12)):                  # markers of every scan of the script (DC first / refine, AC first / refine)
        blobs += _leftover_variants(prog, which)
    # and behind the LAST interval (no marker to find: whatever lies between the last block and the EOI is nobody's)
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(1920, 1080, 31)).save(bio, "JPEG", quality=92, subsampling=2); plain = bio.getvalue()
    for d in (small, big, plain, prog):
        blobs += [d[:-2] + b"\x11" * 1400 + d[-2:], d[:-2] + b"\x11" * 7000 + d[-2:], d[:-2] + b"\x11\xff\x00" * 500 + d[-2:]]
    expect = []
    for b in blobs:
        try:
            expect.append(O.DecodedJpeg(b))
        except ValueError:
            expect.append(None)
    assert sum(e is None for e in expect) > len(blobs) // 4 and sum(e is not None for e in expect) > len(blobs) // 4
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    for k, (e, r) in enumerate(zip(expect, res)):
        assert (hst[k] == 0) == (e is not None), (k, hst[k], int(st[k]), "the oracle " + ("decodes it" if e is not None else "rejects it"))
        if e is not None:
            assert st[k] == 0 and np.array_equal(r[0], e.coeffs) and np.array_equal(r[1], e.max_zag), k
        else:
            assert hst[k] == _capi.ERR_DECODE


def test_device_unstuff_equals_host_unstuff(hip, unstuff_site):
    """the scan as it is in the file -> unstuffed, padded, cut at its restart markers: on the device (k_jpeg_unstuff: get_bits_no_markers'
    FF00 rule jpegload.d:722-743, process_restart :2335-2402) and on the host threads -- the coefficients must be the oracle's either way:
    no restart markers, a marker per MCU row (long segments), every few blocks (a lane each), a marker per block (tiny: the host's share
    unless forced), noise at q 100 (an 0xFF every few hundred bytes), optimised tables"""
    blobs = _restart_files() + [open(p, "rb").read() for p in JPEGS if "_rst" in p or "cfg1" in p]
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0 and hst == [0] * len(blobs) and not st.any(), (rc, hst, st, hip.gamut_hip_last_error())
    for data, (co, zz, info) in zip(blobs, res):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag)


@pytest.mark.parametrize("checkpoints", [1, 3, 9])
def test_counting_passes_with_close_checkpoints(hip, checkpoints):
    """the self-synchronising decoder's re-decode passes stop at the first checkpoint where they stand in the previous pass's state.  A
    checkpoint in the few bits a pass may overshoot its sub-sequence by is reached by some passes only: a pass that runs to its end must
    leave none of an earlier pass standing (round 4: with nine checkpoints per lane the last block of a restart segment of the 1080p
    file below went missing; the shipped six had not shown it).  Every count the lane's area holds, on the files with long restart segments."""
    os.environ["GAMUT_HIP_JPEG_CHECKPOINTS"] = str(checkpoints)
    try:
        blobs = _restart_files() + [open(p, "rb").read() for p in JPEGS if "_rst" in p or "cfg1" in p]
        rc, hst, st, res = _entropy_decode_device(hip, blobs)
        assert rc == 0 and hst == [0] * len(blobs) and not st.any(), (rc, hst, st, hip.gamut_hip_last_error())
        for k, (data, (co, zz, info)) in enumerate(zip(blobs, res)):
            d = O.DecodedJpeg(data)
            assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag), (k, np.count_nonzero(co != d.coeffs))
    finally:
        del os.environ["GAMUT_HIP_JPEG_CHECKPOINTS"]


def test_device_unstuff_restart_marker_errors(hip, unstuff_site):
    """a wrong RSTn number and a missing restart marker fail the FILE (JPGD_BAD_RESTART_MARKER, jpegload.d:2360-2364), whoever finds
    them; its neighbours decode; a scan that ends with a lone 0xFF, or without EOI, is data up to its last byte"""
    import io
    from PIL import Image
    import gen
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(640, 480, 33)).save(bio, "JPEG", quality=90, subsampling=2, restart_marker_rows=2)
    good = bio.getvalue()
    sos = good.index(b"\xff\xda")
    k = good.index(b"\xff\xd3", sos)
    wrong = good[:k + 1] + b"\xd5" + good[k + 2:]                                  # RST3 -> RST5
    missing = good[:k] + good[k + 2:]                                             # RST3 removed: the segment runs on into RST4
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(333, 222, 34)).save(bio, "JPEG", quality=88, subsampling=2)
    plain = bio.getvalue()
    blobs = [good, wrong, missing, good, plain[:-2], plain[:-2] + b"\xff", plain]
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert hst[1] == _capi.ERR_DECODE and hst[2] == _capi.ERR_DECODE and rc == _capi.ERR_DECODE
    assert b"restart marker" in hip.gamut_hip_last_error()
    assert [hst[i] for i in (0, 3, 4, 5, 6)] == [0] * 5 and not st[[0, 3, 4, 6]].any()
    d = O.DecodedJpeg(good)
    for i in (0, 3):
        assert np.array_equal(res[i][0], d.coeffs) and np.array_equal(res[i][1], d.max_zag)
    d = O.DecodedJpeg(plain)
    for i in (4, 6):
        assert np.array_equal(res[i][0], d.coeffs) and np.array_equal(res[i][1], d.max_zag)


def test_files_to_pixels_reports_damaged_entropy_data(hip, handoff):
    """gamut_hip_jpeg_decode_batch_device folds the verdict on a damaged scan into the per-file status and the return value (no status array
    needed), like the PNG batch call -- the verdict being the REFERENCE's: a scan that ends half-way is an image with a flat rest (decoded again on
    the host behind the device pass), a run past coefficient 63 is JPGD_DECODE_ERROR; the neighbours' pixels are the oracle's"""
    import io
    from PIL import Image
    import gen
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(800, 600, 35)).save(bio, "JPEG", quality=90, subsampling=2)
    good = bio.getvalue()
    cut = good[:len(good) // 2]                                                   # the scan ends half-way
    sos = good.index(b"\xff\xda")
    rng = np.random.default_rng(8)
    bad = None
    for _ in range(64):                                                           # noise until the reference refuses the file
        noisy = bytearray(good)
        for k in rng.integers(sos + 20, len(good) - 2, 300):
            noisy[k] = int(rng.integers(0, 255))
        if O.decompress_jpeg(bytes(noisy), 4) is None:
            bad = bytes(noisy); break
    assert bad is not None
    rc, hst, res = _decode_batch_device(hip, [good, cut, bad, good], 4)
    assert rc == _capi.ERR_DECODE and hst[0] == 0 and hst[3] == 0 and hst[1] == 0 and hst[2] == _capi.ERR_DECODE
    exp = O.decompress_jpeg(good, 4)[0]
    assert np.array_equal(res[0], exp) and np.array_equal(res[3], exp)
    assert np.array_equal(res[1], O.decompress_jpeg(cut, 4)[0])


@pytest.mark.parametrize("scan_type,w,h", [(4, 16384, 17), (4, 17, 16384), (1, 16384, 9), (2, 16383, 8), (0, 9, 16384)])
def test_maximum_dimensions(hip, scan_type, w, h):
    """the reference accepts up to 16384 x 16384 (jpegload.d:101-102): the widest and the tallest frames, every tuned kernel"""
    rng = np.random.default_rng(w + h + scan_type)
    mw, mh = MCU[scan_type]
    nblk = ((w + mw - 1) // mw) * ((h + mh - 1) // mh) * NB[scan_type]
    co = random_coeffs(rng, nblk, "natural")
    comps = 1 if scan_type == 0 else 3
    for rc in (4, 3):
        exp = O.jpeg_reconstruct(w, h, comps, scan_type, co, None, rc)
        got = gpu_reconstruct(hip, w, h, scan_type, co[None], None, rc)[0]
        assert np.array_equal(got, exp)
    L = hip
    assert L.gamut_hip_jpeg_reconstruct_batch_device(1, 0, None, 0, 1, 16385 * 4, 0, 16385, 8, 4, 4, 1, None) == _capi.ERR_INVALID_ARG


def test_device_entropy_decode_many_distinct_tables(hip):
    """more distinct Huffman / quant tables in one batch than a workgroup keeps in LDS (16): the tables are then read from
    global memory; long (multi-lane) and short (one lane) segments both"""
    import io
    from PIL import Image
    import gen
    blobs = []
    for k, q in enumerate((35, 50, 62, 71, 80, 88, 93, 97)):
        big = Image.fromarray(gen.synth_rgb(640, 480, 30 + k)); small = Image.fromarray(gen.synth_rgb(48, 40, 60 + k))
        for im in (big, small):
            bio = io.BytesIO(); im.save(bio, "JPEG", quality=q, subsampling=(0, 1, 2)[k % 3], optimize=True); blobs.append(bio.getvalue())
    rc, hst, st, res = _entropy_decode_device(hip, blobs)
    assert rc == 0 and hst == [0] * len(blobs) and not st.any()
    tables = set()
    for data, (co, zz, info) in zip(blobs, res):
        d = O.DecodedJpeg(data)
        assert np.array_equal(co, d.coeffs) and np.array_equal(zz, d.max_zag)
        i = 0
        while True:                                        # count distinct DHT payloads to be sure the test does what it says
            i = data.find(b"\xff\xc4", i)
            if i < 0:
                break
            n = (data[i + 2] << 8) | data[i + 3]
            tables.add(data[i + 4:i + 2 + n]); i += 2 + n
    assert len(tables) > 16


def test_dropin_decompress_on_the_input_layer_files(hip):
    """gamut_hip_decompress_jpeg_image_from_memory on every file of tests/golden/jpeg_fuzz: NULL exactly where expected.json (the second reading of
    jpegload.d, tools/make_jpeg_fuzz_fixtures.py) says null or undefined, otherwise the oracle's pixels and the expected pixelAspectRatio / dotsPerInchY
    -- the round-4 review's probes among them: EXIF 300 x 150 dpi -> 2.0 / 150, byte order `XX` -> NULL (jpegload.d:1704-1816)."""
    import json
    d = os.path.join(HERE, "golden", "jpeg_fuzz")
    expected = json.load(open(os.path.join(d, "expected.json")))
    libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
    seen = set()
    for name, e in sorted(expected.items()):
        data = open(os.path.join(d, name), "rb").read()
        buf = np.frombuffer(data, np.uint8)
        w, h, ac = C.c_int(), C.c_int(), C.c_int()
        par, dpi = C.c_float(), C.c_float()
        p = hip.gamut_hip_decompress_jpeg_image_from_memory(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ac), C.byref(par), C.byref(dpi), 4)
        assert bool(p) == (e["verdict"] == "image"), (name, hip.gamut_hip_last_error())
        if not p:
            continue
        got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h.value, w.value * 4)).copy()
        libc.free(p)
        want = O.decompress_jpeg(data, 4)
        assert np.array_equal(got, want[0]), name
        exp = tuple(float("nan") if v == "nan" else v for v in (e["pixel_aspect_ratio"], e["dpi_y"]))
        assert O.same_density((par.value, dpi.value), exp), (name, par.value, dpi.value, exp)
        seen.add((str(e["pixel_aspect_ratio"]), str(e["dpi_y"])))
    assert ("2.0", "150.0") in seen and ("nan", "nan") in seen


def test_a_batch_of_nothing_but_host_feeder_files_starts_from_clear_status_words(hip):
    """a batch in which NO baseline file is the kernels' (here count = 1: a file whose scan header ends in the FF D9 padding behind
    the file -- prepare_header hands it to the host feeder) never reached the clear of the device status words; the file-level call then folded the
    caller's uninitialised status_dev into its verdict and turned a file the host feeder had decoded into ERR_DECODE.  status_dev arrives as 0xFF."""
    d = os.path.join(HERE, "golden", "jpeg_fuzz")
    data = open(os.path.join(d, "file_ends_inside_its_sos_r05.jpg"), "rb").read()
    want = O.decompress_jpeg(data, 4)
    assert want is not None
    for n in (1, 3):
        bufs = [np.frombuffer(data, np.uint8)] * n
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[len(data)] * n)
        size = want[0].size
        offs = (np.arange(n) * size).astype(np.int64)
        dout = dev_upload(hip, np.full(n * size + 16, 0xA5, np.uint8))
        dst = dev_upload(hip, np.full(4 * n, 0xFF, np.uint8))
        info = (_capi.JpegFrame * n)(); hst = (C.c_int * n)()
        rc = hip.gamut_hip_jpeg_decode_batch_device(ptrs, lens, n, 4, offs.ctypes.data_as(C.POINTER(C.c_int64)), dout, info, hst, dst, None)
        assert rc == 0 and list(hst) == [0] * n, (rc, list(hst), hip.gamut_hip_last_error())
        out = np.empty(n * size + 16, np.uint8); st = np.empty(n, np.uint32)
        _capi.check(hip.gamut_hip_memcpy_d2h(out.ctypes.data, dout, out.nbytes, None))
        _capi.check(hip.gamut_hip_memcpy_d2h(st.ctypes.data, dst, st.nbytes, None))
        _capi.check(hip.gamut_hip_stream_synchronize(None))
        hip.gamut_hip_device_free(dout); hip.gamut_hip_device_free(dst)
        assert not st.any()
        for k in range(n):
            assert np.array_equal(out[k * size:(k + 1) * size], want[0].reshape(-1)), k
    # the coefficient-level entry point: the same file, the caller's status words pre-filled
    co = dev_upload(hip, np.zeros(36 * 64 * 2 + 64, np.uint8)); zz = dev_upload(hip, np.zeros(64, np.uint8)); dst = dev_upload(hip, np.full(4, 0xFF, np.uint8))
    buf = np.frombuffer(data, np.uint8)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data); lens = (C.c_size_t * 1)(len(data))
    z64 = np.zeros(1, np.int64); info = (_capi.JpegFrame * 1)(); hst = (C.c_int * 1)()
    rc = hip.gamut_hip_jpeg_entropy_decode_device(ptrs, lens, 1, z64.ctypes.data_as(C.POINTER(C.c_int64)), z64.ctypes.data_as(C.POINTER(C.c_int64)), co, zz, dst, info, hst, None)
    st = np.empty(1, np.uint32)
    _capi.check(hip.gamut_hip_memcpy_d2h(st.ctypes.data, dst, 4, None)); _capi.check(hip.gamut_hip_stream_synchronize(None))
    for q in (co, zz, dst):
        hip.gamut_hip_device_free(q)
    assert rc == 0 and hst[0] == 0 and st[0] == 0, (rc, hst[0], st[0])


def test_files_to_pixels_with_an_odd_output_offset(hip):
    """the token hand-off stores rgba8 pixels as dwords; an image whose output is not dword-aligned must take the dense hand-off (whose launch
    falls back to the byte-wise kernel) instead of failing the whole call."""
    import io
    from PIL import Image
    import gen
    bio = io.BytesIO(); Image.fromarray(gen.synth_rgb(256, 160, 5)).save(bio, "JPEG", quality=92, subsampling=2); data = bio.getvalue()
    assert len(data) - data.index(b"\xff\xda") >= 4096            # a long segment: the file would take tokens
    n = 3
    bufs = [np.frombuffer(data, np.uint8)] * n
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[len(data)] * n)
    size = 256 * 160 * 4
    offs = np.array([1, 1 + size + 2, 4 + 2 * (size + 4)], np.int64)       # odd, odd, aligned
    total = int(offs[-1]) + size + 16
    dout = dev_upload(hip, np.full(total, 0xA5, np.uint8))
    info = (_capi.JpegFrame * n)(); hst = (C.c_int * n)()
    rc = hip.gamut_hip_jpeg_decode_batch_device(ptrs, lens, n, 4, offs.ctypes.data_as(C.POINTER(C.c_int64)), dout, info, hst, None, None)
    assert rc == 0, hip.gamut_hip_last_error()
    out = np.empty(total, np.uint8)
    _capi.check(hip.gamut_hip_memcpy_d2h(out.ctypes.data, dout, out.nbytes, None))
    _capi.check(hip.gamut_hip_stream_synchronize(None))
    hip.gamut_hip_device_free(dout)
    want = O.decompress_jpeg(data, 4)[0].reshape(-1)
    for k in range(n):
        assert np.array_equal(out[offs[k]:offs[k] + size], want), k
    assert out[0] == 0xA5 and (out[1 + size:1 + size + 2] == 0xA5).all()
