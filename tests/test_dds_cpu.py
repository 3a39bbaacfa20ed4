"""DDS / BC7 encode without a GPU: the serial C restatement (tests/c/bc7_ref.c) against hand-derived blocks, against an independent
decoder (tests/bc7_decode.py) and against its own trace; the computed tables; the header; the bound; argument validation and the
no-device behaviour of every new entry; the Image layer's refusals; and the coverage floor of the inputs the GPU tests reuse."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import bc7_decode
import bc7_ref_c
import dds_cases as cases
from gamut_amd import _capi

REFERENCE = "/root/reference/source/gamut/codecs/bc7enc16.d"            # where the reference tree lies when it is present (tools/d_scanline_exec.py)


@pytest.fixture(scope="module")
def restated():
    tiles = cases.all_tiles()
    blocks, traces = bc7_ref_c.blocks(tiles)
    return tiles, blocks, traces


def _two_colour_tile(a, b, pattern):
    return np.array([b if bit else a for bit in pattern], np.uint8)


def test_hand_derived_blocks():
    """worked out from the reference text, not from the restatement's output"""
    # sixteen (0, 0, 0, 0): the alpha path, mode 6, every field zero
    assert bc7_ref_c.block(np.zeros((16, 4)))[0].hex() == "40" + "00" * 15
    # sixteen (255, 255, 255, 255): mode 6, endpoints 127 with both p-bits 1, selectors 0
    assert bc7_ref_c.block(np.full((16, 4), 255))[0].hex() == "c0ffffffffffffff01" + "00" * 7
    # pixel 0 is (0, 0, 0, 254), the rest (1, 1, 1, 255): both colours are mode-6 endpoints ((0, 0, 0, 127) p 0 and (0, 0, 0, 127) p 1),
    # found by the PCA fit with error 0 (the early return).  Pixel 0 takes selector 0; the others take 8, the first weight (34) at which
    # (1 * w + 32) >> 6 is 1 and (254 * (64 - w) + 255 * w + 32) >> 6 is 255.  Bits: mode at 0..6; r, g, b endpoints zero up to bit 48;
    # alpha 127, 127 at 49..62; p-bits 0, 1 at 63, 64; selector 0 in 3 bits at 65; then fifteen nibbles of 8.
    t = np.full((16, 4), (1, 1, 1, 255), np.uint8)
    t[0] = (0, 0, 0, 254)
    blk, tr = bc7_ref_c.block(t)
    assert blk.hex() == "400000000000fe7f81" + "88" * 7 and tr.alpha and tr.early_zero and tr.error == 0
    # partition 0 (columns 2 and 3 are subset 1) in (4, 4, 129) and white.  Mode 6 cannot hold (4, 4, 129): its p-bit is shared by the
    # channels.  Mode 1: the estimate of partition 0 is 0, both subsets are one colour.  Table: 4 with p-bit 0 is (lo 1, hi 1), 129 with
    # p-bit 0 is (20, 63) -- the first lo for which 46 * low + 18 * high + 32 reaches 129 * 64 is 80 = 20 << 2, with high 253 -- and 255
    # with p-bit 1 is (63, 63); all exact, so p-bits 0 and 1 and error 0.  Every selector is 2, no anchor flips.  Bits: 01 mode, 000000
    # partition, then per channel lo0 hi0 lo1 hi1 in 6 bits: r and g 1, 1, 63, 63; b 20, 63, 63, 63; p-bits 0, 1; selectors 10 (anchor),
    # fourteen times 010, 10 (anchor 15).
    t = _two_colour_tile((4, 4, 129, 255), (255, 255, 255, 255), bc7_decode.PARTITIONS[0])
    blk, tr = bc7_ref_c.block(t)
    assert blk.hex() == "0241f0ff41f0ffd4ffff2a4992244992"
    assert tr.mode == 1 and tr.partition == 0 and tr.single_colour and tr.mode1_won and tr.error == 0


def test_every_restated_block_decodes_to_its_own_error(restated):
    tiles, blocks, traces = restated
    for i, (tile, blk) in enumerate(zip(tiles, blocks)):
        t = traces[i]
        mode = bc7_decode.mode_of(blk)
        assert mode == t.mode and mode in (1, 6), i
        has_alpha = bool((tile[:, 3] < 255).any())
        assert bool(t.alpha) == has_alpha and not (has_alpha and mode == 1), i
        dec = bc7_decode.decode(blk)
        # an opaque tile is weighed on r, g, b alone, as the encoder weighs it (mode 6 may then leave alpha at 254)
        assert bc7_decode.perceptual_error(dec, tile, has_alpha) == t.error, i
        if mode == 1:
            assert (dec[:, 3] == 255).all(), i
    solid = cases.solid_greys()
    for tile, blk in zip(solid, bc7_ref_c.blocks(solid)[0]):
        assert np.array_equal(bc7_decode.decode(blk)[:, :3], tile[:, :3])     # every grey is a mode-6 endpoint


def test_coverage_floor(restated):
    """the committed generators reach every path the trace names, and partitions from all three ranges of the scan"""
    _, _, traces = restated
    n = len(cases.all_tiles())
    assert n >= 1000
    seen = {f: sum(getattr(traces[i], f) for i in range(n)) for f in bc7_ref_c.FLAGS}
    assert all(seen[f] > 0 for f in bc7_ref_c.FLAGS), seen
    assert any(traces[i].mode1_tried and not traces[i].mode1_won for i in range(n))
    iters = [traces[i].partition_iter for i in range(n) if traces[i].mode == 1]
    assert any(0 <= k <= 13 for k in iters) and any(14 <= k <= 34 for k in iters) and any(35 <= k <= 63 for k in iters)
    assert len({traces[i].partition for i in range(n) if traces[i].mode == 1}) >= 24


def test_computed_tables():
    t = bc7_ref_c.table()
    assert [tuple(x) for x in t[255]] == [(4, 63, 63), (0, 63, 63)] and tuple(t[254][1]) == (0, 63, 62)
    assert [tuple(x) for x in t[0]] == [(0, 0, 0), (4, 0, 0)]
    if not os.path.exists(REFERENCE):
        pytest.skip("the reference tree is not here")
    text = open(REFERENCE).read()
    m = re.search(r"g_bc7_mode_1_optimal_endpoints =\s*\[(.*?)\n\];", text, re.S)
    want = np.array(re.findall(r"endpoint_err\((\d+), (\d+), (\d+)\)", m.group(1)), dtype=np.int32).reshape(256, 2, 3)
    assert np.array_equal(t, want)
    for name, got in zip(("g_bc7_weights3x", "g_bc7_weights4x"), bc7_ref_c.weight_tables()):
        m = re.search(name + r" =\s*\[(.*?)\];", text, re.S)
        want = np.array([float(x) for x in re.findall(r"([\d.]+)f", m.group(1))], np.float32).reshape(-1, 4)
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (4096, 3)])
def test_header_fields(w, h):
    f = bc7_ref_c.write_dds(np.zeros((h, w, 3), np.uint8))
    bw, bh = (w + 3) // 4, (h + 3) // 4
    assert len(f) == 148 + 16 * bw * bh == bc7_ref_c.dds_size(w, h)
    assert f[:4] == b"DDS "
    d = struct.unpack("<31I", f[4:128])                                     # DDSURFACEDESC2
    want = [0] * 31
    want[0], want[1], want[2], want[3], want[4] = 124, 0x81007, h, w, 16 * bw * bh
    want[18], want[19], want[20] = 32, 4, struct.unpack("<I", b"DX10")[0]   # ddpfPixelFormat: dwSize, DDPF_FOURCC, dwFourCC
    want[26] = 0x1000                                                       # ddsCaps.dwCaps
    assert list(d) == want
    assert struct.unpack("<5I", f[128:148]) == (98, 3, 0, 1, 0)              # DDS_HEADER_DXT10


def test_gather_of_the_four_source_types():
    """l8 -> (v, v, v, 255), la8 -> (v, v, v, a), rgb8 -> (r, g, b, 255), rgba8 as it is; outside the image (0, 0, 0, 0)"""
    rgba = cases.image(8, 8, 4, 5)
    assert bc7_ref_c.write_dds(rgba)[148:] == bc7_ref_c.blocks(cases.tiles_of(rgba))[0].tobytes()
    la = cases.image(8, 4, 2, 6)
    as_rgba = np.stack([la[:, :, 0]] * 3 + [la[:, :, 1]], axis=2)
    assert bc7_ref_c.write_dds(la)[148:] == bc7_ref_c.blocks(cases.tiles_of(as_rgba))[0].tobytes()
    grey = cases.image(4, 8, 1, 7)
    as_rgba = np.concatenate([np.repeat(grey, 3, axis=2), np.full((8, 4, 1), 255, np.uint8)], axis=2)
    assert bc7_ref_c.write_dds(grey)[148:] == bc7_ref_c.blocks(cases.tiles_of(as_rgba))[0].tobytes()
    assert bc7_ref_c.write_dds(grey[:, :, 0]) == bc7_ref_c.write_dds(grey)
    rgb = cases.image(5, 3, 3, 8)                                           # edge tiles: padded with transparent black, so the alpha path
    pad = np.zeros((4, 8, 4), np.uint8)
    pad[:3, :5, :3] = rgb; pad[:3, :5, 3] = 255
    f = bc7_ref_c.write_dds(rgb)
    assert f[148:] == bc7_ref_c.blocks(cases.tiles_of(pad))[0].tobytes()
    assert all(bc7_decode.mode_of(f[148 + 16 * k:164 + 16 * k]) == 6 for k in range(2))
    flipped = np.ascontiguousarray(rgb[::-1])[::-1]                         # a negative row stride
    assert flipped.strides[0] < 0 and bc7_ref_c.write_dds(flipped) == f


def test_bound_values_and_refusals():
    L = _capi.lib()
    b = L.gamut_hip_dds_encode_bound
    for w, h in ((1, 1), (4, 4), (5, 7), (4096, 3), (257, 131), (65536, 65536 // 32)):
        for comp in (1, 2, 3, 4):
            assert b(w, h, comp) == 148 + 16 * ((w + 3) // 4) * ((h + 3) // 4) == bc7_ref_c.dds_size(w, h)
    for w, h, comp in ((0, 4, 3), (4, 0, 3), (-1, 4, 3), (4, -5, 4), (4, 4, 0), (4, 4, 5), (4, 4, -1)):
        assert b(w, h, comp) == 0
    assert b(46340, 46340, 4) == 148 + 16 * 11585 * 11585                   # 2147395748: the largest square below the limit
    assert b(46344, 46344, 4) == 0 and b(2 ** 31 - 1, 2 ** 31 - 1, 1) == 0
    assert b(2 ** 31 - 1, 1, 1) == 0                                        # 148 + 16 * 2^29 is above 2^31 - 1
    assert b(2 ** 29 - 40, 1, 1) == 148 + 16 * ((2 ** 29 - 40 + 3) // 4)


def _batch_args(src, w, h, comp, out):
    a = lambda t, v: (t * 1)(v)
    return dict(src=a(C.c_void_p, src), pitch=a(C.c_int64, w * comp), w=a(C.c_int32, w), h=a(C.c_int32, h), c=a(C.c_int32, comp),
                off=a(C.c_int64, 0), out=out, n=a(C.c_int64, -77), st=a(C.c_int, -77))


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    enc = L.gamut_hip_dds_encode_batch_device
    assert enc(None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert enc(None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK
    px = np.arange(4 * 3 * 4, dtype=np.uint8)
    out = np.full(512, 0xA5, np.uint8)
    a = _batch_args(px.ctypes.data, 4, 3, 4, out.ctypes.data)
    full = [a["src"], a["pitch"], a["w"], a["h"], a["c"], 1, a["off"], a["out"], a["n"], a["st"], None]
    for missing in (0, 1, 2, 3, 4, 6, 7, 8):                                # every required pointer in turn; status may be NULL
        args = list(full)
        args[missing] = None
        assert enc(*args) == _capi.ERR_INVALID_ARG, missing
        assert b"bad arguments" in L.gamut_hip_last_error()
    assert (out == 0xA5).all() and a["n"][0] == -77 and a["st"][0] == -77
    blocks = L.gamut_hip_bc7_encode_blocks_device
    assert blocks(None, 0, None, None) == _capi.OK
    for args in ((px.ctypes.data, -1, out.ctypes.data), (None, 1, out.ctypes.data), (px.ctypes.data, 1, None), (px.ctypes.data, 2 ** 31, out.ctypes.data)):
        assert blocks(*args, None) == _capi.ERR_INVALID_ARG and b"bad arguments" in L.gamut_hip_last_error()
    assert (out == 0xA5).all()
    n = C.c_int(-77)
    for args in ((None, 16, 4, 3, 4), (px.ctypes.data, 16, 0, 3, 4), (px.ctypes.data, 16, 4, 0, 4), (px.ctypes.data, 16, 4, 3, 5), (px.ctypes.data, 16, 4, 3, 0)):
        assert not L.gamut_hip_dds_write_to_mem(*args, C.byref(n)) and n.value == -77
        assert b"invalid arguments" in L.gamut_hip_last_error()
    assert not L.gamut_hip_dds_write_to_mem(px.ctypes.data, 16, 4, 3, 4, None)


def test_every_new_entry_reports_no_device_and_touches_nothing():
    """ERR_NO_DEVICE (NULL from the host drop-in and the Image entries), the message, and every output exactly as the caller left it"""
    from gamut_amd import image as gi
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = (np.arange(4 * 3 * 4) % 251).astype(np.uint8)
    px0 = px.copy()
    out = np.full(4096, 0xA5, np.uint8)                                     # stands for the device output: never dereferenced without a device
    a = _batch_args(px.ctypes.data, 4, 3, 4, out.ctypes.data)
    n = C.c_int(-77)
    im = gi.Image()
    assert im.createView(px, 4, 3, 12, 16)
    calls = [("dds_encode_batch_device", lambda: L.gamut_hip_dds_encode_batch_device(a["src"], a["pitch"], a["w"], a["h"], a["c"], 1, a["off"], a["out"],
                                                                                     a["n"], a["st"], None), _capi.ERR_NO_DEVICE),
             ("bc7_encode_blocks_device", lambda: L.gamut_hip_bc7_encode_blocks_device(px.ctypes.data, 0 + 1, out.ctypes.data, None), _capi.ERR_NO_DEVICE),
             ("dds_write_to_mem", lambda: L.gamut_hip_dds_write_to_mem(px.ctypes.data, 16, 4, 3, 4, C.byref(n)), None),
             ("image_save_dds_to_memory", lambda: im.save_dds_to_memory(), None)]
    for name, call, want in calls:
        L.gamut_hip_scanlines_convert_device(-1, out.ctypes.data, 4, 0, 12, out.ctypes.data, 4, 0, 1, 1, 1, None)      # leaves another message behind
        assert b"no HIP device" not in L.gamut_hip_last_error()
        rc = call()
        assert (rc == want) if want is not None else not rc, name
        assert b"no HIP device" in L.gamut_hip_last_error(), name
        assert (out == 0xA5).all() and a["n"][0] == -77 and a["st"][0] == -77 and n.value == -77, name
        assert np.array_equal(px, px0) and im.isValid and im.errorMessage is None, name
    assert L.gamut_hip_dds_last_encode_kernel_ms() == -1.0


def test_image_entries_refuse_other_types_and_errored_images(tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    assert gi.FORMAT_DDS == 4
    for t in ("l16", "rgba16", "rgbaf32", "lap8", "rgbap8", "rgb16", "lf32"):
        im = gi.Image()
        assert im.create(5, 4, O.PT[t])
        before = np.asarray(im.pixels()).copy()
        assert im.save_dds_to_memory() is None and im.saveDDSToMemory() is None and not im.saveDDSToFile(tmp_path / "x.dds")
        assert im.isValid and im.errorMessage is None and not (tmp_path / "x.dds").exists()
        assert im.type == O.PT[t] and np.array_equal(np.asarray(im.pixels()), before)
    fresh = gi.Image()                                                      # "Uninitialized image": an error state
    message = fresh.errorMessage
    assert fresh.isError and fresh.save_dds_to_memory() is None and not fresh.saveDDSToFile(tmp_path / "y.dds")
    assert fresh.isError and fresh.errorMessage == message and not (tmp_path / "y.dds").exists()
    nodata = gi.Image()
    assert nodata.createWithNoData(5, 4, O.PT["rgba8"]) and nodata.save_dds_to_memory() is None
    assert nodata.isValid and not nodata.hasData
    L = gi.lib()
    n = C.c_size_t(55)
    assert not L.gamut_image_save_dds_to_memory(None, 0, C.byref(n)) and n.value == 0
    ok = gi.Image()
    assert ok.create(5, 4, O.PT["rgba8"])
    assert not L.gamut_image_save_dds_to_memory(ok.h, 0, None) and not L.gamut_image_save_dds_to_file(ok.h, None, 0)
    assert ok.save_to_memory(gi.FORMAT_DDS) is None and not ok.saveToFile(gi.FORMAT_DDS, tmp_path / "z.dds")      # the generic entries do not dispatch DDS
    assert not (tmp_path / "z.dds").exists() and ok.isValid
    assert L.gamut_identify_format_from_memory(b"DDS " + bytes(200), 204) == gi.FORMAT_UNKNOWN                  # and nothing identifies one
