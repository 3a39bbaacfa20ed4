"""QOIX on the GPU against the serial C restatement of the reference (tests/c/qoix_ref.c, the four deliberate deviations included), byte
for byte: the batched decode over every named case in one call per channel count, refused files among good neighbours, stored-only and
LZ4-only batches, more waves than one round of the grid, rows on either side of the LDS row capacity, every output alignment, the Image
layer and the host drop-in.  Each file sits at the end of its host buffer; output allocations are filled with 0xA5, carry 4 KiB guards
and are compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import qoix_cases
import qoix_gen as G
import qoix_ref_c
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096
RC = {qoix_ref_c.REFUSED: _capi.ERR_DECODE, qoix_ref_c.UNSUPPORTED: _capi.ERR_UNSUPPORTED}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


@pytest.fixture(scope="module")
def CAP(L):
    return L.gamut_hip_qoix_row_capacity()


def _info_words(info):
    return {k: int(v) for k, v in zip(qoix_ref_c.INFO_FIELDS, np.frombuffer(bytes(info), np.int32))}


@pytest.fixture(scope="module")
def expected():
    """the restatement's verdict and pixels per (file, channels), computed once and shared"""
    cache = {}

    def get(f, ch):
        key = (f, ch)
        if key not in cache:
            cache[key] = (qoix_ref_c.header(f), qoix_ref_c.load(f, ch))
            if cache[key][1] is not None:
                cache[key][1][0].setflags(write=False)
        return cache[key]
    return get


def decode_batch(L, expected, files, ch, offsets=None):
    """one gamut_hip_qoix_decode_batch_device call -> (rc, statuses, infos, whole output allocation, offsets, expected allocation, wanted statuses, mask)
    mask: False over the own bytes of a file that is refused on the device (it may leave anything there)"""
    n = len(files)
    exp = [expected(f, ch) for f in files]
    sizes, want = [], []
    for f, ((verdict, hd), loaded) in zip(files, exp):
        early = verdict == qoix_ref_c.OK and hd["compression"] == 1 and hd["orig"] > 255 * (len(f) - 29)        # refused on the host: writes nothing
        want.append(0 if loaded is not None else RC.get(verdict, _capi.ERR_DECODE))
        sizes.append((hd["width"] * hd["height"] * (ch or hd["channels"]), verdict == qoix_ref_c.OK and not early) if verdict == qoix_ref_c.OK else (64, False))
    offs, pos = [], GUARD
    for k, (s, _) in enumerate(sizes):
        if offsets is None:
            pos += 1 + 2 * (k % 8)                                          # odd byte positions, every odd residue mod 16 among them
        else:
            pos = (pos + 15) // 16 * 16 + offsets[k]
        offs.append(pos)
        pos += s + GUARD
        pos += pos & 1
    expect = np.full(pos, 0xA5, np.uint8)
    mask = np.ones(pos, bool)
    for (_, loaded), o, (s, on_device) in zip(exp, offs, sizes):
        if loaded is not None:
            expect[o:o + s] = loaded[0].reshape(-1)
        elif on_device:
            mask[o:o + s] = False
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs])
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.QoixInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_qoix_decode_batch_device(ptrs, lens, n, ch, (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    return rc, list(st), info, out.cpu().numpy(), offs, expect, want, mask, exp


def check_batch(L, expected, files, ch, names=None, offsets=None):
    rc, st, info, got, offs, expect, want, mask, exp = decode_batch(L, expected, files, ch, offsets)
    bad = [i for i, w in enumerate(want) if w]
    assert rc == (want[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for i in range(len(files)):
        assert st[i] == want[i], (i, names[i] if names else None, st[i], want[i])
        assert _info_words(info[i]) == exp[i][0][1], (i, names[i] if names else None)
    same = (got == expect) | ~mask
    if not same.all():                                                      # the WHOLE allocation, guards included
        first = int(np.flatnonzero(~same)[0])
        k = max([i for i in range(len(offs)) if offs[i] - GUARD <= first], default=0)
        assert False, ("channels", ch, "image", k, names[k] if names else None, "first difference at", first - offs[k],
                       "got", got[first:first + 8].tolist(), "want", expect[first:first + 8].tolist())
    return want


@pytest.mark.parametrize("ch", [0, 3, 4])
def test_every_named_case_in_one_batch(L, expected, ch):
    cases = qoix_cases.small_cases()
    want = check_batch(L, expected, [f for _, f, _ in cases], ch, [n for n, _, _ in cases])
    assert [w == 0 for w in want] == [e == "ok" for _, _, e in cases]
    assert sum(w == _capi.ERR_UNSUPPORTED for w in want) >= 8 and sum(w == _capi.ERR_DECODE for w in want) >= 40


def test_refused_files_between_good_neighbours(L, expected):
    cases = qoix_cases.small_cases()
    good = [(n, f) for n, f, e in cases if e == "ok" and len(f) < 2000][::7]
    refused = [(n, f) for n, f, e in cases if e != "ok"]
    files, names = [], []
    for k, (n, f) in enumerate(refused):
        files += [good[k % len(good)][1], f]; names += [good[k % len(good)][0], n]
    files.append(good[0][1]); names.append(good[0][0])
    for ch in (0, 4):
        want = check_batch(L, expected, files, ch, names)
        assert [w != 0 for w in want] == [bool(k & 1) for k in range(len(files))]
    want = check_batch(L, expected, [f for _, f in refused], 3, [n for n, _ in refused])           # nothing but refused files
    assert all(want)


def test_stored_only_lz4_only_and_empty_batches(L, expected):
    cases = [(n, f) for n, f, e in qoix_cases.small_cases() if e == "ok" and len(f) < 3000]
    stored = [(n, f) for n, f in cases if f[16] == 0]
    lz = [(n, f) for n, f in cases if f[16] == 1]
    assert len(stored) > 40 and len(lz) > 20
    for part in (stored, lz, lz[:1], stored[:1]):
        for ch in (0, 3, 4):
            assert not any(check_batch(L, expected, [f for _, f in part], ch, [n for n, _ in part]))
    assert L.gamut_hip_qoix_decode_batch_device(None, None, 0, 0, None, None, None, None, None) == 0
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    f = np.frombuffer(qoix_cases.BASE, np.uint8)
    for ch in (1, 2, 5):
        assert L.gamut_hip_qoix_decode_batch_device((C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), 1, ch, (C.c_int64 * 1)(0), out.data_ptr(), None, None, None) == _capi.ERR_INVALID_ARG
    assert (out.cpu().numpy() == 0xA5).all()


def test_600_tiny_files_are_more_waves_than_one_round_of_the_grid(L, expected):
    rng = np.random.default_rng(11)
    files = []
    for k in range(600):
        w, h, ch = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(3, 5))
        files.append(G.encode(qoix_cases._noisy(w, h, ch, k), lz4=k % 3 == 0))
    files[100] = files[100][:-5] + b"\xe8\xe8\xe8\xe8\xe8"                  # one ADIFF chain off the end in the crowd
    want = check_batch(L, expected, files, 4)
    assert [i for i, w in enumerate(want) if w] in ([100], [])              # (refused unless the image was complete before the chain)
    assert not any(check_batch(L, expected, files[:100] + files[101:], 0))


def test_rows_at_the_lds_capacity_and_one_pixel_wider(L, expected, CAP):
    cases = qoix_cases.row_capacity(CAP)
    assert sorted({qoix_ref_c.header(f)[1]["width"] for _, f, _ in cases}) == [CAP, CAP + 1]
    for ch in (0, 3, 4):
        assert not any(check_batch(L, expected, [f for _, f, _ in cases], ch, [n for n, _, _ in cases]))


def test_all_16_output_residues_with_3_channel_output_in_one_batch(L, expected):
    """rows of 1, 5, 21, 65 and 300 pixels (shorter than a 16-byte piece, head and tail only, several pieces, more than one packing step) x
    out_offset residues 0..15, 3-channel output"""
    files, offsets = [], []
    for r in range(16):
        for w in (1, 5, 21, 65, 300)[r % 2::2] if r < 14 else (1, 5, 21, 65, 300):
            files.append(G.encode(qoix_cases._noisy(w, 3, 3 + (r + w) % 2, r * 1000 + w)))
            offsets.append(r)
    assert not any(check_batch(L, expected, files, 3, offsets=offsets))
    assert {o for o in offsets} == set(range(16))
    assert not any(check_batch(L, expected, files, 4, offsets=offsets))


@pytest.mark.parametrize("device", [False, True])
def test_image_load(L, expected, device):
    import oracle_lib as O
    from gamut_amd import image as gi
    d = {n: f for n, f, _ in qoix_cases.small_cases()}
    names = {9: "rgb8", 12: "rgba8", 15: "rgbap8"}
    files = [d["geometry_65x3_3ch"], d["geometry_65x3_4ch_lz4"], d["colorspace_2_with_4_channels_is_rgbap8"], d["rgba_and_adiff_ops_in_a_3_channel_file"],
             d["header_par_and_dpi_bits_are_kept"], d["photo_like_201x149_rgb_lz4"], G.stored(5, 4, G.RGBA(200, 100, 50, 128) + G.RUN2(9) + G.GRAY(7), 4, par=1.5, dpi=300.0)]
    for f in files:
        ref, info = qoix_ref_c.load(f, 0)
        src = names[info["pixel_type"]]
        for flags in (0, gi.LOAD_GREYSCALE, gi.LOAD_ALPHA, gi.LOAD_RGB | gi.LOAD_NO_ALPHA, gi.LOAD_16BIT, gi.LOAD_GREYSCALE | gi.LOAD_NO_ALPHA, gi.LOAD_NO_PREMUL):
            im = gi.Image(device=device)
            assert im.loadFromMemory(f, flags), im.errorMessage
            want_type = L.gamut_apply_load_flags(O.PT[src], flags)
            assert (im.type, im.width, im.height, im.isDevice) == (want_type, info["width"], info["height"], device)
            if flags == 0:
                assert im.type == info["pixel_type"] and im.pitchInBytes == info["width"] * info["channels"]
            exp = O.scanlines_convert(src, ref.reshape(-1), O.PIXEL_TYPES[want_type], info["width"], info["height"]) if want_type != O.PT[src] else ref
            assert np.array_equal(np.asarray(im.pixels()).reshape(-1).view(np.uint8), np.asarray(exp).reshape(-1).view(np.uint8)), (src, flags)
            bits = np.array([im.pixelAspectRatio, im.dotsPerInchY], np.float32).view(np.int32)
            want_bits = np.array([info["pixel_aspect_ratio"], info["resolution_y"]], np.int32)
            assert np.array_equal(bits, want_bits) or (np.isnan(im.pixelAspectRatio) and info["pixel_aspect_ratio"] == 0x7fc01234), (bits, want_bits)
    for name, msg in (("deviation_3_end_executed", "Image decoding failed"), ("lz4_offset_0_deviation_2", "Image decoding failed"),
                      ("header_width_0", "Image decoding failed"), ("unsupported_8bit_2ch", "Image decoding failed"), ("lz4_truncated_inside_the_literals", "Image decoding failed")):
        im = gi.Image(device=device)
        assert not im.loadFromMemory(d[name]) and im.errorMessage == msg, name
    im = gi.Image(device=device)
    assert not im.loadFromMemory(files[0], gi.LOAD_RGB | gi.LOAD_GREYSCALE) and im.errorMessage == "Invalid image decoding flags"


def test_the_drop_in_against_the_restatement(L):
    cases = [(n, f, e) for n, f, e in qoix_cases.small_cases() if len(f) < 3000][::3]
    assert sum(e == "ok" for _, _, e in cases) > 20 and sum(e != "ok" for _, _, e in cases) > 10
    for name, f, e in cases:
        buf = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            buf[64:] = np.frombuffer(f, np.uint8)
        info, typ = _capi.QoixInfo(), C.c_int(99)
        p = L.gamut_hip_qoix_lz4_decode(buf.ctypes.data + 64, len(f), C.byref(info), 0, C.byref(typ))
        ref = qoix_ref_c.load(f, 0)
        assert (p is not None) == (ref is not None) == (e == "ok"), name
        assert _info_words(info) == qoix_ref_c.header(f)[1], name
        if p is not None:
            got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (ref[0].size,)).copy()
            C.CDLL(None).free(C.c_void_p(p))
            assert np.array_equal(got, ref[0].reshape(-1)) and typ.value == ref[1]["pixel_type"], name
        else:
            assert typ.value == -1
    f = np.frombuffer(qoix_cases.BASE, np.uint8)
    assert L.gamut_hip_qoix_lz4_decode(f.ctypes.data, f.size, None, 0x10000 | 0x80000, None) is None    # LOAD_GREYSCALE | LOAD_RGB: validLoadFlags refuses


def test_kernel_timing_getters(L):
    """-1 unless GAMUT_HIP_QOIX_TIMING=1 was set when the library first decoded; with it, both stages are reported"""
    import os
    f = np.frombuffer(qoix_cases.BASE, np.uint8)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.gamut_hip_qoix_decode_batch_device((C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), 1, 0, (C.c_int64 * 1)(0), out.data_ptr(), None, None, None) == 0
    a, b, t = L.gamut_hip_qoix_last_decode_stage_ms(0), L.gamut_hip_qoix_last_decode_stage_ms(1), L.gamut_hip_qoix_last_decode_kernel_ms()
    if os.environ.get("GAMUT_HIP_QOIX_TIMING") == "1":
        assert a >= 0 and b > 0 and abs(t - (a + b)) < 1e-3
    else:
        assert (a, b, t) == (-1.0, -1.0, -1.0)
