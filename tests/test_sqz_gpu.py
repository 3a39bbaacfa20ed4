"""SQZ on the GPU against the serial C restatement of the reference (tests/c/sqz_ref.c), byte for byte: the reconstruction entry on the
restatement's coefficient planes, the file-level batch call, the Image layer.  Each file sits at the end of its host buffer; output
allocations are filled with 0xA5, carry 4 KiB guards and are compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import sqz_cases
import sqz_ref_c as R
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096
_cache = {}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def expected(f):
    """the restatement's (verdict, info, pixels or None) per file, computed once and shared"""
    if f not in _cache:
        v, info = R.header(f)
        px = R.load(f)[0] if v == R.OK else None
        if px is not None:
            px.setflags(write=False)
        _cache[f] = (v, info, px)
    return _cache[f]


def _info_words(info):
    return {k: int(v) for k, v in zip(R.INFO_FIELDS, np.frombuffer(bytes(info), np.int32))}


def layout(sizes, offsets=None):
    """output offsets: odd byte positions (every odd residue mod 16 among them) unless residues are given -> (offsets, allocation size)"""
    offs, pos = [], GUARD
    for k, s in enumerate(sizes):
        if offsets is None:
            pos += 1 + 2 * (k % 8)
        else:
            pos = (pos + 15) // 16 * 16 + offsets[k]
        offs.append(pos)
        pos += s + GUARD
        pos += pos & 1
    return offs, pos


def compare(got, expect, offs, names=None):
    if not np.array_equal(got, expect):                                     # the WHOLE allocation, guards included
        first = int(np.flatnonzero(got != expect)[0])
        k = max([i for i in range(len(offs)) if offs[i] - GUARD <= first], default=0)
        assert False, ("image", k, names[k] if names else None, "first difference at", first - offs[k], "got", got[first:first + 8].tolist(),
                       "want", expect[first:first + 8].tolist())


def check_files(L, files, names=None, offsets=None):
    """one gamut_hip_sqz_decode_batch_device call, everything compared; -> the statuses wanted"""
    n = len(files)
    exp = [expected(f) for f in files]
    sizes = [px.size if px is not None else 64 for _, _, px in exp]
    want = [0 if v == R.OK else _capi.ERR_DECODE for v, _, _ in exp]
    offs, total = layout(sizes, offsets)
    expect = np.full(total, 0xA5, np.uint8)
    for (_, _, px), o, s in zip(exp, offs, sizes):
        if px is not None:
            expect[o:o + s] = px.reshape(-1)
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs])
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.SqzInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_decode_batch_device(ptrs, lens, n, (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    bad = [i for i, w in enumerate(want) if w]
    assert rc == (want[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for i in range(n):
        assert st[i] == want[i], (i, names[i] if names else None, st[i], want[i])
        assert _info_words(info[i]) == exp[i][1], (i, names[i] if names else None)
    compare(out.cpu().numpy(), expect, offs, names)
    return want


def check_planes(L, items, names=None):
    """one gamut_hip_sqz_reconstruct_batch_device call on [(coefficients, w, h, mode, levels)], at odd output offsets"""
    n = len(items)
    want = [R.pixels(co, w, h, m, lv) for co, w, h, m, lv in items]
    offs, total = layout([p.size for p in want])
    expect = np.full(total, 0xA5, np.uint8)
    for p, o in zip(want, offs):
        expect[o:o + p.size] = p.reshape(-1)
    descs = (_capi.SqzDesc * n)()
    parts, pos = [], 3                                                      # planes at odd element offsets, a gap between images
    for k, (co, w, h, m, lv) in enumerate(items):
        descs[k].width, descs[k].height, descs[k].color_mode, descs[k].levels, descs[k].coeff_offset = w, h, m, lv, pos
        parts.append((pos, co))
        pos += co.size + 5 + 2 * (k % 3)
    host = np.full(pos, 0x5A5A, np.uint16).view(np.int16)
    for p, co in parts:
        host[p:p + co.size] = co
    dco = torch.from_numpy(host.copy()).cuda()
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_reconstruct_batch_device(dco.data_ptr(), descs, n, (C.c_int64 * n)(*offs), out.data_ptr(), st, None)
    torch.cuda.synchronize()
    assert rc == 0, L.gamut_hip_last_error()
    assert list(st) == [0] * n
    compare(out.cpu().numpy(), expect, offs, names)


def test_reconstruct_every_geometry_mode_and_level_count_in_one_batch(L):
    cases = [(n, f) for n, f, e in sqz_cases.small_cases() if e == "ok"]
    items = []
    for _, f in cases:
        co, info = R.coeffs(f)
        items.append((co, info["width"], info["height"], info["color_mode"], info["levels"]))
    assert {(i[3]) for i in items} == {0, 1, 2, 3} and {i[4] for i in items} >= {1, 2, 3, 4, 5}
    check_planes(L, items, [n for n, _ in cases])
    check_planes(L, items[5:6])                                             # a batch of one


@pytest.mark.parametrize("w,h", [(16, 16), (19, 23)])
def test_reconstruct_extreme_coefficients(L, w, h):
    """+-32767 in sign-magnitude (0xFFFE / 0xFFFF), alternating signs, checkerboards and random bits: the 16-bit wraps of both lifting passes
    (the untruncated ints inside the reference's row loop against the shorts of its tail) and the Oklab 64-bit products"""
    rng = np.random.default_rng(w * 100 + h)
    items = []
    for mode in range(4):
        n = (1 if mode == 0 else 3) * w * h
        idx = np.arange(n)
        for k, co in enumerate((np.where(idx & 1, 0xFFFF, 0xFFFE), np.where((idx // w + idx) & 1, 0xFFFE, 0xFFFF), np.full(n, 0xFFFE), np.full(n, 0xFFFF),
                                np.where(idx % 3 == 0, 0xFFFE, 1), rng.integers(0, 65536, n), rng.integers(0, 65536, n) | 0xC000, np.where(idx & 2, 0x8000, 0x7FFF))):
            items.append((co.astype(np.uint16).view(np.int16), w, h, mode, 1))
    check_planes(L, items)


def test_reconstruct_refuses_a_bad_descriptor_among_good_ones(L):
    cases = [f for _, f, e in sqz_cases.small_cases() if e == "ok"][:3]
    co = [R.coeffs(f) for f in cases]
    host = np.concatenate([c for c, _ in co])
    dco = torch.from_numpy(host).cuda()
    descs = (_capi.SqzDesc * 3)()
    pos = 0
    for k, (c, i) in enumerate(co):
        descs[k].width, descs[k].height, descs[k].color_mode, descs[k].levels, descs[k].coeff_offset = i["width"], i["height"], i["color_mode"], i["levels"], pos
        pos += c.size
    descs[1].levels = 4                                                     # more than the size admits
    sizes = [R.load(f)[0].size for f in cases]
    offs, total = layout(sizes)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = (C.c_int * 3)(77, 77, 77)
    rc = L.gamut_hip_sqz_reconstruct_batch_device(dco.data_ptr(), descs, 3, (C.c_int64 * 3)(*offs), out.data_ptr(), st, None)
    torch.cuda.synchronize()
    assert rc == _capi.ERR_INVALID_ARG and list(st) == [0, _capi.ERR_INVALID_ARG, 0] and L.gamut_hip_last_error().startswith(b"image 1:")
    expect = np.full(total, 0xA5, np.uint8)
    for k in (0, 2):
        expect[offs[k]:offs[k] + sizes[k]] = R.load(cases[k])[0].reshape(-1)
    compare(out.cpu().numpy(), expect, offs)


def test_every_named_case_in_one_batch(L):
    cases = sqz_cases.small_cases()
    want = check_files(L, [f for _, f, _ in cases], [n for n, _, _ in cases])
    assert [w == 0 for w in want] == [e == "ok" for _, _, e in cases]
    assert sum(w == _capi.ERR_DECODE for w in want) >= 15


def test_refused_files_between_good_neighbours_and_alone(L):
    cases = sqz_cases.small_cases()
    good = [(n, f) for n, f, e in cases if e == "ok" and len(f) < 3000][::5]
    refused = [(n, f) for n, f, e in cases if e != "ok"]
    files, names = [], []
    for k, (n, f) in enumerate(refused):
        files += [good[k % len(good)][1], f]; names += [good[k % len(good)][0], n]
    files.append(good[0][1]); names.append(good[0][0])
    want = check_files(L, files, names)
    assert [w != 0 for w in want] == [bool(k & 1) for k in range(len(files))]
    assert all(check_files(L, [f for _, f in refused], [n for n, _ in refused]))      # nothing but refused files


def test_empty_batch_and_bad_arguments(L):
    assert L.gamut_hip_sqz_decode_batch_device(None, None, 0, None, None, None, None, None) == 0
    assert L.gamut_hip_sqz_reconstruct_batch_device(None, None, 0, None, None, None, None) == 0
    assert L.gamut_hip_sqz_decode_batch_device(None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_reconstruct_batch_device(None, None, -1, None, None, None, None) == _capi.ERR_INVALID_ARG


def test_600_tiny_files(L):
    files = sqz_cases.tiny_files(600)
    assert not any(check_files(L, files))


def test_all_16_output_residues(L):
    files, offsets = [], []
    for r in range(16):
        for k, (w, h) in enumerate(((16, 16), (21, 17), (130, 16))):
            files.append(sqz_cases.make(w, h, (r + k) % 4, 1, (r + k) % 4, r & 1, seed=2000 + r * 3 + k))
            offsets.append(r)
    assert not any(check_files(L, files, offsets=offsets))


def test_every_prefix_of_a_small_file_as_one_batch(L):
    grey, oklab = sqz_cases.prefix_files()
    assert not any(check_files(L, sqz_cases.prefixes(oklab)))
    assert not any(check_files(L, sqz_cases.prefixes(grey, 3)))


def test_2048x2048_with_8_levels(L):
    assert not any(check_files(L, [sqz_cases.big_case()]))


@pytest.mark.parametrize("device", [False, True])
def test_image_load(L, device):
    import oracle_lib as O
    from gamut_amd import image as gi
    d = {n: f for n, f, _ in sqz_cases.small_cases()}
    names = {0: "l8", 9: "rgb8"}
    files = [d["mode_grey_scan_snake"], d["mode_oklab_scan_hilbert"], d["geometry_19x23_1_levels_ycocg"], d["geometry_47x32_2_levels_logl1"], d["budget_40_oklab"],
             d["geometry_128x72_4_levels_oklab"], d["hand_ends_inside_a_refinement_pass"]]
    for f in files:
        _, info, ref = expected(f)
        src = names[info["pixel_type"]]
        for flags in (0, gi.LOAD_GREYSCALE, gi.LOAD_ALPHA, gi.LOAD_RGB | gi.LOAD_NO_ALPHA, gi.LOAD_16BIT, gi.LOAD_GREYSCALE | gi.LOAD_NO_ALPHA, gi.LOAD_NO_PREMUL):
            im = gi.Image(device=device)
            assert im.loadFromMemory(f, flags), im.errorMessage
            want_type = L.gamut_apply_load_flags(O.PT[src], flags)
            assert (im.type, im.width, im.height, im.isDevice) == (want_type, info["width"], info["height"], device)
            if flags == 0:
                assert im.type == info["pixel_type"] and im.pitchInBytes == info["width"] * info["planes"]
            exp = O.scanlines_convert(src, ref.reshape(-1), O.PIXEL_TYPES[want_type], info["width"], info["height"]) if want_type != O.PT[src] else ref
            assert np.array_equal(np.asarray(im.pixels()).reshape(-1).view(np.uint8), np.asarray(exp).reshape(-1).view(np.uint8)), (src, flags)
            assert im.pixelAspectRatio == -1.0 and im.dotsPerInchY == -1.0
    for name in ("header_length_6", "header_side_7", "header_side_15_two_levels", "header_width_65536"):
        im = gi.Image(device=device)
        assert not im.loadFromMemory(d[name]) and im.errorMessage == "I/O failure while decoding image", name
    im = gi.Image(device=device)
    assert not im.loadFromMemory(d["header_wrong_magic"]) and im.errorMessage == "Unidentified image format"      # 0xA4: not an SQZ file, and no TGA header either
    assert L.gamut_identify_format_from_memory(np.frombuffer(files[0], np.uint8).ctypes.data, len(files[0])) == gi.FORMAT_SQZ == 9
