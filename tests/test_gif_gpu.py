"""GIF on the GPU against the serial C restatement of the reference (tests/c/gif_ref.c), byte for byte: every generated case of
tests/gif_cases.py (LZW, geometry, compositing) in batched calls with guards around every slot, refused files in the batch, one call of
256 mutated files, the Image layer (host and device storage, load flags), and one 640 x 480 file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gif_cases
import gif_ref_c
from gamut_amd import _capi
from test_gif_cpu import FIXTURE, lib_header, ref_header

pytestmark = pytest.mark.gpu
GUARD = 1024


@pytest.fixture(scope="module")
def L(hip):
    return hip


def decode_batch(L, files, capacity=None, odd_offsets=False):
    """one gamut_hip_gif_decode_batch_device call -> (rc, statuses, infos, whole output allocation, offsets, expected allocation, refs);
    capacity: {file number: bytes} for slots that are given less room than they need"""
    n = len(files)
    refs = [gif_ref_c.load(f) for f in files]
    capacity = capacity or {}
    offs, caps, pos = [], [], GUARD
    needs = [r[0].size if r is not None else _room_for_a_refused_file(f) for r, f in zip(refs, files)]
    for i, (r, need) in enumerate(zip(refs, needs)):
        offs.append(pos + (i % 4 if odd_offsets else 0))
        caps.append(capacity.get(i, need))
        pos += need + GUARD
    expect = np.full(pos, 0xA5, np.uint8)
    for i, (r, o) in enumerate(zip(refs, offs)):
        if r is not None and i not in capacity:
            expect[o:o + r[0].size] = r[0].reshape(-1)
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs])
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    offa = (C.c_int64 * n)(*offs); capa = (C.c_int64 * n)(*caps)
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.GifInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_gif_decode_batch_device(ptrs, lens, n, offa, capa, out.data_ptr(), info, st, None)
    return rc, list(st), info, out.cpu().numpy(), offs, expect, refs, needs


def _room_for_a_refused_file(f):
    """A refused file's slot: what its container could claim at most (screen size x one layer per image separator byte), so that the
    capacity test passes, the verdict is the decoder's, and a decoder that missed it would still write inside the allocation."""
    if len(f) < 10 or f[:6] not in (b"GIF87a", b"GIF89a"):
        return 64
    w, h = int.from_bytes(f[6:8], "little"), int.from_bytes(f[8:10], "little")
    assert w * h <= 100 * 70
    return max(64, w * h * 4 * f.count(b"\x2C"))


def check_batch(L, files, names, capacity=None, odd_offsets=False):
    rc, st, info, got, offs, expect, refs, needs = decode_batch(L, files, capacity, odd_offsets)
    capacity = capacity or {}
    want = [_capi.ERR_DECODE if r is None else _capi.ERR_INVALID_ARG if i in capacity else 0 for i, r in enumerate(refs)]
    assert st == want, [(names[i], s, w) for i, (s, w) in enumerate(zip(st, want)) if s != w]
    bad = [s for s in st if s]
    assert rc == (bad[0] if bad else 0), (rc, L.gamut_hip_last_error())
    for i, r in enumerate(refs):
        assert (st[i] == _capi.ERR_DECODE) == (lib_header(files[i]) is None), names[i]      # the kernel's verdict and the host code walk agree
        if r is None:
            continue
        f6 = (info[i].width, info[i].height, info[i].layers, info[i].is_gif89, np.float32(info[i].pixel_aspect_ratio), np.float32(info[i].fps))
        assert f6 == ref_header(files[i]), names[i]
    if not np.array_equal(got, expect):                                     # the WHOLE allocation, guards included
        for i, n in enumerate(needs):
            a, b = got[offs[i] - GUARD:offs[i] + n + GUARD], expect[offs[i] - GUARD:offs[i] + n + GUARD]
            assert np.array_equal(a, b), (names[i], "first difference at byte", int(np.flatnonzero(a != b)[0]) - GUARD, "of", n)
        assert False, "difference outside every file's slot and its guards"
    return refs


def _group(prefixes):
    sel = [(n, f) for n, f, _ in gif_cases.cases() if n.startswith(prefixes)]
    assert sel
    return [n for n, _ in sel], [f for _, f in sel]


LZW = ("lzw_cs", "kwkwk", "flat_", "noise_fills", "deferred_", "several_clears", "no_clear", "avail_after", "code_above", "no_end_code",
       "data_after_end", "one_byte", "payload_", "truncated_", "no_trailer", "lzw_cs_13")
GEOMETRY = ("interlaced_", "frame_", "overhang_", "no_colour_table", "lct_only", "zero_")
COMPOSITING = ("disposal_", "mixed_", "transparency_", "later_frame", "first_frame", "gce_after", "stale_lct", "index_past", "transparent_index",
               "zero_frames", "extensions_", "unknown_ext", "bad_gce")


def test_every_case_is_in_a_group():
    names = {n for n, _, _ in gif_cases.cases()}
    assert names == set(_group(LZW)[0]) | set(_group(GEOMETRY)[0]) | set(_group(COMPOSITING)[0])


@pytest.mark.parametrize("group", [LZW, GEOMETRY, COMPOSITING], ids=["lzw", "geometry", "compositing"])
def test_cases_against_the_reference(L, group):
    names, files = _group(group)
    refs = check_batch(L, files, names)
    assert any(r is None for r in refs) and sum(r is not None for r in refs) > len(refs) // 2


def test_cases_one_file_per_call(L):
    """the statuses and pixels do not depend on the batch around a file: a few cases alone, at byte offsets that are no multiple of 4"""
    by_name = {n: f for n, f, _ in gif_cases.cases()}
    for name in ("interlaced_h3_y3", "disposal_2", "first_frame_sees_last_gce", "avail_after_clear", "zero_frames", "flat_300x40"):
        check_batch(L, [by_name[name]] * 2, [name, name], odd_offsets=True)


def test_mixed_batch_with_refused_files_and_a_small_slot(L):
    cases = gif_cases.cases()
    sel = [c for c in cases if c[0].startswith("interlaced_h")][::2] + [c for c in cases if c[0].startswith(("disposal_", "lzw_cs", "stale", "index_past", "overhang", "frame_",
                                                                                                          "transparen", "first_frame", "later_frame"))]
    names = [n for n, _, _ in sel]; files = [f for _, f, _ in sel]
    names.insert(3, "empty"); files.insert(3, b"")
    names.insert(11, "damaged"); files.insert(11, files[5][:len(files[5]) // 2])
    names.insert(20, "fixture"); files.insert(20, FIXTURE)
    assert 38 <= len(files) <= 48
    small = {7: gif_ref_c.load(files[7])[0].size - 1, 20: 100 * 100 * 4 * 3}
    first = check_batch(L, files, names, capacity=small)
    again = check_batch(L, files, names, capacity=small)                     # the same call twice (the staging buffers are reused)
    assert [r is None for r in first] == [r is None for r in again]
    rc, st, info, got, offs, expect, refs, _ = decode_batch(L, files, capacity=small)
    assert rc == _capi.ERR_DECODE and L.gamut_hip_last_error().startswith(b"image 3:")
    assert st[7] == st[20] == _capi.ERR_INVALID_ARG and info[20].layers == 4 and info[20].width == 100


def test_count_zero(L):
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.gamut_hip_gif_decode_batch_device(None, None, 0, None, None, out.data_ptr(), None, None, None) == _capi.OK
    assert bool((out == 0xA5).all())


def test_fuzz_256_mutated_files(L):
    files = gif_cases.mutated(256, seed=21)
    names = [f"mutated_{k}" for k in range(256)]
    refs = check_batch(L, files, names)
    n_bad = sum(r is None for r in refs)
    assert n_bad >= 26 and 256 - n_bad >= 26, n_bad


def _image_layers(im):
    return np.stack([im.layer(i).pixels() for i in range(im.layers)]) if im.layers else np.zeros((0, im.height, im.scanlineInBytes), np.uint8)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_image_load(L, device):
    from gamut_amd import image as gi
    for name, f in (("fixture", FIXTURE), ("three_frames", gif_cases.three_frames())):
        ref, info, (aspect, fps) = gif_ref_c.load(f)
        im = gi.Image(device=device)
        assert im.loadFromMemory(f), (name, im.errorMessage)
        assert (im.layers, im.width, im.height, im.type) == (info["layers"], info["width"], info["height"], 12), name
        assert np.float32(im.pixelAspectRatio) == aspect and im.dotsPerInchY == -1.0
        assert np.array_equal(_image_layers(im), ref.reshape(info["layers"], info["height"], -1)), name
        for flags in (gi.LOAD_RGB | gi.LOAD_NO_ALPHA, gi.LOAD_16BIT, gi.LOAD_GREYSCALE | gi.LOAD_ALPHA | gi.LOAD_FP32,
                      gi.LAYOUT_VERT_FLIPPED | gi.LAYOUT_ALIGNED[64] | gi.LAYOUT_TRAILING[3], gi.LOAD_RGB | gi.LOAD_NO_ALPHA | gi.LAYOUT_BORDER[2] | gi.LAYOUT_MULTIPLICITY[4]):
            src = ref.copy()
            view = gi.Image()
            assert view.createLayeredView(src, info["width"], info["height"], info["layers"], 12, info["width"] * 4, info["width"] * info["height"] * 4)
            want = view.clone()                                             # convertTo applied to the reference's rgba8 layers
            target = gi.lib().gamut_apply_load_flags(12, flags)
            assert want.convertTo(target, flags & 0xFFFF)
            got = gi.Image(device=device)
            assert got.loadFromMemory(f, flags), (name, hex(flags), got.errorMessage)
            assert got.type == target and got.layers == info["layers"], (name, hex(flags))
            assert (got.width, got.height, got.scanlineInBytes) == (want.width, want.height, want.scanlineInBytes)
            assert np.array_equal(_image_layers(got), _image_layers(want)), (name, hex(flags))
            assert got.isStoredUpsideDown == bool(flags & gi.LAYOUT_VERT_FLIPPED)
            assert np.float32(got.pixelAspectRatio) == aspect


def test_image_load_zero_frames(L):
    from gamut_amd import image as gi
    by_name = {n: f for n, f, _ in gif_cases.cases()}
    im = gi.Image()
    assert im.loadFromMemory(by_name["zero_frames"]) and (im.layers, im.width, im.height, im.type) == (0, 40, 30, 12)
    bad = gi.Image(device=True)
    assert not bad.loadFromMemory(by_name["deferred_clear_crossing_8192"]) and bad.errorMessage == "Image decoding failed"


def test_large_file(L):
    """640 x 480, 8 frames: both kernels span many workgroups, an index buffer of 307200 bytes"""
    f = gif_cases.large()
    refs = check_batch(L, [f], ["large"])
    assert refs[0][0].shape == (8, 480, 640, 4)
