"""TGA on the GPU against the serial C restatement of the reference (tests/c/tga_ref.c), byte for byte: the batched decode over every
variant and geometry in one call, the run-length edge cases (packets across rows and across the kernel's windows, overrun, bad
indices), truncated files among good neighbours, the Image layer, TGA files in the mixed-format call.  Output allocations are filled
with 0xA5, carry guards and are compared whole; output offsets are odd."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import tga_cases
import tga_gen
import tga_ref_c
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


@pytest.fixture(scope="module")
def WIN(L):
    return L.gamut_hip_tga_rle_window()


def decode_batch(L, files, req):
    """one gamut_hip_tga_decode_batch_device call -> (rc, statuses, infos, whole output allocation, offsets, expected allocation, refs, mask)
    mask: False over the own bytes of a run-length file that is refused (the device may leave anything there)"""
    n = len(files)
    refs = [tga_ref_c.load(f, req) for f in files]
    heads = [tga_ref_c.header(f) for f in files]
    sizes = []
    for r, (det, ok, hd) in zip(refs, heads):
        sizes.append(r[0].size if r is not None else hd["width"] * hd["height"] * (req or hd["channels_in_file"]) if ok and hd["width"] * hd["height"] < 1 << 24 else 64)
    offs, pos = [], GUARD
    for k, s in enumerate(sizes):
        pos += 1 + 2 * (k % 8)                                              # odd byte positions, every residue mod 16 among them
        offs.append(pos)
        pos += s + GUARD
        pos += pos & 1
    expect = np.full(pos, 0xA5, np.uint8)
    mask = np.ones(pos, bool)
    for r, o, s, (det, ok, hd) in zip(refs, offs, sizes, heads):
        if r is not None:
            expect[o:o + r[0].size] = r[0].reshape(-1)
        elif ok and hd["rle"]:
            mask[o:o + s] = False
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs])
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    offa = (C.c_int64 * n)(*offs)
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.TgaInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_tga_decode_batch_device(ptrs, lens, n, req, offa, out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    return rc, list(st), info, out.cpu().numpy(), offs, expect, refs, mask


def check_batch(L, files, req, names=None):
    rc, st, info, got, offs, expect, refs, mask = decode_batch(L, files, req)
    bad = [i for i, r in enumerate(refs) if r is None]
    assert rc == (_capi.ERR_DECODE if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for i, r in enumerate(refs):
        assert st[i] == (0 if r is not None else _capi.ERR_DECODE), (i, names[i] if names else None, st[i])
        if r is not None:
            assert {k: int(getattr(info[i], k)) for k in tga_ref_c.INFO_FIELDS} == r[1], (i, names[i] if names else None)
    same = (got == expect) | ~mask
    if not same.all():                                                      # the WHOLE allocation, guards included
        first = int(np.flatnonzero(~same)[0])
        k = max([i for i in range(len(offs)) if offs[i] - GUARD <= first], default=0)
        assert False, ("req", req, "image", k, names[k] if names else None, "first difference at", first - offs[k], "of", refs[k][0].size if refs[k] else None,
                       "got", got[first:first + 8].tolist(), "want", expect[first:first + 8].tolist())
    return refs


VARIANTS = tga_cases.variant_files()


def test_unpacked_runs_at_every_output_alignment(L):
    """a row of 1 pixel (3 bytes: shorter than the 16-byte head of its store), of 5 (head and tail, no 16-byte body) and of 1025 (one
    pixel into a second 1024-pixel unit) in one batch of three 2-row true-colour files at req_comp 3, with EVERY out_offset at
    residue r modulo 16, r = 0..15 in turn; the whole allocation, canaries included, against the Python reading of the reference"""
    import tga_ref
    files = [tga_gen.make(w, 2, 2, 24, top_down=w == 5, seed=w) for w in (1, 5, 1025)]
    refs = [tga_ref.decode(f, 3)[0] for f in files]
    assert [r.shape for r in refs] == [(2, 1, 3), (2, 5, 3), (2, 1025, 3)]
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * 3)(*[b.size for b in bufs])
    for r in range(16):
        offs, pos = [], 0
        for ref in refs:
            pos = (pos + 64 + 15) // 16 * 16 + r                            # at least 64 canary bytes in front of every image
            offs.append(pos); pos += ref.size
        pos += 64
        expect = np.full(pos, 0xA5, np.uint8)
        for ref, o in zip(refs, offs):
            expect[o:o + ref.size] = ref.reshape(-1)
        out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0 and all(o % 16 == r for o in offs)
        info = (_capi.TgaInfo * 3)(); st = (C.c_int * 3)(77, 77, 77)
        rc = L.gamut_hip_tga_decode_batch_device(ptrs, lens, 3, 3, (C.c_int64 * 3)(*offs), out.data_ptr(), info, st, None)
        assert rc == 0 and list(st) == [0, 0, 0], (r, L.gamut_hip_last_error())
        bad = np.flatnonzero(out.cpu().numpy() != expect)
        assert bad.size == 0, ("residue", r, "first difference at", int(bad[0]), "offsets", offs)


@pytest.mark.parametrize("req", [0, 3, 4])
def test_every_variant_and_geometry_in_one_call(L, req):
    """types 1 / 2 / 3 / 9 / 10 / 11 x every depth and colour-map entry size x 8- and 16-bit indices at 1x1, 3x2, 5x3, 33x5, 257x7 and
    1100x2, both row orders, ID fields, colour-map starts, descriptor junk and footers mixed in"""
    refs = check_batch(L, [f for _, f in VARIANTS], req, [n for n, _ in VARIANTS])
    assert len(refs) == 38 * 6 and all(r is not None for r in refs)
    assert {r[1]["channels_in_file"] for r in refs} == {1, 2, 3, 4}


@pytest.mark.parametrize("count", [1, 17])
def test_batches_of_1_and_17_files(L, count):
    for start, step in ((0, 13), (5, 13), (100, 7), (114, 6), (139, 5)):    # unpacked only, both kinds, run-length only
        pick = VARIANTS[start::step][:count]
        assert len(pick) == count
        for req in (0, 3, 4):
            check_batch(L, [f for _, f in pick], req, [n for n, _ in pick])


def test_rle_edge_cases(L, WIN):
    cases = tga_cases.rle_edge_cases(WIN)
    assert sum(n.startswith("three_windows") for n, _ in cases) >= 3
    for req in (0, 3, 4):
        refs = check_batch(L, [f for _, f in cases], req, [n for n, _ in cases])
        assert all(r is not None for r in refs)


def test_a_stream_over_many_windows(L, WIN):
    """1100 x 40 pixels of one-pixel packets and of mixed packets: 40+ windows each, top-down and bottom-up, in one batch with a tiny file"""
    files = [tga_gen.make(1100, 40, 10, 32, policy="one", seed=1), tga_gen.make(1100, 40, 10, 24, policy="mixed", top_down=True, seed=2),
             tga_gen.make(1, 1, 10, 32, seed=3), tga_gen.make(1100, 40, 9, 16, 32, policy="raw", seed=4)]
    assert len(files[0]) > 40 * WIN
    for req in (0, 4):
        check_batch(L, files, req)


def test_truncated_files_are_refused_alone(L, WIN):
    cuts = tga_cases.truncations(WIN)
    good = VARIANTS[3::17]
    files, names = [], []
    for k, (n, f) in enumerate(cuts):
        files += [good[k % len(good)][1], f]; names += [good[k % len(good)][0], n]
    files.append(good[0][1]); names.append(good[0][0])
    for req in (0, 4):
        refs = check_batch(L, files, req, names)
        assert [r is None for r in refs] == [bool(k & 1) for k in range(len(files))]
    refs = check_batch(L, [f for _, f in cuts], 0, [n for n, _ in cuts])    # nothing but refused files: no launch for the unpacked ones
    assert all(r is None for r in refs)


def test_header_refusals_and_bad_arguments_in_a_batch(L):
    files = [VARIANTS[0][1]] + [f for _, f, _ in tga_cases.header_refusals() if len(f) < 1000] + [VARIANTS[150][1]]
    refs = check_batch(L, files, 0)
    assert refs[0] is not None and refs[-1] is not None and all(r is None for r in refs[1:-1])
    f = np.frombuffer(VARIANTS[0][1], np.uint8)
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    for req in (1, 2, 5):
        assert L.gamut_hip_tga_decode_batch_device((C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), 1, req, (C.c_int64 * 1)(0), out.data_ptr(), None, None, None) == _capi.ERR_INVALID_ARG
    assert (out.cpu().numpy() == 0xA5).all()


@pytest.mark.parametrize("device", [False, True])
def test_image_load(L, device, WIN):
    import oracle_lib as O
    from gamut_amd import image as gi
    names = {1: "l8", 2: "la8", 3: "rgb8", 4: "rgba8"}
    files = [tga_gen.make(37, 5, 2, 24, seed=1), tga_gen.make(33, 4, 10, 32, top_down=True, seed=2), tga_gen.make(16, 3, 3, 8, seed=3),
             tga_gen.make(9, 2, 11, 16, seed=4), tga_gen.make(21, 6, 9, 8, 15, pal_start=4, id_len=5, seed=5), tga_gen.make(5, 3, 2, 16, seed=6),
             tga_cases.window_case(WIN, seed=7)[0]]
    for f in files:
        ref, info = tga_ref_c.load(f, 0)
        comps = ref.shape[2]
        for flags in (0, gi.LOAD_GREYSCALE, gi.LOAD_ALPHA, gi.LOAD_RGB | gi.LOAD_ALPHA, gi.LOAD_16BIT, gi.LOAD_GREYSCALE | gi.LOAD_NO_ALPHA):
            im = gi.Image(device=device)
            assert im.loadFromMemory(f, flags), im.errorMessage
            want_type = L.gamut_apply_load_flags(O.PT[names[comps]], flags)
            assert (im.type, im.width, im.height, im.isDevice) == (want_type, info["width"], info["height"], device)
            exp = O.scanlines_convert(names[comps], ref.reshape(-1), O.PIXEL_TYPES[want_type], info["width"], info["height"]) if want_type != O.PT[names[comps]] else ref
            assert np.array_equal(np.asarray(im.pixels()).reshape(-1).view(np.uint8), np.asarray(exp).reshape(-1).view(np.uint8)), (comps, flags)
            assert im.pixelAspectRatio == np.float32(-1) and im.dotsPerInchY == np.float32(-1)                 # unknown, plugins/tga.d:87-88
        for req, typ in ((3, "rgb8"), (4, "rgba8")):                        # req_comp 3 / 4 of the batch call IS convertTo(rgb8 / rgba8)
            conv = O.scanlines_convert(names[comps], ref.reshape(-1), typ, info["width"], info["height"]) if typ != names[comps] else ref
            assert np.array_equal(np.asarray(conv).reshape(-1).view(np.uint8), tga_ref_c.load(f, req)[0].reshape(-1))
    for name, f in tga_cases.truncations(WIN)[:3]:
        im = gi.Image(device=device)
        assert not im.loadFromMemory(f) and im.errorMessage == "Image decoding failed", name
    im = gi.Image(device=device)
    assert im.loadFromMemory(files[0]) and im.save_to_memory(gi.FORMAT_TGA) is None


@pytest.mark.parametrize("req", [3, 4])
def test_tga_files_in_the_mixed_format_call(L, req):
    import bmp_gen
    import gen
    from PIL import Image
    a = gen.synth_rgb(45, 31, 3)
    bio = io.BytesIO(); Image.fromarray(a).save(bio, "PNG"); png = bio.getvalue()
    bio = io.BytesIO(); Image.fromarray(a).save(bio, "JPEG", quality=90); jpg = bio.getvalue()
    qoi = gen.qoi_encode(a)
    bmp = bmp_gen.make(45, 31, 24, 40, seed=1)
    tgas = [tga_gen.make(45, 31, 2, 24, seed=1), tga_gen.make(17, 3, 9, 8, 32, seed=2), tga_gen.make(40, 30, 11, 16, top_down=True, seed=3),
            tga_gen.make(9, 4, 10, 32, seed=1, pkts=[(False, 10), (True, 10), (False, 16)])[:18 + 41]]

    def run(files):
        n = len(files)
        bufs = [np.frombuffer(f, np.uint8) for f in files]
        offs, pos = [], GUARD
        for f in files:
            offs.append(pos); pos += 45 * 31 * 4 + GUARD
        out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        info = (_capi.ImageInfo * n)(); st = (C.c_int * n)()
        rc = L.gamut_hip_decode_batch_device((C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs]), n, req,
                                             (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None)
        return rc, list(st), info, out.cpu().numpy(), offs
    plain = [jpg, png, qoi, bmp, jpg]
    rc0, st0, info0, out0, offs0 = run(plain)
    assert rc0 == 0 and st0 == [0] * 5 and [i.format for i in info0] == [0, 1, 2, 7, 0]
    mixed = [tgas[0], jpg, png, tgas[1], qoi, tgas[3], bmp, tgas[2], jpg]
    rc, st, info, out, offs = run(mixed)
    assert rc == _capi.ERR_DECODE and st == [0, 0, 0, 0, 0, _capi.ERR_DECODE, 0, 0, 0] and L.gamut_hip_last_error().startswith(b"image 5:")
    assert [i.format for i in info] == [5, 0, 1, 5, 2, 5, 7, 5, 0]
    expect = np.full(out.size, 0xA5, np.uint8)
    npx = 45 * 31 * req
    for k, src in ((1, 0), (2, 1), (4, 2), (6, 3), (8, 4)):                 # the other formats: what the TGA-free batch gave
        expect[offs[k]:offs[k] + npx] = out0[offs0[src]:offs0[src] + npx]
    for k in (0, 3, 7):
        r = tga_ref_c.load(mixed[k], req)
        expect[offs[k]:offs[k] + r[0].size] = r[0].reshape(-1)
        assert (info[k].width, info[k].height, info[k].channels_in_file, info[k].channels) == (r[1]["width"], r[1]["height"], r[1]["channels_in_file"], req)
    out[offs[5]:offs[5] + 9 * 4 * req] = 0xA5                               # (the refused run-length file's own bytes may hold anything)
    assert np.array_equal(out, expect)
    assert np.array_equal(out0[offs0[1]:offs0[1] + npx].reshape(31, 45, req)[..., :3], a)              # (the PNG leg, as a sanity anchor)
