"""The TGA encoder on the GPU against the serial C restatement of the reference (tests/c/tga_write_ref.c), byte for byte: one batched
call over every source type, width and content, the geometry extremes, padded / negative pitches and misaligned sources, raw and
mixed batches, refused images among good neighbours, the round trip through the GPU decoder, the Image layer.  Output allocations
are filled with 0xA5, carry 4 KiB guards and are compared whole; output offsets are odd."""
import ctypes as C

import numpy as np
import pytest
import torch

import tga_encode_cases as cases
import tga_encode_ref
import tga_gen
import tga_write_ref_c
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def arr(t, vals):
    return (t * len(vals))(*vals)


def encode_batch(L, imgs, rle=None, pitch_kind="tight", shift=0, override=None):
    """One gamut_hip_tga_encode_batch_device call.  imgs: (h, w, comp) arrays; rle: None (NULL) or a list of 0 / 1; pitch_kind: tight,
    padded or negative; shift: the sources' base modulo 16; override: {index: (width, height, comp, null_source)} turns image `index`
    into a refused one.  -> (rc, statuses, lengths, the whole output allocation, offsets, the expected allocation)"""
    n = len(imgs)
    override = override or {}
    blob, places, pos = [], [], 0
    for k, im in enumerate(imgs):
        h, w, comp = im.shape
        row = w * comp
        pitch = row if pitch_kind == "tight" else row + 5 + k % 3
        pos = (pos + 15) // 16 * 16 + shift
        mem = np.full(pitch * h, 0x3C, np.uint8)
        for y in range(h):
            at = (h - 1 - y) * pitch if pitch_kind == "negative" else y * pitch
            mem[at:at + row] = im[y].reshape(-1)
        places.append((pos + ((h - 1) * pitch if pitch_kind == "negative" else 0), -pitch if pitch_kind == "negative" else pitch))
        blob.append((pos, mem))
        pos += mem.size
    host = np.full(pos + 16, 0x3C, np.uint8)
    for at, mem in blob:
        host[at:at + mem.size] = mem
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    W = [im.shape[1] for im in imgs]; H = [im.shape[0] for im in imgs]; Cc = [im.shape[2] for im in imgs]
    ptrs = [src.data_ptr() + p for p, _ in places]
    for k, (w, h, c, null) in override.items():
        W[k], H[k], Cc[k] = w, h, c
        if null:
            ptrs[k] = None
    refs = [None if k in override else tga_write_ref_c.encode(im, True if rle is None else bool(rle[k])) for k, im in enumerate(imgs)]
    offs, opos = [], GUARD
    for k, im in enumerate(imgs):
        opos += 1 + 2 * (k % 8)                                             # odd byte positions, every odd residue mod 16 among them
        offs.append(opos)
        opos += tga_encode_ref.bound(im.shape[1], im.shape[0], im.shape[2]) + GUARD
        opos += opos & 1
    expect = np.full(opos, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((opos,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = arr(C.c_int64, [-7] * n)
    st = arr(C.c_int, [77] * n)
    rc = L.gamut_hip_tga_encode_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int64, [p for _, p in places]), arr(C.c_int32, W), arr(C.c_int32, H),
                                             arr(C.c_int32, Cc), None if rle is None else arr(C.c_int32, list(rle)), n, arr(C.c_int64, offs),
                                             out.data_ptr(), olen, st, None)
    torch.cuda.synchronize()
    return rc, list(st), list(olen), out.cpu().numpy(), offs, expect, refs


def check_batch(L, imgs, names=None, **kw):
    rc, st, olen, got, offs, expect, refs = encode_batch(L, imgs, **kw)
    bad = [k for k, r in enumerate(refs) if r is None]
    assert rc == (_capi.ERR_INVALID_ARG if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for k, r in enumerate(refs):
        name = names[k] if names else k
        assert st[k] == (0 if r is not None else _capi.ERR_INVALID_ARG), (name, st[k])
        assert olen[k] == (len(r) if r is not None else 0), (name, olen[k], r and len(r))
        if r is not None and not np.array_equal(got[offs[k]:offs[k] + len(r)], expect[offs[k]:offs[k] + len(r)]):
            d = int(np.flatnonzero(got[offs[k]:offs[k] + len(r)] != expect[offs[k]:offs[k] + len(r)])[0])
            assert False, f"{name}: first difference at file byte {d} of {len(r)}"
    assert np.array_equal(got, expect), "a byte outside every file was written"      # the WHOLE allocation, guards included
    return [None if r is None else got[o:o + len(r)].tobytes() for r, o in zip(refs, offs)]


def test_one_batched_call_over_types_widths_and_contents(L):
    win = L.gamut_hip_tga_encode_window()
    assert win > 0 and win % 64 == 0
    items = cases.matrix_images((63, 64, 65, win - 1, win, win + 1, 2 * win + 1))
    assert len(items) > 300
    check_batch(L, [im for _, im in items], [n for n, _ in items])


def test_known_rows(L):
    """the rows whose packets the issue lists, as l8 images of one row: the files carry exactly those packets"""
    imgs = [np.asarray(row, np.uint8).reshape(1, -1, 1) for _, row, _ in cases.KNOWN_ROWS]
    files = check_batch(L, imgs, [n for n, _, _ in cases.KNOWN_ROWS])
    for f, (name, row, packets) in zip(files, cases.KNOWN_ROWS):
        got, p = [], 18
        while p < len(f):
            op = f[p]
            got.append(("R" if op & 0x80 else "raw") + str((op & 127) + 1))
            p += 1 + 3 * (1 if op & 0x80 else (op & 127) + 1)
        assert got == packets, name


def test_geometry_extremes(L):
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 3, (1, 65535, 4)).astype(np.uint8)
    wide[0, 20000:20300] = 9                                                # a long run inside the random stretch
    wide[0, 40000:] = np.repeat(wide[0, 40000::3], 3, axis=0)[:25535]       # runs of three
    tall = rng.integers(0, 256, (65535, 1, 3)).astype(np.uint8)
    imgs = [wide, tall] + [cases.content("alphabet", 300, 200, comp, 40 + comp) for comp in (1, 2, 3, 4)]
    files = check_batch(L, imgs)
    assert len(files[1]) == tga_encode_ref.bound(1, 65535, 3) == L.gamut_hip_tga_encode_bound(1, 65535, 3)     # the bound is reached at width 1


@pytest.mark.parametrize("pitch_kind", ["padded", "negative"])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_layouts(L, pitch_kind, shift):
    items = [(n, im) for n, im in cases.matrix_images((513,)) if im.shape[1] in (3, 129, 258, 513)]
    check_batch(L, [im for _, im in items], [n for n, _ in items], pitch_kind=pitch_kind, shift=shift)


def test_source_base_off_alignment_with_tight_rows(L):
    items = cases.random_images(24, 7, 300)
    for shift in (1, 3):
        check_batch(L, [im for _, im in items], [n for n, _ in items], shift=shift)


def test_raw_files_and_a_batch_that_mixes_both_modes(L):
    items = cases.random_images(20, 11, 600) + [(n, im) for n, im in cases.matrix_images() if im.shape[1] in (1, 130, 257)][:40]
    imgs = [im for _, im in items]
    check_batch(L, imgs, rle=[0] * len(imgs))
    files = check_batch(L, imgs, rle=[k % 2 for k in range(len(imgs))])
    assert files[0][2] == 2 and files[1][2] == 10
    assert len(files[0]) == 18 + imgs[0].shape[0] * imgs[0].shape[1] * tga_encode_ref.file_channels(imgs[0].shape[2])


def test_refused_images_do_not_disturb_their_neighbours(L):
    items = cases.random_images(12, 13, 500)                                # more than eight images of different geometry
    imgs = [im for _, im in items]
    check_batch(L, imgs, override={2: (65536, 3, 3, False), 5: (7, 3, 5, False), 9: (7, 3, 4, True)})
    check_batch(L, imgs, override={0: (0, 3, 3, False), 11: (3, 0, 3, False)})
    n = len(imgs)
    one = arr(C.c_int64, [0] * n)
    assert L.gamut_hip_tga_encode_batch_device(None, one, None, None, None, None, n, one, None, one, None, None) == _capi.ERR_INVALID_ARG


def test_round_trip_through_the_gpu_decoder(L):
    items = cases.random_images(16, 17, 700) + [("wide", cases.content("stretch127", 1500, 3, 4, 3))]
    imgs = [im for _, im in items]
    for rle in (None, [0] * len(imgs)):
        files = check_batch(L, imgs, rle=rle)
        n = len(files)
        bufs = [np.frombuffer(f, np.uint8).copy() for f in files]
        want = [tga_encode_ref.converted_source(im) for im in imgs]
        offs, pos = [], 0
        for wnt in want:
            offs.append(pos)
            pos += (wnt.size + 15) // 16 * 16
        out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        info = (_capi.TgaInfo * n)()
        st = arr(C.c_int, [77] * n)
        rc = L.gamut_hip_tga_decode_batch_device(arr(C.c_void_p, [b.ctypes.data for b in bufs]), arr(C.c_size_t, [b.size for b in bufs]), n, 0,
                                                 arr(C.c_int64, offs), out.data_ptr(), info, st, None)
        torch.cuda.synchronize()
        assert rc == 0 and list(st) == [0] * n, L.gamut_hip_last_error()
        got = out.cpu().numpy()
        for k, wnt in enumerate(want):
            assert info[k].rle == (0 if rle else 1) and info[k].bottom_up == 1 and info[k].channels_in_file == wnt.shape[2]
            assert np.array_equal(got[offs[k]:offs[k] + wnt.size].reshape(wnt.shape), wnt), items[k][0]


def test_host_drop_in(L):
    for name, im in cases.random_images(6, 19, 400):
        h, w, comp = im.shape
        for rle in (1, 0):
            n = C.c_int(0)
            p = L.gamut_hip_tga_write_to_mem(im.ctypes.data, w * comp, w, h, comp, rle, C.byref(n))
            assert p, L.gamut_hip_last_error()
            assert C.string_at(p, n.value) == tga_write_ref_c.encode(im, bool(rle)), name
            C.CDLL(None).free(C.c_void_p(p))
        flipped = np.ascontiguousarray(im[::-1])                            # a negative pitch: row 0 is the last one in memory
        n = C.c_int(0)
        p = L.gamut_hip_tga_write_to_mem(flipped.ctypes.data + (h - 1) * w * comp, -w * comp, w, h, comp, 1, C.byref(n))
        assert p and C.string_at(p, n.value) == tga_write_ref_c.encode(im, True), name
        C.CDLL(None).free(C.c_void_p(p))


@pytest.mark.parametrize("device", [False, True])
def test_image_save(L, device, tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    names = {1: "l8", 2: "la8", 3: "rgb8", 4: "rgba8"}
    for comp in (1, 2, 3, 4):
        im = gi.Image(device=device)
        if comp <= 2:                                                       # (l8 / la8 images encode to 24 / 32-bit files: load grey files instead)
            assert im.loadFromMemory(tga_gen.make(141, 6, 11, 8 * comp, policy="mixed", seed=50 + comp))
            px = np.asarray(im.pixels()).reshape(6, 141, comp).copy()
        else:
            px = cases.content("alphabet", 141, 6, comp, 50 + comp)
            assert im.loadFromMemory(tga_write_ref_c.encode(px, False))
            assert np.array_equal(np.asarray(im.pixels()).reshape(px.shape), px)
        assert im.type == O.PT[names[comp]] and im.isDevice == device
        want = tga_write_ref_c.encode(px, True)
        enc = im.save_tga_to_memory()
        assert enc == want, comp
        assert im.saveTGAToMemory(12345) == want                            # flags are ignored
        path = tmp_path / f"x{comp}.tga"
        assert im.saveTGAToFile(path) and path.read_bytes() == want
        assert im.save_to_memory(gi.FORMAT_TGA) is None                     # the generic entry does not dispatch TGA
        assert im.isValid and im.errorMessage is None
        again = gi.Image(device=device)
        assert again.loadFromMemory(enc) and np.array_equal(np.asarray(again.pixels()), tga_encode_ref.converted_source(px).reshape(6, -1))


def test_image_save_of_views(L):
    import oracle_lib as O
    from gamut_amd import image as gi
    px = cases.content("stretch126", 300, 5, 4, 61)
    up = gi.Image()                                                         # bottom-up view: a negative pitch
    mem = np.ascontiguousarray(px[::-1])
    assert up.createView(mem, 300, 5, O.PT["rgba8"], -1200) and up.isStoredUpsideDown
    assert up.save_tga_to_memory() == tga_write_ref_c.encode(px, True)
    layers = np.stack([cases.content("alphabet", 70, 4, 3, 70 + k) for k in range(3)])
    lay = gi.Image()
    assert lay.createLayeredView(layers, 70, 4, 3, O.PT["rgb8"], 210, 840) and lay.layers == 3
    assert lay.save_tga_to_memory() == tga_write_ref_c.encode(layers[0], True)         # layer 0
    assert lay.layer(2).save_tga_to_memory() == tga_write_ref_c.encode(layers[2], True)
