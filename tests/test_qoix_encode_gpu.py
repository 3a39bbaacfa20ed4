"""The QOIX encoder on the GPU against the serial C restatement of the reference (tests/c/qoix_write_ref.c), byte for byte: one batched
call per test over widths and contents, runs, alpha steps, LUMA bounds, the index, crafted LZ4 strings, the container choice at its
boundary, padded / negative pitches and misaligned sources, refused images among good neighbours, the round trip through the GPU
decoder, the host drop-in and the Image layer.  Output allocations are filled with 0xA5, carry 4 KiB guards and are compared whole;
output offsets are odd."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import qoix_encode_cases as cases
import qoix_gen
import qoix_write_ref_c as ref
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


def layout_outputs(bounds):
    """odd byte positions, every odd residue mod 16 among them, 4 KiB guards -> (offsets, allocation size)"""
    offs, opos = [], GUARD
    for k, b in enumerate(bounds):
        opos += 1 + 2 * (k % 8)
        offs.append(opos)
        opos += b + GUARD
        opos += opos & 1
    return offs, opos


def encode_batch(L, imgs, modes=None, pitch_kind="tight", shift=0, override=None, bad_offset=(), par=1.0, dpi=96.0):
    """One gamut_hip_qoix_encode_batch_device call.  imgs: (h, w, 3 | 4) arrays; modes: 0 / 1 per image (default 0); pitch_kind: tight,
    padded or negative; shift: the sources' base modulo 16; override: {index: (width, height, channels, colorspace, null_source)} turns
    image `index` into a refused one, as does an index in bad_offset (a negative out_offset)."""
    n = len(imgs)
    override = override or {}
    modes = modes or [0] * n
    blob, places, pos = [], [], 0
    for k, im in enumerate(imgs):
        h, w, ch = im.shape
        row = w * ch
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
    descs = (_capi.QoixDesc * n)()
    for k, im in enumerate(imgs):
        descs[k] = _capi.QoixDesc(im.shape[1], im.shape[0], im.shape[2], k % 3 if im.shape[2] == 4 else 0, modes[k], par, dpi)
    ptrs = [src.data_ptr() + p for p, _ in places]
    for k, (w, h, c, cs, null) in override.items():
        descs[k].width, descs[k].height, descs[k].channels, descs[k].colorspace = w, h, c, cs
        if null:
            ptrs[k] = None
    refused = set(override) | set(bad_offset)
    refs = [None if k in refused else ref.encode(im, modes[k], colorspace=descs[k].colorspace, par=par, dpi=dpi) for k, im in enumerate(imgs)]
    offs, size = layout_outputs([ref.bound(im.shape[1], im.shape[0], im.shape[2]) for im in imgs])
    expect = np.full(size, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = arr(C.c_int64, [-7] * n)
    st = arr(C.c_int, [77] * n)
    given = [-5 if k in bad_offset else o for k, o in enumerate(offs)]
    rc = L.gamut_hip_qoix_encode_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int64, [p for _, p in places]), descs, n, arr(C.c_int64, given),
                                              out.data_ptr(), olen, st, None)
    torch.cuda.synchronize()
    return rc, list(st), list(olen), out.cpu().numpy(), offs, expect, refs


def compare(L, rc, st, olen, got, offs, expect, refs, names, what):
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
            assert False, f"{name}: first difference at {what} byte {d} of {len(r)}"
    assert np.array_equal(got, expect), "a byte outside every output was written"     # the WHOLE allocation, guards included
    return [None if r is None else got[o:o + len(r)].tobytes() for r, o in zip(refs, offs)]


def check_batch(L, imgs, names=None, **kw):
    rc, st, olen, got, offs, expect, refs = encode_batch(L, imgs, **kw)
    return compare(L, rc, st, olen, got, offs, expect, refs, names, "file")


def both_modes(L, items, **kw):
    imgs, names = [im for _, im in items], [n for n, _ in items]
    check_batch(L, imgs, names, modes=[1] * len(imgs), **kw)
    return check_batch(L, imgs, names, modes=[0] * len(imgs), **kw)


def test_widths_and_contents(L):
    win = L.gamut_hip_qoix_encode_window()
    assert win > 0
    items = cases.matrix_images(sorted({1, 2, 3, 63, 64, 65, win - 1, win + 1, 2 * win + 1, 700}))      # 700: a row's bytes cross a flush of the staging
    assert len(items) >= 250
    both_modes(L, items)


def test_known_streams(L):
    files = check_batch(L, [im for _, im, _ in cases.KNOWN_STREAMS], [n for n, _, _ in cases.KNOWN_STREAMS])
    for f, (name, im, stream) in zip(files, cases.KNOWN_STREAMS):
        assert f[16] == 0 and f[25:].hex() == stream, name


def test_runs(L):
    both_modes(L, cases.run_images())


def test_alpha_luma_and_the_index(L):
    both_modes(L, cases.op_images())


def lz4_batch(L, strings, null=()):
    n = len(strings)
    blob, at = bytearray(), []
    for k, s in enumerate(strings):
        blob += bytes((-len(blob)) % 16 + (1, 3, 0)[k % 3])                # string bases at 1, 3 and 0 modulo 16
        at.append(len(blob))
        blob += s
    src = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), np.uint8).copy()).cuda()
    refs = [None if k in null else ref.lz4_compress(s) for k, s in enumerate(strings)]
    for s in strings:
        assert L.gamut_hip_lz4_compress_bound(len(s)) == ref.lz4_bound(len(s)) == len(s) + len(s) // 255 + 16
    offs, size = layout_outputs([ref.lz4_bound(len(s)) for s in strings])
    expect = np.full(size, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    olen, st = arr(C.c_int64, [-7] * n), arr(C.c_int, [77] * n)
    ptrs = [None if k in null else src.data_ptr() + a for k, a in enumerate(at)]
    rc = L.gamut_hip_lz4_compress_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int32, [len(s) for s in strings]), n, arr(C.c_int64, offs),
                                               out.data_ptr(), olen, st, None)
    torch.cuda.synchronize()
    return rc, list(st), list(olen), out.cpu().numpy(), offs, expect, refs


def test_lz4_crafted_strings(L):
    items = cases.lz4_strings()
    assert ref.lz4_compress(b"") == b"\x00"                                 # the reference accepts length 0: one token
    compare(L, *lz4_batch(L, [s for _, s in items]), [n for n, _ in items], "block")


def test_lz4_batch_of_100_and_a_null_source(L):
    strings = cases.lz4_mixed(100)
    compare(L, *lz4_batch(L, strings), None, "block")
    compare(L, *lz4_batch(L, strings, null=(41, 77)), None, "block")


def test_container_choice_at_the_boundary(L):
    items = cases.boundary_images()
    big = cases.content("noise", 160, 140, 3, 5)                            # an op stream of >= 65547 bytes: LZ4's byU32 path
    assert len(ref.encode(big, 1)) - 25 >= 65547
    more = [("noise 160x140", big), ("photo 200x100x4", qoix_gen.photo_like(200, 100, 4, 3)), ("flat 160x140", qoix_gen.flat_image(160, 140, 3, 4))]
    imgs = [im for _, im, _ in items] + [im for _, im in more]
    files = check_batch(L, imgs, [n for n, _, _ in items] + [n for n, _ in more])
    packed = [f[16] for f in files]
    assert packed.count(1) >= 5 and packed.count(0) >= 5
    for f, (name, _, diff) in zip(files, items):
        assert f[16] == (1 if diff < 0 else 0), name


@pytest.mark.parametrize("pitch_kind", ["padded", "negative"])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_layouts(L, pitch_kind, shift):
    items = [(n, im) for n, im in cases.matrix_images((3, 65, 129)) if im.shape[0] > 1]
    imgs, names = [im for _, im in items], [n for n, _ in items]
    check_batch(L, imgs, names, modes=[k % 2 for k in range(len(imgs))], pitch_kind=pitch_kind, shift=shift)


def test_source_base_off_alignment_with_tight_rows(L):
    items = cases.matrix_images((64, 130))
    for shift in (1, 3):
        check_batch(L, [im for _, im in items], [n for n, _ in items], shift=shift)


def test_refused_images_do_not_disturb_their_neighbours(L):
    items = [(n, im) for n, im in cases.matrix_images((2, 65, 131)) if im.shape[0] == 5][:14]     # more than eight images of different geometry
    imgs = [im for _, im in items]
    assert len(imgs) == 14
    check_batch(L, imgs, override={0: (0, 5, 3, 0, False), 3: (7, 0, 3, 0, False), 5: (7, 3, 2, 0, False), 6: (7, 3, 5, 0, False),
                                   8: (7, 3, 4, 3, False), 10: (20000, 20000, 3, 0, False), 12: (7, 3, 4, 0, True)}, bad_offset=(13,))
    check_batch(L, imgs, override={13: (2, 200000000, 3, 0, False)})
    n = len(imgs)
    one = arr(C.c_int64, [0] * n)
    assert L.gamut_hip_qoix_encode_batch_device(None, one, None, n, one, None, one, None, None) == _capi.ERR_INVALID_ARG


def test_round_trip_through_the_gpu_decoder(L):
    items = [(n, im) for n, im in cases.matrix_images((65, 200)) if im.shape[0] == 5] + cases.boundary_images()[:8]
    imgs = [it[1] for it in items]
    files = check_batch(L, imgs)
    assert {f[16] for f in files} == {0, 1}                                 # stored and LZ4 files both
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8).copy() for f in files]
    offs, pos = [], 0
    for im in imgs:
        offs.append(pos)
        pos += (im.size + 15) // 16 * 16
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.QoixInfo * n)()
    st = arr(C.c_int, [77] * n)
    rc = L.gamut_hip_qoix_decode_batch_device(arr(C.c_void_p, [b.ctypes.data for b in bufs]), arr(C.c_size_t, [b.size for b in bufs]), n, 0,
                                              arr(C.c_int64, offs), out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    assert rc == 0 and list(st) == [0] * n, L.gamut_hip_last_error()
    got = out.cpu().numpy()
    for k, im in enumerate(imgs):
        assert info[k].channels == im.shape[2] and info[k].compression == files[k][16]
        assert np.array_equal(got[offs[k]:offs[k] + im.size].reshape(im.shape), im), items[k][0]


def test_host_drop_in(L):
    free = C.CDLL(None).free
    for k, (name, im) in enumerate(cases.matrix_images((37,))[-6:] + [("big", cases.content("photo", 120, 90, 4, 9))]):
        h, w, ch = im.shape
        for mode in (0, 1):
            d = _capi.QoixDesc(w, h, ch, 0, mode, 2.0, 72.0)
            n = C.c_int(0)
            p = L.gamut_hip_qoix_write_to_mem(im.ctypes.data, w * ch, C.byref(d), C.byref(n))
            assert p, L.gamut_hip_last_error()
            assert C.string_at(p, n.value) == ref.encode(im, mode, par=2.0, dpi=72.0), name
            free(C.c_void_p(p))
        flipped = np.ascontiguousarray(im[::-1])                            # a negative pitch: row 0 is the last one in memory
        d = _capi.QoixDesc(w, h, ch, 0, 0, 1.0, 96.0)
        n = C.c_int(0)
        p = L.gamut_hip_qoix_write_to_mem(flipped.ctypes.data + (h - 1) * w * ch, -w * ch, C.byref(d), C.byref(n))
        assert p and C.string_at(p, n.value) == ref.encode(im), name
        free(C.c_void_p(p))
    bad = _capi.QoixDesc(4, 4, 2, 0, 0, 1.0, 96.0)
    assert not L.gamut_hip_qoix_write_to_mem(np.zeros(64, np.uint8).ctypes.data, 8, C.byref(bad), C.byref(C.c_int(0)))


@pytest.mark.parametrize("device", [False, True])
def test_image_save(L, device, tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    for tname, ch, cs in (("rgb8", 3, 0), ("rgba8", 4, 0), ("rgbap8", 4, 2)):
        px = cases.content("photo" if ch == 3 else "alphabet", 141, 6, ch, 50 + ch + cs)
        im = gi.Image(device=device)
        assert im.loadFromMemory(qoix_gen.encode(px, colorspace=cs, par=1.5, dpi=300.0))       # a file that carries par and dpi
        assert im.type == O.PT[tname] and im.isDevice == device
        assert np.array_equal(np.asarray(im.pixels()).reshape(px.shape), px)
        want = ref.encode(px, 0, colorspace=cs, par=im.pixelAspectRatio, dpi=im.dotsPerInchY)
        assert want[17:25] == struct.pack(">ff", 1.5, 300.0)
        enc = im.save_qoix_to_memory()
        assert enc == want, tname
        assert im.saveQOIXToMemory(12345) == want                           # flags are ignored
        path = tmp_path / f"x{ch}{cs}.qoix"
        assert im.saveQOIXToFile(path) and path.read_bytes() == want
        assert im.save_to_memory(gi.FORMAT_QOIX) is None                    # the generic entry does not dispatch QOIX
        assert im.isValid and im.errorMessage is None
        again = gi.Image(device=device)
        assert again.loadFromMemory(enc) and again.type == im.type and np.array_equal(np.asarray(again.pixels()), np.asarray(im.pixels()))


def test_image_save_of_views(L):
    import oracle_lib as O
    from gamut_amd import image as gi
    px = cases.content("flat", 300, 5, 4, 61)
    up = gi.Image()                                                         # bottom-up view: a negative pitch
    mem = np.ascontiguousarray(px[::-1])
    assert up.createView(mem, 300, 5, O.PT["rgba8"], -1200) and up.isStoredUpsideDown
    assert up.save_qoix_to_memory() == ref.encode(px, 0, par=up.pixelAspectRatio, dpi=up.dotsPerInchY)
    layers = np.stack([cases.content("alphabet", 70, 4, 3, 70 + k) for k in range(3)])
    lay = gi.Image()
    assert lay.createLayeredView(layers, 70, 4, 3, O.PT["rgb8"], 210, 840) and lay.layers == 3
    kw = dict(par=lay.pixelAspectRatio, dpi=lay.dotsPerInchY)
    assert lay.save_qoix_to_memory() == ref.encode(layers[0], 0, **kw)      # layer 0
    assert lay.layer(2).save_qoix_to_memory() == ref.encode(layers[2], 0, **kw)
