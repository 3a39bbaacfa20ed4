"""The QOI-Plane encoder on the GPU against the serial C restatement of qoiplane_encode (tests/c/qoiplane_write_ref.c; LZ4 and the
container choice from tests/c/qoix_write_ref.c), byte for byte, in modes 0 and 1, with gamut_hip_qoix_set_plane(1): every named case in
one call per channel count and one image per call, shapes around the segment size, runs that are cut at and carried over segment
boundaries, segment boundaries on odd nibbles, the op thresholds, padded / negative pitches, sources at every base and outputs at every
offset modulo 16, batches that mix grey and colour images, refused images among good neighbours, the switch turned off again, the round
trip through the GPU decoder, the host drop-in and the Image layer.  Output allocations are filled with 0xA5, carry 4 KiB guards and are
compared whole.  The switch is process-wide: every test runs inside a fixture that restores the value it found."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import qoiplane_encode_cases as cases
import qoiplane_gen as P
import qoiplane_write_ref_c as ref
import qoix_encode_cases as colour_cases
import qoix_write_ref_c as colour_ref
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


@pytest.fixture(autouse=True)
def plane_on(L):
    prev = L.gamut_hip_qoix_set_plane(1)
    yield
    L.gamut_hip_qoix_set_plane(prev)


@pytest.fixture(scope="module")
def S(L):
    return L.gamut_hip_qoix_plane_encode_segment()


def arr(t, vals):
    return (t * len(vals))(*vals)


def ref_of(im):
    return ref if im.shape[2] < 3 else colour_ref


def layout_outputs(bounds):
    """image k at residue 7 * k + 1 modulo 16 (every residue within 16 images), 4 KiB guards -> (offsets, allocation size)"""
    offs, opos = [], GUARD
    for k, b in enumerate(bounds):
        opos += (7 * k + 1 - opos) % 16
        offs.append(opos)
        opos += b + GUARD
    return offs, opos


def encode_batch(L, imgs, modes=None, pitch_kind="tight", shift=0, override=None, bad_offset=(), colorspace=None, par=1.0, dpi=96.0, per_call=False,
                 expect_refused=False):
    """One gamut_hip_qoix_encode_batch_device call (per_call: one call per image, same buffers).  imgs: (h, w, 1..4) arrays; modes: 0 / 1 per
    image (default 0); pitch_kind: tight, padded or negative; shift: the sources' base modulo 16; override: {index: (width, height,
    channels, colorspace, null_source)} turns image `index` into a refused one, as does an index in bad_offset (a negative out_offset);
    expect_refused: every grey image is expected to be refused (the switch is off)."""
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
        cs = colorspace[k] if colorspace else (k % 3 if im.shape[2] in (2, 4) else k % 2)
        descs[k] = _capi.QoixDesc(im.shape[1], im.shape[0], im.shape[2], cs, modes[k], par, dpi)
    ptrs = [src.data_ptr() + p for p, _ in places]
    for k, (w, h, c, cs, null) in override.items():
        descs[k].width, descs[k].height, descs[k].channels, descs[k].colorspace = w, h, c, cs
        if null:
            ptrs[k] = None
    refused = set(override) | set(bad_offset) | ({k for k, im in enumerate(imgs) if im.shape[2] < 3} if expect_refused else set())
    refs = [None if k in refused else ref_of(im).encode(im, modes[k], colorspace=descs[k].colorspace, par=par, dpi=dpi) for k, im in enumerate(imgs)]
    bounds = [ref_of(im).bound(im.shape[1], im.shape[0], im.shape[2]) for im in imgs]
    if not expect_refused:
        for k, im in enumerate(imgs):
            if k not in override:
                assert L.gamut_hip_qoix_encode_bound(C.byref(descs[k])) == bounds[k]
    offs, size = layout_outputs(bounds)
    expect = np.full(size, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = arr(C.c_int64, [-7] * n)
    st = arr(C.c_int, [77] * n)
    given = [-5 if k in bad_offset else o for k, o in enumerate(offs)]
    pitches = [p for _, p in places]
    if per_call:
        rc = 0
        for k in range(n):
            one_len, one_st = arr(C.c_int64, [-7]), arr(C.c_int, [77])
            r = L.gamut_hip_qoix_encode_batch_device(arr(C.c_void_p, ptrs[k:k + 1]), arr(C.c_int64, pitches[k:k + 1]), C.byref(descs[k]), 1,
                                                     arr(C.c_int64, given[k:k + 1]), out.data_ptr(), one_len, one_st, None)
            rc = rc or r
            olen[k], st[k] = one_len[0], one_st[0]
    else:
        rc = L.gamut_hip_qoix_encode_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int64, pitches), descs, n, arr(C.c_int64, given),
                                                  out.data_ptr(), olen, st, None)
    torch.cuda.synchronize()
    return rc, list(st), list(olen), out.cpu().numpy(), offs, expect, refs


def compare(L, rc, st, olen, got, offs, expect, refs, names):
    bad = [k for k, r in enumerate(refs) if r is None]
    assert rc == (_capi.ERR_INVALID_ARG if bad else 0), (rc, L.gamut_hip_last_error())
    for k, r in enumerate(refs):
        name = names[k] if names else k
        assert st[k] == (0 if r is not None else _capi.ERR_INVALID_ARG), (name, st[k])
        assert olen[k] == (len(r) if r is not None else 0), (name, olen[k], r and len(r))
        if r is not None and not np.array_equal(got[offs[k]:offs[k] + len(r)], expect[offs[k]:offs[k] + len(r)]):
            d = int(np.flatnonzero(got[offs[k]:offs[k] + len(r)] != expect[offs[k]:offs[k] + len(r)])[0])
            assert False, f"{name}: first difference at file byte {d} of {len(r)}: {got[offs[k] + d]:02x}, expected {expect[offs[k] + d]:02x}"
    assert np.array_equal(got, expect), "a byte outside every output was written"     # the WHOLE allocation, guards included
    return [None if r is None else got[o:o + len(r)].tobytes() for r, o in zip(refs, offs)]


def check_batch(L, imgs, names=None, **kw):
    return compare(L, *encode_batch(L, imgs, **kw), names)


def both_modes(L, items, **kw):
    imgs, names = [im for _, im in items], [n for n, _ in items]
    check_batch(L, imgs, names, modes=[1] * len(imgs), **kw)
    return check_batch(L, imgs, names, modes=[0] * len(imgs), **kw)


@pytest.mark.parametrize("ch", [1, 2])
def test_every_named_case_in_one_call(L, S, ch):
    items = [(n, im) for n, im in cases.named(S) if im.shape[2] == ch]
    assert len(items) >= 60
    offs, _ = layout_outputs([1] * len(items))
    assert {o % 16 for o in offs} == set(range(16))                         # out_offset at every residue modulo 16
    files = both_modes(L, items)
    assert {f[16] for f in files} == {0, 1}                                 # stored and LZ4 files both


@pytest.mark.parametrize("mode", [0, 1])
def test_every_named_case_one_image_per_call(L, S, mode):
    items = cases.named(S)
    check_batch(L, [im for _, im in items], [n for n, _ in items], modes=[mode] * len(items), per_call=True)


def test_hand_worked_streams(L):
    files = check_batch(L, [im for _, im, _ in cases.HAND_WORKED], [n for n, _, _ in cases.HAND_WORKED], colorspace=[0] * len(cases.HAND_WORKED))
    for f, (name, im, stream) in zip(files, cases.HAND_WORKED):
        assert f[16] == 0 and f[25:].hex() == stream, name


def test_shapes_around_the_segment_size(L, S):
    assert S % 64 == 0 and S > 0
    both_modes(L, cases.geometry(S))


def test_runs_cut_and_carried_over_segments(L, S):
    both_modes(L, cases.runs(S))


def test_segment_boundaries_on_odd_nibbles(L, S):
    both_modes(L, cases.shared_bytes(S))


def test_op_thresholds_and_wraps(L):
    both_modes(L, cases.thresholds())


def test_container_choice_at_the_boundary(L):
    items = cases.boundary_images() + [cases.byu32_image()]
    files = check_batch(L, [im for _, im in items], [n for n, _ in items])
    for f, d in zip(files, cases.boundary_diffs()):
        assert f[16] == (1 if d < 0 else 0)


def layout_items(S):
    keep = ("geometry_3x40", "geometry_65x2", "geometry_65x40", "geometry_1x40", "pixels_%d_" % (S + 1), "pixels_%d_" % (2 * S + 1), "alpha_ramp_77")
    return [(n, im) for n, im in cases.geometry(S) if n.startswith(keep)]


@pytest.mark.parametrize("pitch_kind", ["tight", "padded", "negative"])
def test_layouts_with_sources_at_every_base_modulo_16(L, S, pitch_kind):
    items = layout_items(S)
    assert len(items) >= 12 and any(im.shape[0] > 1 for _, im in items)
    imgs, names = [im for _, im in items], [n for n, _ in items]
    for shift in range(16):
        check_batch(L, imgs, names, modes=[(k + shift) % 2 for k in range(len(imgs))], pitch_kind=pitch_kind, shift=shift)


def mixed_items(S):
    grey = [(n, im) for n, im in cases.geometry(S) if n.startswith(("geometry_65x", "geometry_3x", "pixels_"))]
    colour = [(n, im) for n, im in colour_cases.matrix_images((3, 65, 130)) if im.shape[0] > 1][:len(grey)]
    assert len(colour) >= 8
    out = []
    for k in range(max(len(grey), len(colour))):
        out += grey[k:k + 1] + colour[k:k + 1]
    return out


def test_grey_and_colour_images_in_one_call(L, S):
    items = mixed_items(S)
    assert {im.shape[2] for _, im in items} == {1, 2, 3, 4}
    both_modes(L, items)
    imgs = [im for _, im in items]
    check_batch(L, imgs, modes=[k // 2 % 2 for k in range(len(imgs))], pitch_kind="padded", shift=3)


def test_refused_images_do_not_disturb_their_neighbours(L, S):
    items = mixed_items(S)[:16]
    imgs = [im for _, im in items]
    files = check_batch(L, imgs, override={0: (0, 5, 1, 0, False), 2: (7, 0, 2, 0, False), 3: (7, 3, 5, 0, False), 4: (7, 3, 2, 3, False),
                                           6: (1, 357913942, 2, 0, False), 8: (20000, 20000, 1, 0, False), 10: (7, 3, 1, 0, True),
                                           12: (7, 3, 0, 0, False)}, bad_offset=(14,))
    assert sum(f is not None for f in files) == 7
    assert L.gamut_hip_last_error().startswith(b"image 0:")


def test_colour_only_batches_are_what_they_are_with_the_switch_off(L):
    items = [(n, im) for n, im in colour_cases.matrix_images((3, 65, 129)) if im.shape[0] > 1]
    on = both_modes(L, items)
    assert L.gamut_hip_qoix_set_plane(0) == 1
    try:
        off = both_modes(L, items)
    finally:
        assert L.gamut_hip_qoix_set_plane(1) == 0
    assert on == off


def test_with_the_switch_off_grey_images_are_refused_as_before(L, S):
    items = mixed_items(S)[:12]
    imgs = [im for _, im in items]
    assert L.gamut_hip_qoix_set_plane(0) == 1
    try:
        files = check_batch(L, imgs, expect_refused=True)
        assert sum(f is None for f in files) == sum(im.shape[2] < 3 for im in imgs) > 0 and any(f is not None for f in files)
        for ch in (1, 2):
            assert L.gamut_hip_qoix_encode_bound(C.byref(_capi.QoixDesc(5, 5, ch, 0, 0, 1.0, 96.0))) == -1
            px = np.zeros(64, np.uint8); n = C.c_int(-1)
            assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4 * ch, C.byref(_capi.QoixDesc(4, 4, ch, 0, 0, 1.0, 96.0)), C.byref(n)) and n.value == -1
    finally:
        assert L.gamut_hip_qoix_set_plane(1) == 0


def test_round_trip_through_the_gpu_decoder(L, S):
    items = [(n, im) for n, im in cases.geometry(S) if n.startswith(("geometry_65x", "pixels_", "flat_", "alpha_ramp"))] + cases.boundary_images()
    imgs = [im for _, im in items]
    files = check_batch(L, imgs, colorspace=[k % 2 for k in range(len(imgs))])
    assert {f[16] for f in files} == {0, 1}
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


def test_host_drop_in(L, S):
    free = C.CDLL(None).free
    for name, im in [(n, im) for n, im in cases.geometry(S) if n.startswith(("geometry_65x40", "pixels_%d_" % (S + 1)))]:
        h, w, ch = im.shape
        for mode in (0, 1):
            d = _capi.QoixDesc(w, h, ch, 0, mode, 2.0, 72.0)
            n = C.c_int(0)
            p = L.gamut_hip_qoix_write_to_mem(im.ctypes.data, w * ch, C.byref(d), C.byref(n))
            assert p, L.gamut_hip_last_error()
            assert C.string_at(p, n.value) == ref.encode(im, mode, par=2.0, dpi=72.0), name
            free(C.c_void_p(p))
        flipped = np.ascontiguousarray(im[::-1])                            # a negative pitch: row 0 is the last one in memory
        d = _capi.QoixDesc(w, h, ch, 1, 0, 1.0, 96.0)
        n = C.c_int(0)
        p = L.gamut_hip_qoix_write_to_mem(flipped.ctypes.data + (h - 1) * w * ch, -w * ch, C.byref(d), C.byref(n))
        assert p and C.string_at(p, n.value) == ref.encode(im, colorspace=1), name
        free(C.c_void_p(p))


@pytest.mark.parametrize("device", [False, True])
def test_image_save(L, S, device, tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    for tname, ch in (("l8", 1), ("la8", 2)):
        px = P.noisy(141, 37, ch, 50 + ch)                                  # more than one segment
        assert px.shape[0] * px.shape[1] > S
        im = gi.Image(device=device)
        assert im.loadFromMemory(ref.encode(px, 0, par=1.5, dpi=300.0))     # a file that carries par and dpi
        assert im.type == O.PT[tname] and im.isDevice == device
        assert np.array_equal(np.asarray(im.pixels()).reshape(px.shape), px)
        want = ref.encode(px, 0, par=im.pixelAspectRatio, dpi=im.dotsPerInchY)
        assert want[17:25] == struct.pack(">ff", 1.5, 300.0)
        enc = im.save_qoix_to_memory()
        assert enc == want, tname
        assert im.saveQOIXToMemory(12345) == want                           # flags are ignored
        path = tmp_path / f"x{ch}.qoix"
        assert im.saveQOIXToFile(path) and path.read_bytes() == want
        assert im.save_to_memory(gi.FORMAT_QOIX) is None                    # the generic entry does not dispatch QOIX
        assert im.isValid and im.errorMessage is None
        again = gi.Image(device=device)
        assert again.loadFromMemory(enc) and again.type == im.type and np.array_equal(np.asarray(again.pixels()), np.asarray(im.pixels()))
        if ch == 2:                                                         # lap8: 2 channels with colorspace 2, as saveQOIX writes it
            assert im.convertTo(O.PT["lap8"]) and im.type == O.PT["lap8"] and im.isDevice == device
            pre = np.asarray(im.pixels()).reshape(px.shape).copy()
            want = ref.encode(pre, 0, colorspace=2, par=im.pixelAspectRatio, dpi=im.dotsPerInchY)
            assert want[13] == 2 and want[15] == 2
            assert im.save_qoix_to_memory() == want
            assert not gi.Image(device=device).loadFromMemory(want)        # which qoiplane_decode refuses


def test_image_save_of_views(L):
    import oracle_lib as O
    from gamut_amd import image as gi
    px = P.flat_image(300, 5, 2, 61)
    up = gi.Image()                                                         # bottom-up view: a negative pitch
    mem = np.ascontiguousarray(px[::-1])
    assert up.createView(mem, 300, 5, O.PT["la8"], -600) and up.isStoredUpsideDown
    assert up.save_qoix_to_memory() == ref.encode(px, 0, par=up.pixelAspectRatio, dpi=up.dotsPerInchY)
    lap = gi.Image()
    assert lap.createView(np.ascontiguousarray(px), 300, 5, O.PT["lap8"], 600)
    assert lap.save_qoix_to_memory() == ref.encode(px, 0, colorspace=2, par=lap.pixelAspectRatio, dpi=lap.dotsPerInchY)
    layers = np.stack([P.noisy(70, 4, 1, 70 + k) for k in range(3)])
    lay = gi.Image()
    assert lay.createLayeredView(layers, 70, 4, 3, O.PT["l8"], 70, 280) and lay.layers == 3
    kw = dict(par=lay.pixelAspectRatio, dpi=lay.dotsPerInchY)
    assert lay.save_qoix_to_memory() == ref.encode(layers[0], 0, **kw)      # layer 0
    assert lay.layer(2).save_qoix_to_memory() == ref.encode(layers[2], 0, **kw)
