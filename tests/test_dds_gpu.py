"""The BC7 / DDS encoder on the GPU against the serial C restatement of the reference (tests/c/bc7_ref.c), byte for byte: the blocks
entry on every tile of tests/dds_cases.py and on the counts at which four tiles per wave can go wrong; the file entry on every small
size and source type, padded / negative pitches, every output residue, 600 tiny images in one call, refused images among good
neighbours; the host drop-in and the Image layer.  Output allocations are filled with 0xA5, carry guards and are compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc7_ref_c
import dds_cases as cases
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 1024


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


@pytest.fixture(scope="module")
def restated():
    tiles = cases.all_tiles()
    return tiles, bc7_ref_c.blocks(tiles)[0]


def arr(t, vals):
    return (t * len(vals))(*vals)


def encode_blocks(L, tiles, shift_in=0, shift_out=0):
    """one gamut_hip_bc7_encode_blocks_device call inside guarded allocations -> the (n, 16) blocks"""
    tiles = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 64)
    n = tiles.shape[0]
    src = torch.from_numpy(np.concatenate([np.zeros(shift_in, np.uint8), tiles.reshape(-1)])).cuda()
    out = torch.full((GUARD + shift_out + 16 * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.gamut_hip_bc7_encode_blocks_device(src.data_ptr() + shift_in, n, out.data_ptr() + GUARD + shift_out, None)
    torch.cuda.synchronize()
    assert rc == 0, L.gamut_hip_last_error()
    got = out.cpu().numpy()
    assert (got[:GUARD + shift_out] == 0xA5).all() and (got[GUARD + shift_out + 16 * n:] == 0xA5).all(), "a byte outside the blocks was written"
    return got[GUARD + shift_out:GUARD + shift_out + 16 * n].reshape(n, 16)


def assert_blocks(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        assert False, f"{what}: {bad.size} of {len(want)} blocks differ, first tile {int(bad[0])}: {got[bad[0]].tobytes().hex()} for {want[bad[0]].tobytes().hex()}"


def test_every_case_tile_in_one_call(L, restated):
    tiles, want = restated
    assert_blocks(encode_blocks(L, tiles), want, "all tiles")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
def test_tile_counts_around_a_wave(L, restated, n):
    tiles, want = restated
    start = 0 if n == 1000 else 600                                         # 600..: noise tiles, mode 1 among them
    assert_blocks(encode_blocks(L, tiles[start:start + n]), want[start:start + n], f"n = {n}")


def test_blocks_at_odd_addresses(L, restated):
    tiles, want = restated
    for shift_in, shift_out in ((1, 0), (0, 1), (3, 7), (2, 4)):
        assert_blocks(encode_blocks(L, tiles[590:660], shift_in, shift_out), want[590:660], f"shifts {shift_in}, {shift_out}")


def encode_batch(L, imgs, pitch_kind="tight", shift=0, override=None, residues=None):
    """One gamut_hip_dds_encode_batch_device call.  imgs: (h, w, comp) arrays; pitch_kind: tight, padded or negative; shift: the sources'
    base modulo 16; override: {index: (width, height, comp, null_source)} turns image `index` into a refused one; residues: the output
    offsets modulo 16, cycled.  -> (rc, statuses, lengths, the whole output allocation, offsets, the expected allocation, the files)"""
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
    refs = [None if k in override else bc7_ref_c.write_dds(im) for k, im in enumerate(imgs)]
    offs, opos = [], GUARD
    for k, im in enumerate(imgs):
        res = (1 + 2 * (k % 8)) if residues is None else residues[k % len(residues)]
        opos = (opos + 15) // 16 * 16 + res
        offs.append(opos)
        opos += bc7_ref_c.dds_size(im.shape[1], im.shape[0]) + 32 + k % 5     # a guard between neighbours too
    opos += GUARD
    expect = np.full(opos, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((opos,), 0xA5, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    olen = arr(C.c_int64, [-7] * n)
    st = arr(C.c_int, [77] * n)
    rc = L.gamut_hip_dds_encode_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int64, [p for _, p in places]), arr(C.c_int32, W), arr(C.c_int32, H),
                                             arr(C.c_int32, Cc), n, arr(C.c_int64, offs), out.data_ptr(), olen, st, None)
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


@pytest.mark.parametrize("comp", [1, 2, 3, 4])
def test_every_small_size(L, comp):
    """1..9 x 1..9: every way a width and a height can end inside a tile, one call per source type"""
    sizes = [(w, h) for h in range(1, 10) for w in range(1, 10)]
    check_batch(L, [cases.image(w, h, comp, 10 * comp) for w, h in sizes], [f"{w}x{h}x{comp}" for w, h in sizes])


def test_a_larger_odd_image(L):
    check_batch(L, [cases.image(257, 131, 3, 2)])


@pytest.mark.parametrize("pitch_kind,shift", [("padded", 0), ("negative", 0), ("padded", 5), ("negative", 11), ("tight", 3)])
def test_layouts(L, pitch_kind, shift):
    imgs = [cases.image(w, h, comp, 40 + comp) for comp in (1, 2, 3, 4) for w, h in ((13, 6), (4, 4), (31, 9))]
    check_batch(L, imgs, pitch_kind=pitch_kind, shift=shift)


def test_every_output_residue(L):
    imgs = [cases.image(9 + k % 4, 5 + k % 3, 1 + k % 4, 60 + k) for k in range(16)]
    check_batch(L, imgs, residues=list(range(16)))


def test_600_tiny_images_in_one_call(L):
    rng = np.random.default_rng(600)
    shapes = [(int(rng.integers(1, 10)), int(rng.integers(1, 10)), int(rng.integers(1, 5))) for _ in range(600)]
    check_batch(L, [cases.image(w, h, comp, k) for k, (w, h, comp) in enumerate(shapes)])


def test_refused_images_do_not_disturb_their_neighbours(L):
    imgs = [cases.image(11, 7, 1 + k % 4, 80 + k) for k in range(7)]
    check_batch(L, imgs, override={1: (0, 7, 2, False), 3: (11, 7, 5, False), 4: (11, 7, 1, True), 6: (11, -2, 3, False)})
    check_batch(L, imgs[:2], override={0: (11, 0, 1, False), 1: (11, 7, 0, False)})      # nothing left to launch


def test_count_zero(L):
    assert L.gamut_hip_dds_encode_batch_device(None, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.gamut_hip_bc7_encode_blocks_device(None, 0, None, None) == 0


def test_host_drop_in(L):
    for comp in (1, 2, 3, 4):
        im = cases.image(37, 10, comp, 90 + comp)
        h, w, _ = im.shape
        n = C.c_int(0)
        p = L.gamut_hip_dds_write_to_mem(im.ctypes.data, w * comp, w, h, comp, C.byref(n))
        assert p, L.gamut_hip_last_error()
        assert C.string_at(p, n.value) == bc7_ref_c.write_dds(im), comp
        C.CDLL(None).free(C.c_void_p(p))
        flipped = np.ascontiguousarray(im[::-1])                            # a negative pitch: row 0 is the last one in memory
        n = C.c_int(0)
        p = L.gamut_hip_dds_write_to_mem(flipped.ctypes.data + (h - 1) * w * comp, -w * comp, w, h, comp, C.byref(n))
        assert p and C.string_at(p, n.value) == bc7_ref_c.write_dds(im), comp
        C.CDLL(None).free(C.c_void_p(p))


def _file_that_loads_as(px):
    """a file the existing loaders turn into exactly these pixels, of the matching 8-bit type"""
    import tga_write_ref_c
    return tga_write_ref_c.encode(px, False)


@pytest.mark.parametrize("device", [False, True])
def test_image_save(L, device, tmp_path):
    import oracle_lib as O
    import tga_gen
    from gamut_amd import image as gi
    names = {1: "l8", 2: "la8", 3: "rgb8", 4: "rgba8"}
    for comp in (1, 2, 3, 4):
        im = gi.Image(device=device)
        if comp <= 2:                                                       # grey TGA files load as l8 / la8
            assert im.loadFromMemory(tga_gen.make(41, 10, 11, 8 * comp, policy="mixed", seed=50 + comp))
            px = np.asarray(im.pixels()).reshape(10, 41, comp).copy()
        else:
            px = cases.image(41, 10, comp, 50 + comp)
            assert im.loadFromMemory(_file_that_loads_as(px))
            assert np.array_equal(np.asarray(im.pixels()).reshape(px.shape), px)
        assert im.type == O.PT[names[comp]] and im.isDevice == device
        want = bc7_ref_c.write_dds(px)
        assert im.save_dds_to_memory() == want, comp
        assert im.saveDDSToMemory(12345) == want                            # flags are ignored
        path = tmp_path / f"x{comp}.dds"
        assert im.saveDDSToFile(path) and path.read_bytes() == want
        assert im.save_to_memory(gi.FORMAT_DDS) is None                     # the generic entry does not dispatch DDS
        assert im.isValid and im.errorMessage is None
        assert np.array_equal(np.asarray(im.pixels()).reshape(px.shape), px)
        again = gi.Image(device=device)
        assert not again.loadFromMemory(want)                               # and nothing loads one, as in the reference


def test_image_save_of_views(L):
    import oracle_lib as O
    from gamut_amd import image as gi
    px = cases.image(30, 5, 4, 61)
    up = gi.Image()                                                         # bottom-up view: a negative pitch
    mem = np.ascontiguousarray(px[::-1])
    assert up.createView(mem, 30, 5, O.PT["rgba8"], -120) and up.isStoredUpsideDown
    assert up.save_dds_to_memory() == bc7_ref_c.write_dds(px)
    layers = np.stack([cases.image(22, 6, 3, 70 + k) for k in range(3)])
    lay = gi.Image()
    assert lay.createLayeredView(layers, 22, 6, 3, O.PT["rgb8"], 66, 396) and lay.layers == 3
    assert lay.save_dds_to_memory() == bc7_ref_c.write_dds(layers[0])       # layer 0
    assert lay.layer(2).save_dds_to_memory() == bc7_ref_c.write_dds(layers[2])
