"""BMP on the GPU against the serial C restatement of the reference (tests/c/bmp_ref.c), byte for byte: the batched decode over every
variant of the generator and the widths at which a lane, a dword, a nibble or a bit runs out; truncated files; the all_a rule; the
batched encode at every source / destination alignment; the Image layer; BMP files in the mixed-format call."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import bmp_gen
import bmp_ref_c
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def decode_batch(L, files, req, at_end_of_buffer=False):
    """one gamut_hip_bmp_decode_batch_device call -> (rc, statuses, infos, whole output allocation, offsets, expected allocation)"""
    n = len(files)
    refs = [bmp_ref_c.load(f, req) for f in files]
    offs, pos = [], GUARD
    for r in refs:
        offs.append(pos)
        pos += (r[0].size if r is not None else 64) + GUARD
    expect = np.full(pos, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + r[0].size] = r[0].reshape(-1)
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
    info = (_capi.BmpInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_bmp_decode_batch_device(ptrs, lens, n, req, offa, out.data_ptr(), info, st, None)
    return rc, list(st), info, out.cpu().numpy(), offs, expect, refs


def check_batch(L, files, req, names=None):
    rc, st, info, got, offs, expect, refs = decode_batch(L, files, req)
    bad = [i for i, r in enumerate(refs) if r is None]
    assert rc == (st[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    for i, r in enumerate(refs):
        assert (st[i] == 0) == (r is not None), (i, names[i] if names else None, st[i])
        if r is None:
            assert st[i] == _capi.ERR_DECODE
            continue
        assert {k: int(getattr(info[i], k)) & 0xffffffff for k in bmp_ref_c.INFO_FIELDS} == r[1], (i, names[i] if names else None)
        assert np.array_equal(np.float32([info[i].pixels_per_meter_x, info[i].pixels_per_meter_y, info[i].pixel_aspect_ratio]), np.float32(r[2]))
    if not np.array_equal(got, expect):                                     # the WHOLE allocation, guards included
        for i, r in enumerate(refs):
            n = r[0].size if r is not None else 64
            assert np.array_equal(got[offs[i] - GUARD:offs[i] + n + GUARD], expect[offs[i] - GUARD:offs[i] + n + GUARD]), \
                (i, names[i] if names else None, "req", req, "first difference at", int(np.flatnonzero(got[offs[i] - GUARD:offs[i] + n + GUARD] != expect[offs[i] - GUARD:offs[i] + n + GUARD])[0]) - GUARD)
        assert False, "difference outside every image and its guards"
    return refs


@pytest.mark.parametrize("req", [0, 1, 2, 3, 4])
def test_decode_matrix(L, req):
    """every variant of the generator (header sizes, depths, masks, both row orders, short palettes, gaps) at every width of WIDTHS and
    heights 1 / 2 / 5, and at 1100 / 2053 (a row longer than one workgroup's span, a ragged last unit), in ONE call per req_comp"""
    files, names = [], []
    for w in WIDTHS:
        for h in (1, 2, 5):
            for name, f in bmp_gen.variants(w, h, seed=w * 8 + h):
                files.append(f); names.append(f"{name}_{w}x{h}")
    for w, h in ((1100, 2), (2053, 5)):
        for name, f in bmp_gen.variants(w, h, seed=w):
            files.append(f); names.append(f"{name}_{w}x{h}")
    refs = check_batch(L, files, req, names)
    assert sum(r is not None for r in refs) > len(files) * 0.8 and any(r is None for r in refs)   # (the 10-bit mask set is refused)


def test_mixed_batch_with_refused_and_empty_files(L):
    rng = np.random.default_rng(3)
    files = [bmp_gen.random_file(rng) for _ in range(61)]
    files.insert(5, b""); files.insert(9, bmp_gen.make(4, 4, 8, 40, compression=1)); files.insert(40, b"BM" + bytes(30))
    assert len(files) == 64
    for req in (0, 4):
        rc, st, info, got, offs, expect, refs = decode_batch(L, files, req)
        first_bad = min(i for i, r in enumerate(refs) if r is None)
        assert first_bad <= 5 and rc == st[first_bad] == _capi.ERR_DECODE
        assert L.gamut_hip_last_error().startswith(b"image %d:" % first_bad)
        assert [s == 0 for s in st] == [r is not None for r in refs]
        assert np.array_equal(got, expect)


def test_truncated_files(L):
    """cut inside the palette, in mid-row, one byte short: the reference's reader hands out zeros past the end"""
    files, names = [], []
    for w, h in ((9, 3), (33, 2), (1100, 2)):
        for name, f in bmp_gen.variants(w, h, seed=w + 100):
            off = int.from_bytes(f[10:14], "little")
            for cut in sorted({off - 5, off + 1, off + (len(f) - off) // 2, off + (len(f) - off) // 2 + 1, len(f) - 1, len(f) - 3}):
                files.append(f[:cut]); names.append(f"{name}_{w}x{h}_cut{cut}")
    for req in (0, 4, 1):
        check_batch(L, files, req, names)


@pytest.mark.parametrize("w,h", [(3, 2), (2053, 5)])
def test_all_a_rule(L, w, h):
    import test_bmp_cpu as T
    cases = T._all_a_files(w, h)
    files = [f for _, f, _ in cases]
    files.insert(2, bmp_gen.make(w, h, 24, 40, seed=1))                     # an unaffected image in the same batch
    for req in (4, 2, 3, 0, 1):
        refs = check_batch(L, files, req)
        if req in (4, 0):
            assert (refs[0][0][..., 3] == 255).all() and (refs[1][0][..., 3] == 0).sum() == w * h - 1 and (refs[3][0][..., 3] == 0).all()
        if req == 2:
            assert (refs[0][0][..., 1] == 255).all() and (refs[3][0][..., 1] == 0).all()


def test_decode_runs_at_every_output_alignment(L):
    """a row of 1 pixel (3 bytes: shorter than the 16-byte head of its store), of 5 (head and tail, no 16-byte body) and of 1025 (one
    pixel into a second 1024-pixel unit) in one batch of three 2-row files at req_comp 3, with EVERY out_offset at residue r modulo 16,
    r = 0..15 in turn; the whole allocation, canaries between and around the images included, against the reference"""
    files = [bmp_gen.make(w, 2, 24, 40, top_down=w == 5, seed=w) for w in (1, 5, 1025)]
    refs = [bmp_ref_c.load(f, 3)[0] for f in files]
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
        info = (_capi.BmpInfo * 3)(); st = (C.c_int * 3)(77, 77, 77)
        rc = L.gamut_hip_bmp_decode_batch_device(ptrs, lens, 3, 3, (C.c_int64 * 3)(*offs), out.data_ptr(), info, st, None)
        assert rc == 0 and list(st) == [0, 0, 0], (r, L.gamut_hip_last_error())
        bad = np.flatnonzero(out.cpu().numpy() != expect)
        assert bad.size == 0, ("residue", r, "first difference at", int(bad[0]), "offsets", offs)


def encode_batch(L, imgs, pitch_kind, src_shift, out_mod, ppm):
    """imgs: list of (h, w, c) arrays, or (w, h, c) tuples for shapes that must be refused"""
    n = len(imgs)
    srcs, ptrs, pitches, W, H, Cc, keep = [], [], [], [], [], [], []
    for im in imgs:
        if isinstance(im, tuple):
            w, h, c = im
            t = torch.zeros(64, dtype=torch.uint8, device="cuda")
            keep.append(t); ptrs.append(t.data_ptr()); pitches.append(max(w * c, 1)); W.append(w); H.append(h); Cc.append(c)
            continue
        h, w, c = im.shape
        row = w * c
        pitch = row if pitch_kind == "tight" else row + 7
        host = np.full(src_shift + pitch * h + 16, 0x5A, np.uint8)
        for y in range(h):
            yy = h - 1 - y if pitch_kind == "negative" else y
            host[src_shift + yy * pitch:src_shift + yy * pitch + row] = im[y].reshape(-1)
        t = torch.from_numpy(host).cuda()
        keep.append(t)
        ptrs.append(t.data_ptr() + src_shift + ((h - 1) * pitch if pitch_kind == "negative" else 0))
        pitches.append(-pitch if pitch_kind == "negative" else pitch); W.append(w); H.append(h); Cc.append(c)
    offs, pos = [], GUARD
    for k in range(n):
        pos = (pos + 15) // 16 * 16 + (out_mod + k) % 16 if out_mod >= 0 else pos
        offs.append(pos)
        pos += max(bmp_ref_c.bound(W[k], H[k], Cc[k]), 64) + GUARD
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    arr = lambda t, v: (t * n)(*v)
    olen = (C.c_int64 * n)(*([-1] * n)); st = (C.c_int * n)(*([77] * n))
    px = arr(C.c_int32, [ppm] * n)
    rc = L.gamut_hip_bmp_encode_batch_device(arr(C.c_void_p, ptrs), arr(C.c_int64, pitches), arr(C.c_int32, W), arr(C.c_int32, H), arr(C.c_int32, Cc),
                                             px if ppm else None, px if ppm else None, n, arr(C.c_int64, offs), out.data_ptr(), olen, st, None)
    torch.cuda.synchronize()
    return rc, list(st), list(olen), out.cpu().numpy(), offs


@pytest.mark.parametrize("comp", [3, 4])
@pytest.mark.parametrize("pitch_kind", ["tight", "padded", "negative"])
def test_encode_matrix(L, comp, pitch_kind):
    rng = np.random.default_rng(comp * 10 + len(pitch_kind))
    shapes = [(w, h) for w in WIDTHS for h in (1, 2, 5)] + [(1100, 2), (2053, 5)]
    imgs = [rng.integers(0, 256, (h, w, comp), dtype=np.uint8) for w, h in shapes]
    imgs.insert(7, (4, 4, 2)); imgs.insert(20, (0, 4, comp)); imgs.insert(30, (32768, 1, comp))      # refused shapes in mid-batch
    for src_shift, out_mod, ppm in ((0, 0, 0), (1, 1, 3780), (2, 2, 0), (3, 3, 3780)):
        rc, st, olen, got, offs = encode_batch(L, imgs, pitch_kind, src_shift, out_mod, ppm)
        assert rc == _capi.ERR_INVALID_ARG and L.gamut_hip_last_error().startswith(b"image 7:")
        expect = np.full(got.size, 0xA5, np.uint8)
        for k, im in enumerate(imgs):
            if isinstance(im, tuple):
                assert st[k] == _capi.ERR_INVALID_ARG and olen[k] == 0
                continue
            f = bmp_ref_c.write(im, ppm, ppm)
            assert st[k] == 0 and olen[k] == len(f) == bmp_ref_c.bound(im.shape[1], im.shape[0], comp)
            expect[offs[k]:offs[k] + len(f)] = np.frombuffer(f, np.uint8)
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, (src_shift, out_mod, "first difference at", int(bad[0]), [k for k in range(len(offs)) if offs[k] <= bad[0]][-1:])


def test_encode_runs_at_every_output_alignment(L):
    """rgb8 images of 1 and 5 pixels by 2 rows (bodies of 8 and 32 bytes behind the 122-byte header), each file at every residue
    modulo 16 in turn: 16 launches, the whole allocation with its 0xA5 fill against the reference's files"""
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, (2, w, 3), dtype=np.uint8) for w in (1, 5)]
    want = [np.frombuffer(bmp_ref_c.write(im, 0, 0), np.uint8) for im in imgs]
    seen = [set(), set()]
    for r in range(16):
        rc, st, olen, got, offs = encode_batch(L, imgs, "tight", 0, r, 0)
        assert rc == 0 and st == [0, 0] and olen == [f.size for f in want]
        expect = np.full(got.size, 0xA5, np.uint8)
        for k, f in enumerate(want):
            expect[offs[k]:offs[k] + f.size] = f
            seen[k].add(offs[k] % 16)
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, ("residue", r, "first difference at", int(bad[0]), "offsets", offs)
    assert seen == [set(range(16))] * 2


def test_round_trip_on_the_device(L):
    from PIL import Image
    rng = np.random.default_rng(9)
    for comp in (3, 4):
        imgs = [rng.integers(0, 256, (h, w, comp), dtype=np.uint8) for w, h in ((1, 1), (5, 3), (33, 5), (1100, 2), (257, 7))]
        rc, st, olen, got, offs = encode_batch(L, imgs, "tight", 0, 0, 2835)
        assert rc == 0
        files = [got[o:o + n].tobytes() for o, n in zip(offs, olen)]
        rc, st, info, out, doffs, expect, refs = decode_batch(L, files, 0)
        assert rc == 0
        for k, im in enumerate(imgs):
            assert info[k].channels_in_file == comp and (info[k].width, info[k].height) == (im.shape[1], im.shape[0])
            assert np.array_equal(out[doffs[k]:doffs[k] + im.size].reshape(im.shape), im)
            pil = Image.open(io.BytesIO(files[k])); pil.load()
            assert np.array_equal(np.asarray(pil.convert("RGBA" if comp == 4 else "RGB")), im)
        n = C.c_int(0)                                                     # the host drop-in
        p = L.gamut_hip_bmp_write_to_mem(imgs[2].ctypes.data, imgs[2].shape[1] * comp, imgs[2].shape[1], imgs[2].shape[0], comp, 2835, 2835, C.byref(n))
        assert p and C.string_at(p, n.value) == files[2]
        C.CDLL(None).free(C.c_void_p(p))


@pytest.mark.parametrize("device", [False, True])
def test_image_load_and_save(L, device, tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    names = {1: "l8", 2: "la8", 3: "rgb8", 4: "rgba8"}
    files = [bmp_gen.make(37, 5, 8, 40, ppm=(3780, 2835), seed=1), bmp_gen.make(33, 4, 24, 108, top_down=True, seed=2),
             bmp_gen.make(16, 3, 32, 40, ppm=(0, 2835), seed=3), bmp_gen.make(9, 2, 16, 56, 3, bmp_gen.MASK_SETS_16[2], seed=4)]
    for f in files:
        for flags, req in ((0, 0), (gi.LOAD_GREYSCALE, 1), (gi.LOAD_ALPHA, None), (gi.LOAD_RGB | gi.LOAD_ALPHA, 4), (gi.LOAD_16BIT, 0), (gi.LOAD_GREYSCALE | gi.LOAD_NO_ALPHA, 1)):
            im = gi.Image(device=device)
            assert im.loadFromMemory(f, flags), im.errorMessage
            rq = L.gamut_compute_requested_image_components(flags)
            rq = 0 if rq == -1 else rq
            ref, info, dens = bmp_ref_c.load(f, rq)
            comps = ref.shape[2]
            want_type = L.gamut_apply_load_flags(O.PT[names[comps]], flags)
            assert (im.type, im.width, im.height, im.isDevice) == (want_type, info["width"], info["height"], device)
            exp = O.scanlines_convert(names[comps], ref.reshape(-1), O.PIXEL_TYPES[want_type], info["width"], info["height"]) if want_type != O.PT[names[comps]] else ref
            assert np.array_equal(np.asarray(im.pixels()).reshape(-1).view(np.uint8), np.asarray(exp).reshape(-1).view(np.uint8))
            assert im.pixelAspectRatio == np.float32(dens[2]) and im.dotsPerInchY == (np.float32(-1) if dens[1] == -1 else np.float32(dens[1]) / np.float32(39.37007874))
    for comp in (3, 4):
        px = np.random.default_rng(comp).integers(0, 256, (6, 21, comp), dtype=np.uint8)
        f = bmp_ref_c.write(px, 3780, 2835)
        im = gi.Image(device=device)
        assert im.loadFromMemory(f, 0) and im.type == O.PT[names[comp]]
        enc = im.save_bmp_to_memory()
        ppm_y = int(np.round(np.float32(2835) / np.float32(39.37007874) * np.float32(39.37007874)))
        ppm_x = int(np.round(np.float32(2835) / np.float32(39.37007874) * (np.float32(3780) / np.float32(2835)) * np.float32(39.37007874)))
        assert enc == bmp_ref_c.write(px, ppm_x, ppm_y)
        path = tmp_path / f"x{comp}.bmp"
        assert im.saveBMPToFile(path) and path.read_bytes() == enc
        assert im.save_to_memory(7) is None                                 # the generic entry does not dispatch BMP
        again = gi.Image(device=device)
        assert again.loadFromMemory(enc) and np.array_equal(np.asarray(again.pixels()).reshape(px.shape), px)


@pytest.mark.parametrize("req", [3, 4])
def test_bmp_files_in_the_mixed_format_call(L, req):
    import gen
    from PIL import Image
    rng = np.random.default_rng(req)
    a = gen.synth_rgb(45, 31, 3)
    bio = io.BytesIO(); Image.fromarray(a).save(bio, "PNG"); png = bio.getvalue()
    bio = io.BytesIO(); Image.fromarray(a).save(bio, "JPEG", quality=90); jpg = bio.getvalue()
    qoi = gen.qoi_encode(a)
    bmps = [bmp_gen.make(45, 31, 24, 40, seed=1), bmp_gen.make(17, 3, 8, 12, seed=2), bmp_gen.make(64, 2, 32, 108, 3, bmp_gen.MASK_SETS_32[1], seed=3),
            bmp_gen.make(5, 5, 4, 40, compression=2)]

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
    plain = [jpg, png, qoi, png, jpg]
    rc0, st0, info0, out0, offs0 = run(plain)
    assert rc0 == 0 and st0 == [0] * 5 and [i.format for i in info0] == [0, 1, 2, 1, 0]
    mixed = [bmps[0], jpg, png, bmps[1], qoi, bmps[3], png, bmps[2], jpg]
    rc, st, info, out, offs = run(mixed)
    assert rc == _capi.ERR_DECODE and st == [0, 0, 0, 0, 0, _capi.ERR_DECODE, 0, 0, 0] and L.gamut_hip_last_error().startswith(b"image 5:")
    assert [i.format for i in info] == [7, 0, 1, 7, 2, 7, 1, 7, 0]
    expect = np.full(out.size, 0xA5, np.uint8)
    npx = 45 * 31 * req
    for k, src in ((1, 0), (2, 1), (4, 2), (6, 3), (8, 4)):                 # the other formats: what the BMP-free batch gave
        expect[offs[k]:offs[k] + npx] = out0[offs0[src]:offs0[src] + npx]
    for k in (0, 3, 7):
        r = bmp_ref_c.load(mixed[k], req)
        expect[offs[k]:offs[k] + r[0].size] = r[0].reshape(-1)
        assert (info[k].width, info[k].height, info[k].channels_in_file, info[k].channels) == (r[1]["width"], r[1]["height"], r[1]["channels_in_file"], req)
    assert np.array_equal(out, expect)
    assert np.array_equal(out0[offs0[1]:offs0[1] + npx].reshape(31, 45, req)[..., :3], a)              # (the PNG leg, as a sanity anchor)
