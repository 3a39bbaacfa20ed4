"""SQZ encode on the GPU, bit for bit against the two restatements of the reference's encoder (tests/c/sqz_ref.c through
tests/c/sqz_ref_fwd.c, and tests/sqz_encode_ref.py): the front half (gamut_hip_sqz_analyze_batch_device from pixels,
gamut_hip_sqz_dwt_batch_device from planes), the file-level batch call, the round trip through the GPU decoder and the Image layer.
Coefficient and file buffers are filled with a sentinel, carry guards and are compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import sqz_cases
import sqz_encode_ref as P
import sqz_ref_c as R
import sqz_ref_fwd_c as F
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 512                                                                 # int16 elements / bytes around every image's output
SENTINEL = 0x5A5A
TW, TH = 128, 16                                                            # the level kernel's tile (sqz_encode.hip: kTW, kTH)
_refs = {}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def planes_of(mode):
    return 1 if mode == 0 else 3


def reference(px, mode, levels, python):
    """both readings' coefficients for a picture, computed once and shared; they must agree"""
    key = (px.tobytes(), px.shape, mode, levels)
    if key not in _refs:
        co = F.analyze(px, mode, levels)
        if python:
            h, w = px.shape[:2]
            assert np.array_equal(P.analyze(px, mode, P.clamp_levels(w, h, levels)), co)
        co.setflags(write=False)
        _refs[key] = co
    return _refs[key]


def fill_descs(items):
    n = len(items)
    descs = (_capi.SqzEncodeDesc * n)()
    for k, it in enumerate(items):
        descs[k].width, descs[k].height, descs[k].color_mode, descs[k].levels = it["w"], it["h"], it["mode"], it["levels"]
        descs[k].scan_order, descs[k].subsampling, descs[k].budget = it.get("scan", 0), it.get("ss", 0), it.get("budget", 0)
    return descs


def upload(items):
    """the pictures in ONE device buffer: tight, padded ("pad"), bottom-up ("neg") or at an odd address ("odd") -> (buffer, pointers, pitches)"""
    blobs, where, pos = [], [], 0
    for it in items:
        px = it.get("px")
        if px is None:
            where.append(None)
            continue
        h, w = px.shape[:2]
        row = w * planes_of(it["mode"])
        kind = it.get("src", "tight")
        pitch = row + (5 if kind == "pad" else 0)
        pos = (pos + 15) // 16 * 16 + (1 if kind == "odd" else 0)
        mem = np.full(h * pitch, 0xEE, np.uint8).reshape(h, pitch)
        mem[:, :row] = (px[::-1] if kind == "neg" else px).reshape(h, row)
        blobs.append((pos, mem.reshape(-1)))
        where.append((pos + (h - 1) * pitch, -pitch) if kind == "neg" else (pos, pitch))
        pos += mem.size
    host = np.full(pos + 16, 0xEE, np.uint8)
    for at, mem in blobs:
        host[at:at + mem.size] = mem
    dev = torch.from_numpy(host).cuda()
    ptrs = (C.c_void_p * len(items))(*[None if wh is None else dev.data_ptr() + wh[0] for wh in where])
    pitches = (C.c_int64 * len(items))(*[0 if wh is None else wh[1] for wh in where])
    return dev, ptrs, pitches


def coeff_layout(items):
    offs, pos = [], GUARD + 1
    for it in items:
        offs.append(it.get("offset", pos))
        pos += planes_of(it["mode"] & 3) * it["w"] * it["h"] + GUARD + 1     # odd element offsets
    return offs, pos


def check_analyze(L, items, python=True):
    """one gamut_hip_sqz_analyze_batch_device call; items carry px, mode, levels and maybe src / want (a status) / offset"""
    n = len(items)
    for it in items:
        if "px" in it and it["px"] is not None:
            it["h"], it["w"] = it["px"].shape[:2]
    offs, total = coeff_layout(items)
    expect = np.full(total, SENTINEL, np.uint16).view(np.int16)
    for it, o in zip(items, offs):
        if not it.get("want"):
            co = reference(it["px"], it["mode"], it["levels"], python)
            expect[o:o + co.size] = co
    dev, ptrs, pitches = upload(items)
    out = torch.from_numpy(np.full(total, SENTINEL, np.uint16).view(np.int16).copy()).cuda()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_analyze_batch_device(ptrs, pitches, fill_descs(items), n, out.data_ptr(), (C.c_int64 * n)(*offs), st, None)
    torch.cuda.synchronize()
    want = [it.get("want", 0) for it in items]
    bad = [i for i, w in enumerate(want) if w]
    assert rc == (want[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    assert list(st) == want
    got = out.cpu().numpy()
    if not np.array_equal(got, expect):
        first = int(np.flatnonzero(got != expect)[0])
        k = max([i for i in range(n) if offs[i] - GUARD <= first], default=0)
        it = items[k]
        at = first - offs[k]
        assert False, ("image", k, it["w"], it["h"], it["mode"], it["levels"], it.get("src"), "plane", at // (it["w"] * it["h"]), "row", at % (it["w"] * it["h"]) // it["w"],
                       "column", at % it["w"], "got", got[first:first + 6].tolist(), "want", expect[first:first + 6].tolist())


def item(w, h, mode, levels, seed=0, **kw):
    return dict(px=sqz_cases.picture(w, h, planes_of(mode), seed), mode=mode, levels=levels, **kw)


def test_analyze_every_mode_on_the_geometry_list(L):
    items = []
    for k, (w, h, lv) in enumerate(((16, 16, 1), (17, 16, 1), (16, 17, 1), (19, 23, 1), (31, 33, 1), (32, 33, 2), (47, 32, 2), (64, 40, 3), (128, 72, 4), (300, 130, 5))):
        for mode in range(4):
            items.append(item(w, h, mode, lv, 300 + k))
    check_analyze(L, items)


def test_analyze_around_the_tile(L):
    """sides one below, at and one above the tile's width and height, and twice those; the deepest level each size admits"""
    items = []
    for k, (w, h) in enumerate(((TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW - 1, 2 * TH - 1), (2 * TW, 2 * TH), (2 * TW + 1, 2 * TH + 1),
                                (TH - 1, TW + 1), (2 * TH + 1, 2 * TW - 1))):
        items.append(item(w, h, 0, 8, 400 + k))
        items.append(item(w, h, 1 + k % 3, 8, 420 + k))
    check_analyze(L, items)


def test_analyze_2048_square_grey_eight_levels(L):
    check_analyze(L, [item(2048, 2048, 0, 8, 77)])


def test_analyze_pitches_and_addresses(L):
    items = []
    for k, kind in enumerate(("pad", "neg", "odd")):
        for mode in range(4):
            items.append(item(47, 32, mode, 2, 500 + k, src=kind))
        items.append(item(300, 130, 2, 5, 510 + k, src=kind))
    check_analyze(L, items)


def test_analyze_forty_images_some_of_them_refused(L):
    rng = np.random.default_rng(9)
    items = []
    for k in range(40):
        w, h = int(rng.integers(8, 150)), int(rng.integers(8, 90))
        it = item(w, h, k % 4, 1 + k % 8, 600 + k, src=("tight", "pad", "neg", "odd")[(k // 4) % 4])
        if k in (0, 13):                                                    # a colour mode that does not exist: no pixels to lay out either
            it["px"], it["w"], it["h"], it["mode"], it["want"] = None, w, h, 4 if k == 0 else -1, _capi.ERR_INVALID_ARG
        if k == 7:
            it["levels"], it["want"] = 0, _capi.ERR_INVALID_ARG
        if k == 21:
            it["levels"], it["want"] = 9, _capi.ERR_INVALID_ARG
        if k == 30:
            it["offset"], it["want"] = -8, _capi.ERR_INVALID_ARG
        if k == 33:
            it["px"], it["w"], it["h"], it["want"] = None, w, h, _capi.ERR_INVALID_ARG
        if k == 39:
            it["scan"], it["want"] = 4, _capi.ERR_INVALID_ARG
        items.append(it)
    for w, h in ((7, 16), (16, 7), (65536, 8)):
        items.append(dict(px=None, w=w, h=h, mode=0, levels=1, want=_capi.ERR_INVALID_ARG, offset=5))
    assert sum(1 for it in items if it.get("want")) == 10
    check_analyze(L, items)


def test_analyze_every_colour_there_is(L):
    """all 2^24 colours in one 4096 x 4096 Oklab image, two levels: every input SQZ_i32_cbrt_01 can get from 8-bit pixels.  Against the C
    reading alone (the Python one agrees with it on the other tests' pictures and takes too long here)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8).reshape(4096, 4096, 3)
    check_analyze(L, [dict(px=px, mode=2, levels=2)], python=False)


def check_dwt(L, items):
    """one gamut_hip_sqz_dwt_batch_device call on [(planes (p, h, w) int16, levels)]"""
    n = len(items)
    its = [dict(w=p.shape[2], h=p.shape[1], mode=0 if p.shape[0] == 1 else 1, levels=lv) for p, lv in items]
    offs, total = coeff_layout(its)
    expect = np.full(total, SENTINEL, np.uint16).view(np.int16)
    src = np.full(total, 0x1111, np.int16)
    for (p, lv), it, o in zip(items, its, offs):
        want = F.forward(p, it["w"], it["h"], lv)
        assert np.array_equal(P.dwt(p, it["w"], it["h"], P.clamp_levels(it["w"], it["h"], lv)), want)       # the two readings
        expect[o:o + want.size] = want
        src[o:o + p.size] = p.reshape(-1)
    dsrc = torch.from_numpy(src).cuda()
    out = torch.from_numpy(np.full(total, SENTINEL, np.uint16).view(np.int16).copy()).cuda()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_dwt_batch_device(dsrc.data_ptr(), fill_descs(its), n, out.data_ptr(), (C.c_int64 * n)(*offs), st, None)
    torch.cuda.synchronize()
    assert rc == 0 and list(st) == [0] * n, L.gamut_hip_last_error()
    assert np.array_equal(dsrc.cpu().numpy(), src)                          # the input planes are only read
    got = out.cpu().numpy()
    if not np.array_equal(got, expect):
        first = int(np.flatnonzero(got != expect)[0])
        k = max([i for i in range(n) if offs[i] - GUARD <= first], default=0)
        at = first - offs[k]
        assert False, ("image", k, its[k], "plane", at // (its[k]["w"] * its[k]["h"]), "row", at % (its[k]["w"] * its[k]["h"]) // its[k]["w"], "column", at % its[k]["w"],
                       "got", got[first:first + 6].tolist(), "want", expect[first:first + 6].tolist())


def test_dwt_on_random_full_range_planes(L):
    rng = np.random.default_rng(3)
    items = []
    for (w, h, lv, p) in ((16, 16, 1, 1), (17, 19, 1, 3), (33, 31, 2, 1), (64, 40, 3, 3), (129, 35, 3, 1), (300, 130, 5, 3), (258, 257, 6, 1)):
        items.append((rng.integers(-32768, 32768, (p, h, w)).astype(np.int16), lv))
    check_dwt(L, items)


def test_dwt_on_constructed_extremes(L):
    """±32767 checkerboards, alternating rows and columns, all -32768 and single spikes at 64 x 40 (3 levels) and 33 x 31 (1 level).

    This tells the two readings of the horizontal pass apart.  Take a row -32768, 32767, -32768, 32767, ..: every high value is the int
    32767 + 32768 = 65535, stored as the short -1.  The reference keeps the ints in its loop, so low[2] = -32768 + ((65535 + 65535 +
    2) >> 2) = 0; a pass that truncated its running values like its stores would give -32768 + ((-1 - 1 + 2) >> 2) = -32768.  (low[0],
    low[1] and the last low value of the row DO see the truncated -1: cf1 is assigned from the cast at i = 0 and the tail reads
    h_band[w - 1] back.)"""
    row = np.array([[-32768, 32767] * 8], np.int16)
    P.horizontal_pass(row)
    assert row[0, 2] == 0 and row[0, 8:].tolist() == [-1] * 8 and row[0, 0] == -32768 and row[0, 1] == -16384
    items = []
    for (w, h, lv) in ((64, 40, 3), (33, 31, 1)):
        yy, xx = np.mgrid[0:h, 0:w]
        board = np.where((xx + yy) & 1, 32767, -32767)
        for p in (board, -board, np.where(yy & 1, 32767, -32767), np.where(xx & 1, 32767, -32768), np.where(xx & 1, -32768, 32767),
                  np.where(yy & 1, -32768, 32767), np.full((h, w), -32768), np.full((h, w), 32767)):
            items.append((p.astype(np.int16)[None], lv))
        for (y, x, v) in ((0, 0, 32767), (h - 1, w - 1, -32768), (h // 2, w // 2 + 1, -32768), (1, w - 2, 32767)):
            p = np.zeros((1, h, w), np.int16)
            p[0, y, x] = v
            items.append((p, lv))
    check_dwt(L, items)


def encode_batch(L, items):
    """one gamut_hip_sqz_encode_batch_device call -> the files; the host output buffer is compared whole"""
    n = len(items)
    for it in items:
        it["h"], it["w"] = it["px"].shape[:2]
    want = [R.encode(it["px"], it["mode"], it["levels"], it["scan"], it["ss"], it["budget"]) for it in items]
    offs, pos = [], GUARD
    for k, it in enumerate(items):
        pos += 1 + 2 * (k % 8)
        offs.append(pos)
        pos += it["budget"] + GUARD
    expect = np.full(pos, 0xA5, np.uint8)
    for f, o in zip(want, offs):
        expect[o:o + len(f)] = np.frombuffer(f, np.uint8)
    dev, ptrs, pitches = upload(items)
    out = np.full(pos, 0xA5, np.uint8)
    lens = (C.c_int64 * n)(*([-1] * n))
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_encode_batch_device(ptrs, pitches, fill_descs(items), n, (C.c_int64 * n)(*offs), out.ctypes.data, lens, st, None)
    assert rc == 0 and list(st) == [0] * n, L.gamut_hip_last_error()
    for k in range(n):
        assert lens[k] == len(want[k]), (k, items[k]["w"], items[k]["h"], items[k]["mode"], items[k]["scan"], items[k]["budget"], lens[k], len(want[k]))
    assert np.array_equal(out, expect)                                      # nothing outside [offset, offset + length)
    return want


def lossless_budget(px):
    return 64 + px.size * 3


def test_encode_batch_the_mode_scan_budget_matrix(L):
    items = []
    for mode in range(4):
        px = sqz_cases.picture(16, 16, planes_of(mode), 40 + mode)
        for scan in range(4):
            for ss in (0, 1):
                for b in (7, 8, 9, 16, 40, 100, 300, 1000, lossless_budget(px)):
                    items.append(dict(px=px, mode=mode, levels=1, scan=scan, ss=ss, budget=b))
    for k, (w, h, lv) in enumerate(((17, 16, 1), (19, 23, 1), (32, 33, 2), (47, 32, 2), (64, 40, 3), (128, 72, 4))):
        for mode in (k % 4, 2):
            px = sqz_cases.picture(w, h, planes_of(mode), 200 + k)
            for b in (100, 1000, lossless_budget(px)):
                items.append(dict(px=px, mode=mode, levels=lv, scan=(k + mode) % 4, ss=k & 1, budget=b, src=("pad", "neg", "odd")[k % 3]))
    encode_batch(L, items)


def test_encode_batch_every_budget_of_one_file_and_the_way_back(L):
    """16 x 17 Oklab: every byte budget from 7 to the lossless length in one call -- cuts inside sorting passes, inside refinement passes
    and between them -- each the prefix of the lossless file; then gamut_hip_sqz_decode_batch_device on a share of the files"""
    px = sqz_cases.picture(16, 17, 3, 32)
    full = sqz_cases.prefix_files()[1]
    items = [dict(px=px, mode=2, levels=1, scan=R.SNAKE, ss=1, budget=b) for b in range(7, len(full) + 1)]
    files = encode_batch(L, items)
    assert files[-1] == full and all(f == full[:7 + k] for k, f in enumerate(files))
    files = files[::17] + [full]
    px2 = sqz_cases.picture(128, 72, 1, 9)
    files += encode_batch(L, [dict(px=px2, mode=0, levels=4, scan=R.HILBERT, ss=0, budget=b) for b in (500, lossless_budget(px2))])
    n = len(files)
    want = [R.load(f)[0] for f in files]
    offs, pos = [], 64
    for p in want:
        offs.append(pos)
        pos += p.size + 64
    expect = np.full(pos, 0xA5, np.uint8)
    for p, o in zip(want, offs):
        expect[o:o + p.size] = p.reshape(-1)
    bufs = [np.frombuffer(f, np.uint8).copy() for f in files]
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    st = (C.c_int * n)()
    rc = L.gamut_hip_sqz_decode_batch_device((C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[len(f) for f in files]), n,
                                             (C.c_int64 * n)(*offs), out.data_ptr(), None, st, None)
    torch.cuda.synchronize()
    assert rc == 0 and list(st) == [0] * n
    assert np.array_equal(out.cpu().numpy(), expect)


def test_encode_batch_refusals_and_the_host_drop_in(L):
    px = sqz_cases.picture(47, 32, 3, 7)
    good = dict(px=px, mode=2, levels=7, scan=1, ss=1, budget=300)
    items = [dict(good), dict(good, budget=6), dict(good), dict(good, mode=5)]
    for it in items:
        it["h"], it["w"] = 32, 47
    dev, ptrs, pitches = upload([dict(it, mode=2) for it in items])
    out = np.full(4 * 1024, 0xA5, np.uint8)
    lens = (C.c_int64 * 4)(*([-1] * 4))
    st = (C.c_int * 4)(*([77] * 4))
    rc = L.gamut_hip_sqz_encode_batch_device(ptrs, pitches, fill_descs(items), 4, (C.c_int64 * 4)(0, 1024, 2048, 3072), out.ctypes.data, lens, st, None)
    assert rc == _capi.ERR_INVALID_ARG and L.gamut_hip_last_error().startswith(b"image 1:")
    assert list(st) == [0, _capi.ERR_INVALID_ARG, 0, _capi.ERR_INVALID_ARG] and list(lens) == [300, 0, 300, 0]
    want = R.encode(px, 2, 7, 1, 1, 300)
    assert out[:300].tobytes() == want == out[2048:2348].tobytes()
    assert (out[300:2048] == 0xA5).all() and (out[2348:] == 0xA5).all()
    # gamut_hip_sqz_write_to_mem: host pixels, a bottom-up view
    d = fill_descs([good | dict(w=47, h=32)])
    flipped = np.ascontiguousarray(px[::-1])
    n = C.c_int(0)
    p = L.gamut_hip_sqz_write_to_mem(flipped.ctypes.data + 31 * 141, -141, d, C.byref(n))
    assert p and C.string_at(p, n.value) == want, L.gamut_hip_last_error()
    C.CDLL(None).free(C.c_void_p(p))
    d[0].budget = 6
    assert not L.gamut_hip_sqz_write_to_mem(px.ctypes.data, 141, d, C.byref(n)) and n.value == 0


def calm(w, h, seed):
    """a picture that ENCODE_SQZ_QUALITY_MAX (about 8 bits per pixel) holds without loss: shallow ramps and three odd pixels.  At 8 x 8
    that budget is 69 bytes and Oklab's 12-bit L spends them fast: mid grey with one pixel a step brighter (43 bytes)."""
    if w * h <= 64:
        px = np.full((h, w, 3), 99, np.uint8)
        px[3, 4] = (100, 99, 99)
        return px
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.stack([120 + (xx * 6) // w + (yy * 3) // h, 130 - (xx * 4) // w, 125 + (yy * 5) // h], 2)
    for _ in range(3):
        px[rng.integers(0, h), rng.integers(0, w)] += rng.integers(-6, 7, 3)
    return np.ascontiguousarray(px.astype(np.uint8))


@pytest.mark.parametrize("device", [False, True])
def test_image_save(L, device, tmp_path):
    import oracle_lib as O
    from gamut_amd import image as gi
    for k, (w, h) in enumerate(((8, 8), (47, 32), (200, 120), (47, 32))):
        px = calm(w, h, 700 + k) if k < 3 else sqz_cases.picture(w, h, 3, 700 + k)     # the last one: noise, no budget holds it
        host = gi.Image()
        assert host.createView(px, w, h, O.PT["rgb8"], 3 * w)
        im = host
        if device:                                                          # through a lossless file into device storage
            im = gi.Image(device=True)
            assert im.loadFromMemory(host.save_to_memory(gi.FORMAT_QOI)) and im.type == O.PT["rgb8"]
            assert np.array_equal(np.asarray(im.pixels()).reshape(h, w, 3), px)
        assert im.isDevice == device
        for flags in (0, gi.ENCODE_SQZ_QUALITY_BPP1_0, gi.ENCODE_SQZ_QUALITY_MAX):
            budget = L.gamut_hip_sqz_budget_from_flags(w, h, flags)
            enc = im.save_sqz_to_memory(flags)
            assert enc == R.encode(px, R.OKLAB, 7, R.SNAKE, 1, budget), (w, h, flags)
            if flags == gi.ENCODE_SQZ_QUALITY_MAX and k < 3:
                assert len(enc) < budget                                    # lossless: the file is the bytes used, not the budget
            assert im.isValid and im.errorMessage is None and im.type == O.PT["rgb8"] and im.isDevice == device
            again = gi.Image(device=device)
            assert again.loadFromMemory(enc) and np.array_equal(np.asarray(again.pixels()).reshape(h, w, 3), R.load(enc)[0])
        assert im.save_to_memory(gi.FORMAT_SQZ) is None                     # the generic entry does not dispatch SQZ
        path = tmp_path / ("x%d.sqz" % k)
        assert im.saveSQZToFile(path, gi.ENCODE_SQZ_QUALITY_BPP1_0) and path.read_bytes() == im.save_sqz_to_memory(gi.ENCODE_SQZ_QUALITY_BPP1_0)
        assert not im.saveToFile(gi.FORMAT_SQZ, tmp_path / "no.sqz")


def test_image_save_layers_and_refusals(L):
    import oracle_lib as O
    from gamut_amd import image as gi
    layers = np.stack([sqz_cases.picture(40, 24, 3, 800 + k) for k in range(3)])
    lay = gi.Image()
    assert lay.createLayeredView(layers, 40, 24, 3, O.PT["rgb8"], 120, 120 * 24) and lay.layers == 3
    budget = L.gamut_hip_sqz_budget_from_flags(40, 24, 0)
    assert lay.save_sqz_to_memory() == R.encode(layers[0], R.OKLAB, 7, R.SNAKE, 1, budget)
    assert lay.layer(2).save_sqz_to_memory() == R.encode(layers[2], R.OKLAB, 7, R.SNAKE, 1, budget)
    for tname, w, h, ch in (("rgba8", 16, 16, 4), ("l8", 16, 16, 1), ("rgb8", 7, 8, 3), ("rgb8", 8, 7, 3)):
        px = sqz_cases.picture(w, h, 3, 900)[..., :ch] if ch < 4 else np.dstack([sqz_cases.picture(w, h, 3, 900), np.full((h, w), 255, np.uint8)])
        px = np.ascontiguousarray(px)
        im = gi.Image()
        assert im.createView(px, w, h, O.PT[tname], w * ch)
        assert im.save_sqz_to_memory() is None and im.save_sqz_to_memory(gi.ENCODE_SQZ_QUALITY_MAX) is None
        assert im.isValid and im.errorMessage is None and im.type == O.PT[tname] and (im.width, im.height) == (w, h)
    fresh = gi.Image()                                                      # "Uninitialized image" stays what it is
    msg = fresh.errorMessage
    assert fresh.save_sqz_to_memory() is None and fresh.errorMessage == msg and fresh.isError
