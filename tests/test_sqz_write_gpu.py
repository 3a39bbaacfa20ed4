"""The SQZ device writer, byte for byte: files left in HBM by gamut_hip_sqz_encode_batch_to_device against the C restatement's encoder
(tests/c/sqz_ref.c), constructed coefficient buffers through gamut_hip_sqz_write_batch_device against the unchanged host writer
gamut_hip_sqz_encode_coeffs (and the Python restatement where the case is small), the round trip, and the writer switch.  Every output
allocation carries guards (0xA5 fill, odd offsets) and is compared whole."""
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
GUARD = 512
_files = {}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def planes_of(mode):
    return 1 if mode == 0 else 3


def lossless_budget(px):
    return 64 + px.size * 3


def ref_file(px, mode, levels, scan, ss, budget):
    """tests/c/sqz_ref.c's file, computed once per case and shared"""
    key = (px.tobytes(), px.shape, mode, levels, scan, ss, budget)
    if key not in _files:
        _files[key] = R.encode(px, mode, levels, scan, ss, budget)
    return _files[key]


def fill_descs(items):
    descs = (_capi.SqzEncodeDesc * len(items))()
    for k, it in enumerate(items):
        descs[k].width, descs[k].height, descs[k].color_mode, descs[k].levels = it["w"], it["h"], it["mode"], it["levels"]
        descs[k].scan_order, descs[k].subsampling, descs[k].budget = it.get("scan", 0), it.get("ss", 0), it["budget"]
    return descs


def upload(items):
    """the pictures in ONE device buffer: tight, padded ("pad"), bottom-up ("neg") or at an odd address ("odd"); "null": no source"""
    blobs, where, pos = [], [], 0
    for it in items:
        px, kind = it["px"], it.get("src", "tight")
        if kind == "null":
            where.append(None)
            continue
        h = px.shape[0]
        row = px.size // h
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


def out_layout(items):
    offs, pos = [], GUARD
    for k, it in enumerate(items):
        pos += 1 + 2 * (k % 8)                                              # odd offsets
        offs.append(it.get("offset", pos))
        pos += max(int(it["budget"]), 0) + GUARD
    return offs, pos


def check_call(L, items, want, call, stream=None):
    """`call(descs, n, offs, out_ptr, lens, st, stream)` is one batch call with `out` in DEVICE memory; want[k] is the file, or a status"""
    n = len(items)
    offs, total = out_layout(items)
    expect = np.full(total, 0xA5, np.uint8)
    for f, o in zip(want, offs):
        if not isinstance(f, int):
            expect[o:o + len(f)] = np.frombuffer(f, np.uint8)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = (C.c_int64 * n)(*([-1] * n))
    st = (C.c_int * n)(*([77] * n))
    torch.cuda.synchronize()
    rc = call(fill_descs(items), n, (C.c_int64 * n)(*offs), out.data_ptr(), lens, st, stream)
    got = out.cpu().numpy()                                                 # no synchronize: the call returns when the files are in place
    status = [f if isinstance(f, int) else 0 for f in want]
    bad = [i for i, s in enumerate(status) if s]
    assert rc == (status[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    assert list(st) == status
    for k in range(n):
        it = items[k]
        assert lens[k] == (0 if status[k] else len(want[k])), (k, it["w"], it["h"], it["mode"], it["levels"], it.get("scan"), it["budget"], lens[k])
    if not np.array_equal(got, expect):
        first = int(np.flatnonzero(got != expect)[0])
        k = max([i for i in range(n) if offs[i] - GUARD <= first], default=0)
        it = items[k]
        assert False, ("image", k, it["w"], it["h"], it["mode"], it["levels"], it.get("scan"), it.get("ss"), it["budget"], "byte", first - offs[k],
                       "got", got[first:first + 8].tolist(), "want", expect[first:first + 8].tolist())
    return want


def to_device(L, items, stream=None):
    """one gamut_hip_sqz_encode_batch_to_device call on pictures; an item with "want" is refused with that status"""
    for it in items:
        it.setdefault("h", it["px"].shape[0]); it.setdefault("w", it["px"].shape[1])
    want = [it["want"] if "want" in it else ref_file(it["px"], it["mode"], it["levels"], it["scan"], it["ss"], it["budget"]) for it in items]
    dev, ptrs, pitches = upload(items)
    return check_call(L, items, want, lambda d, n, offs, out, lens, st, s: L.gamut_hip_sqz_encode_batch_to_device(ptrs, pitches, d, n, offs, out, lens, st, s), stream)


def host_writer(L, it):
    """the unchanged host writer on a coefficient buffer -> the file, or its status"""
    co = np.ascontiguousarray(it["co"], np.int16).reshape(-1)
    d = fill_descs([it])
    dst = np.zeros(it["budget"] + 8, np.uint8)
    n = C.c_int64(0)
    rc = L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, d, dst.ctypes.data, C.byref(n))
    return rc if rc else dst[:n.value].tobytes()


def python_writer(it):
    try:
        f = P.encode_coeffs(it["co"], it["w"], it["h"], it["mode"], it["levels"], it.get("scan", 0), it.get("ss", 0), it["budget"])
    except P.Undefined:
        return _capi.ERR_INVALID_ARG
    return f


def write_coeffs(L, items, python=False, dwt_from=None):
    """one gamut_hip_sqz_write_batch_device call on coefficient buffers at odd element offsets of one device buffer.  dwt_from: the
    int16 planes the buffers are made of ON THE DEVICE by gamut_hip_sqz_dwt_batch_device (it["co"] is then the C restatement's result)."""
    n = len(items)
    want = [host_writer(L, it) for it in items]
    if python:
        for it, f in zip(items, want):
            assert python_writer(it) == f, (it["w"], it["h"], it["budget"])
    coffs, pos = [], 7
    for it in items:
        coffs.append(pos)
        pos += it["co"].size + 9
    host = np.full(pos, 0x5A5A, np.uint16).view(np.int16)
    for k, (it, o) in enumerate(zip(items, coffs)):
        host[o:o + it["co"].size] = (it["co"] if dwt_from is None else dwt_from[k]).reshape(-1)
    dco = torch.from_numpy(host.copy()).cuda()
    c_offs = (C.c_int64 * n)(*coffs)
    if dwt_from is not None:
        src, dco = dco, torch.full_like(dco, 0x5A5A)
        st = (C.c_int * n)()
        assert L.gamut_hip_sqz_dwt_batch_device(src.data_ptr(), fill_descs(items), n, dco.data_ptr(), c_offs, st, None) == 0
        torch.cuda.synchronize()
        for it, o in zip(items, coffs):
            assert np.array_equal(dco[o:o + it["co"].size].cpu().numpy(), it["co"].reshape(-1))
    before = dco.clone()
    check_call(L, items, want, lambda d, k, offs, out, lens, st, s: L.gamut_hip_sqz_write_batch_device(dco.data_ptr(), c_offs, d, k, offs, out, lens, st, s))
    assert torch.equal(dco, before)                                         # the coefficients are only read
    return want


def matrix_items():
    items = []
    for mode in range(4):
        px = sqz_cases.picture(16, 16, planes_of(mode), 40 + mode)
        for scan in range(4):
            for ss in (0, 1):
                for b in (7, 8, 9, 16, 40, 100, 300, 1000, lossless_budget(px)):
                    items.append(dict(px=px, mode=mode, levels=1, scan=scan, ss=ss, budget=b))
    for k, (w, h) in enumerate(((17, 16), (19, 23), (32, 33), (47, 32), (64, 40), (128, 72))):
        for lv in range(1, 5):
            mode = (k + lv) % 4
            px = sqz_cases.picture(w, h, planes_of(mode), 200 + k)
            for b in (100, 1000, lossless_budget(px)):
                items.append(dict(px=px, mode=mode, levels=lv, scan=(k + lv + mode) % 4, ss=(k + lv) & 1, budget=b, src=("pad", "neg", "odd")[(k + lv) % 3]))
    for mode in (0, 2):                                                     # 8 x 8 at one level: bands of 16 coefficients, fewer than a wave
        px = sqz_cases.picture(8, 8, planes_of(mode), 77 + mode)
        for scan in range(4):
            for b in (7, 20, lossless_budget(px)):
                items.append(dict(px=px, mode=mode, levels=1, scan=scan, ss=scan & 1, budget=b))
    return items


def test_mode_scan_budget_matrix_and_the_way_back(L):
    items = matrix_items()
    files = to_device(L, items)
    files = files[5::23] + files[-30::7]                                    # a share of them through the GPU decoder
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


def test_every_budget_of_one_file(L):
    """16 x 17 Oklab, snake, subsampled: every byte budget from 7 to the lossless length in one call, each the prefix of the lossless
    file -- cuts inside sorting passes, inside refinement passes, inside run codes and between segments"""
    px = sqz_cases.picture(16, 17, 3, 32)
    full = sqz_cases.prefix_files()[1]
    files = to_device(L, [dict(px=px, mode=2, levels=1, scan=R.SNAKE, ss=1, budget=b) for b in range(7, len(full) + 1)])
    assert files[-1] == full and all(f == full[:7 + k] for k, f in enumerate(files))


@pytest.mark.parametrize("scan", range(4))
def test_chunk_boundaries(L, scan):
    """grey one-level images whose largest band (the LL band, ceil(w / 2) x ceil(h / 2)) holds C - 1, C, C + 1 and 2 C + 1 coefficients,
    C the coefficients a wave takes per step; random full-range planes, transformed on the device"""
    c = L.gamut_hip_sqz_write_chunk()
    rng = np.random.default_rng(50 + scan)
    items, planes = [], []
    for target in (c - 1, c, c + 1, 2 * c + 1):
        a = next(a for a in range(int(target ** 0.5), 3, -1) if target % a == 0)      # the factor pair nearest a square, both at least 4
        bw, bh = target // a, a
        w, h = 2 * bw - (target & 1), 2 * bh
        assert ((w + 1) // 2) * ((h + 1) // 2) == target and min(w, h) >= 8
        p = rng.integers(-32768, 32768, (1, h, w)).astype(np.int16)
        co = F.forward(p, w, h, 1)
        for budget in (target // 3, 64 + 6 * w * h):
            items.append(dict(co=co, w=w, h=h, mode=0, levels=1, scan=scan, ss=0, budget=budget))
            planes.append(p)
    write_coeffs(L, items, python=False, dwt_from=planes)


def band_view(a, o):
    """orientation o of a one-level coefficient plane (subbands interleaved in place): even / odd rows, left / right half"""
    return a[(o > 1)::2, (a.shape[1] // 2 if o & 1 else 0):(a.shape[1] if o & 1 else a.shape[1] // 2)]


def test_constructed_coefficient_buffers(L):
    rng = np.random.default_rng(8)
    items = []

    def add(a, scans=(0, 1, 2, 3)):
        h, w = a.shape
        for scan in scans:
            for budget in (64 + 6 * w * h, 7 + (w * h) // 5):
                items.append(dict(co=a.astype(np.uint16).view(np.int16).copy(), w=w, h=h, mode=0, levels=1, scan=scan, ss=0, budget=budget))

    add(np.zeros((32, 32), np.uint16))                                      # every max_bitplane is 0: header nibbles alone
    a = np.zeros((32, 32), np.uint16); band_view(a, 2)[5, 7] = 1 << 14; add(a)          # one value on plane 14 and nothing else
    a = np.zeros((32, 32), np.uint16); band_view(a, 2)[5, 7] = (1 << 14) | 1; add(a, (1,))
    a = rng.integers(0, 8, (32, 32)).astype(np.uint16)                      # bit 15 beside smaller values: the blind top bit
    band_view(a, 1)[...] = 0x8000 | rng.integers(0, 0x8000, (16, 16)); band_view(a, 1)[3, 3] = 6
    band_view(a, 3)[...] = 0x8000 | rng.integers(0, 64, (16, 16)); band_view(a, 3)[15, 15] = 0x0155; band_view(a, 3)[0, 0] = 0xFFFF
    add(a)
    a = np.zeros((32, 32), np.uint16)                                       # a band where every class 1..14 occurs (and class 0)
    band_view(a, 0)[...] = ((1 << rng.integers(0, 15, (16, 16))) | rng.integers(0, 1 << 14, (16, 16))) & ((2 << rng.integers(0, 15, (16, 16))) - 1)
    band_view(a, 0)[0, :15] = [1 << k for k in range(15)]
    band_view(a, 3)[...] = band_view(a, 0)[::-1]
    add(a)
    for count in (64, 65):                                                  # a class that occurs exactly 64 and 65 times
        a = rng.integers(0, 16, (32, 32)).astype(np.uint16)
        for o, cls in ((0, 9), (1, 4), (2, 7)):
            v = band_view(a, o).reshape(-1).copy()
            at = rng.permutation(256)[:count]
            v[at] = (1 << cls) | rng.integers(0, 1 << cls, count)
            band_view(a, o)[...] = v.reshape(16, 16)
        band_view(a, 3).reshape(16, 16)[...] = np.where(np.arange(256).reshape(16, 16) < count, 0x0400 | 1, 2)      # 64 / 65 in a row, then the rest
        add(a)
    a = rng.integers(0, 1 << 10, (32, 32)).astype(np.uint16)
    add(a | 1, (0, 3)); add(a & ~np.uint16(1), (0, 3))                      # signs all set, all clear
    want = write_coeffs(L, items, python=True)
    assert all(not isinstance(f, int) for f in want)


def test_long_runs(L):
    """1024 x 512 grey, one level, raster: bands of 512 x 256 = 131072 coefficients, nearly empty.  LL: runs of 65535 and 65536; HL: a
    run of 131071; LH: a run of 131072 = 2^17, the first the reference writes in two parts (34 bits) -- and on the plane below it a
    termination run of 131072, the longest a band of this size has (a band's maximum is on its top plane, so a pass that emits nothing
    runs over at most n - 1 elements, and 131073 cannot occur); HH: one value at the front, termination runs of 131072 on every plane.  Every budget from 7 to the
    lossless length: the cuts fall inside the two-part code among everything else."""
    w, h = 1024, 512
    a = np.zeros((h, w), np.uint16)
    ll, hl, lh, hh = (band_view(a, o) for o in range(4))
    for band, at, v in ((ll, 65534, 4), (ll, 131070, 5), (hl, 131070, 4), (lh, 131071, 9), (hh, 0, 12)):
        band[at // 512, at % 512] = v
    co = a.view(np.int16)
    full = host_writer(L, dict(co=co, w=w, h=h, mode=0, levels=1, scan=0, ss=0, budget=4096))
    assert not isinstance(full, int) and 20 < len(full) < 200
    bits = "".join("{:08b}".format(x) for x in full)
    assert "".join("0" + b for b in bin(131072)[3:]) + "1" in bits          # the 34-bit code of 2^17 and what ends it
    items = [dict(co=co, w=w, h=h, mode=0, levels=1, scan=0, ss=0, budget=b) for b in list(range(7, len(full) + 1)) + [4096]]
    files = write_coeffs(L, items)
    assert all(f == full[:it["budget"]] for f, it in zip(files, items))


def test_deviation_1_between_good_neighbours(L):
    """the last band of the finest level holds nothing but negative shorts: with a budget that ends before the schedule reaches that
    band's header nibble the file is an ordinary one, with one byte more the image is refused -- by both writers"""
    w, h, lv = 64, 40, 3
    rng = np.random.default_rng(4)
    co = F.forward(rng.integers(-40, 40, (1, h, w)).astype(np.int16), w, h, lv).reshape(h, w).copy()
    band_view(co, 3)[...] = (0x8000 | rng.integers(0, 0x8000, (h // 2, w // 2))).astype(np.uint16).view(np.int16)
    it = dict(co=co, w=w, h=h, mode=0, levels=lv, scan=1, ss=0)
    budgets = range(7, 64 + 6 * w * h)
    verdict = lambda b: isinstance(host_writer(L, dict(it, budget=b)), int)
    lo, hi = 7, budgets[-1]                                                 # refusal is monotone in the budget: find the first refused one
    assert not verdict(lo) and verdict(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if verdict(mid) else (mid, hi)
    good = dict(co=F.forward(rng.integers(-40, 40, (1, h, w)).astype(np.int16), w, h, lv), w=w, h=h, mode=0, levels=lv, scan=2, ss=0, budget=5000)
    items = [dict(good), dict(it, budget=lo), dict(good, scan=3), dict(it, budget=hi), dict(good, budget=300), dict(it, budget=hi + 1000), dict(good, scan=0)]
    want = write_coeffs(L, items, python=True)
    assert [isinstance(f, int) for f in want] == [False, False, False, True, False, True, False] and want[3] == _capi.ERR_INVALID_ARG
    assert len(want[1]) == lo and b"image 3: sqz: a subband holds nothing but" in L.gamut_hip_last_error()


def test_forty_images_some_of_them_refused(L):
    rng = np.random.default_rng(9)
    items = []
    for k in range(40):
        w, h = int(rng.integers(8, 150)), int(rng.integers(8, 90))
        mode = k % 4
        px = sqz_cases.picture(w, h, planes_of(mode), 600 + k)
        it = dict(px=px, mode=mode, levels=1 + k % 8, scan=(k // 4) % 4, ss=(k // 2) & 1, budget=(50, 400, 3000, lossless_budget(px))[(k // 3) % 4],
                  src=("tight", "pad", "neg", "odd")[(k // 4) % 4])
        if k in (0, 17):
            it["budget"], it["want"] = 6, _capi.ERR_INVALID_ARG
        if k == 13:
            it["mode"], it["want"] = 5, _capi.ERR_INVALID_ARG
        if k == 26:
            it["src"], it["want"] = "null", _capi.ERR_INVALID_ARG
        if k == 33:
            it["offset"], it["want"] = -8, _capi.ERR_INVALID_ARG
        items.append(it)
    assert sum(1 for it in items if "want" in it) == 5 and any(it["levels"] > F.clamp_levels(it["px"].shape[1], it["px"].shape[0], it["levels"]) for it in items)
    to_device(L, items)


def test_stale_scratch_and_a_second_stream(L):
    """a large call, then a small one on the same thread: the small file must not see the large call's bits; then on the caller's stream"""
    big = [dict(px=sqz_cases.picture(128, 72, planes_of(k % 4), 900 + k % 4), mode=k % 4, levels=4, scan=k % 4, ss=k & 1) for k in range(64)]
    for it in big:
        it["budget"] = lossless_budget(it["px"])
    to_device(L, big)
    small = dict(px=sqz_cases.picture(16, 16, 3, 42), mode=2, levels=1, scan=1, ss=1, budget=40)
    to_device(L, [dict(small)])
    s = torch.cuda.Stream()
    to_device(L, [dict(small)], stream=C.c_void_p(s.cuda_stream))
    to_device(L, [dict(small, budget=9)])


def test_the_switch(L):
    """with the device writer selected, the three entries with unchanged signatures give the files they give with the host writer"""
    import oracle_lib as O
    from gamut_amd import image as gi
    items = [dict(px=sqz_cases.picture(47, 32, 3, 7), mode=2, levels=7, scan=1, ss=1, budget=300),
             dict(px=sqz_cases.picture(64, 40, 1, 8), mode=0, levels=3, scan=3, ss=0, budget=lossless_budget(sqz_cases.picture(64, 40, 1, 8))),
             dict(px=sqz_cases.picture(19, 23, 3, 9), mode=1, levels=1, scan=2, ss=1, budget=6)]
    for it in items:
        it["h"], it["w"] = it["px"].shape[:2]
    dev, ptrs, pitches = upload(items)
    px = sqz_cases.picture(200, 120, 3, 704)
    host = gi.Image()
    assert host.createView(px, 200, 120, O.PT["rgb8"], 600)
    on_dev = gi.Image(device=True)
    assert on_dev.loadFromMemory(host.save_to_memory(gi.FORMAT_QOI)) and on_dev.isDevice

    def run():
        n = len(items)
        offs, total = out_layout(items)
        out = np.full(total, 0xA5, np.uint8)
        lens = (C.c_int64 * n)(*([-1] * n)); st = (C.c_int * n)(*([77] * n))
        rc = L.gamut_hip_sqz_encode_batch_device(ptrs, pitches, fill_descs(items), n, (C.c_int64 * n)(*offs), out.ctypes.data, lens, st, None)
        msg = L.gamut_hip_last_error()
        k = C.c_int(0)
        flipped = np.ascontiguousarray(items[0]["px"][::-1])
        p = L.gamut_hip_sqz_write_to_mem(flipped.ctypes.data + 31 * 141, -141, fill_descs(items[:1]), C.byref(k))
        assert p
        mem = C.string_at(p, k.value)
        C.CDLL(None).free(C.c_void_p(p))
        saved = [im.save_sqz_to_memory(f) for im in (host, on_dev) for f in (0, gi.ENCODE_SQZ_QUALITY_BPP1_0, gi.ENCODE_SQZ_QUALITY_MAX)]
        return rc, msg, list(lens), list(st), out.tobytes(), mem, saved

    prev = L.gamut_hip_sqz_set_writer(0)
    try:
        with_host = run()
        assert L.gamut_hip_sqz_set_writer(1) == 0
        with_device = run()
        assert L.gamut_hip_sqz_set_writer(0) == 1
    finally:
        L.gamut_hip_sqz_set_writer(prev)
    assert with_device == with_host
    rc, msg, lens, st, _, mem, saved = with_host
    assert rc == _capi.ERR_INVALID_ARG and msg.startswith(b"image 2:") and st == [0, 0, _capi.ERR_INVALID_ARG] and lens[0] == 300 and lens[2] == 0
    assert mem == ref_file(items[0]["px"], 2, 7, 1, 1, 300)
    for k, flags in enumerate((0, gi.ENCODE_SQZ_QUALITY_BPP1_0, gi.ENCODE_SQZ_QUALITY_MAX)):
        want = R.encode(px, R.OKLAB, 7, R.SNAKE, 1, L.gamut_hip_sqz_budget_from_flags(200, 120, flags))
        assert saved[k] == want == saved[3 + k]
        where = on_dev.save_sqz_to_device(flags)                            # the same bytes, left in HBM and owned by the image
        assert where is not None and where[1] == len(want)
        got = np.zeros(where[1], np.uint8)
        _capi.check(L.gamut_hip_memcpy_d2h(got.ctypes.data, where[0], where[1], None))
        _capi.check(L.gamut_hip_stream_synchronize(None))
        assert got.tobytes() == want
    assert host.save_sqz_to_device() is None and on_dev.isValid and on_dev.type == O.PT["rgb8"]
