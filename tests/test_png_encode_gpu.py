"""GPU PNG encode (png_encode.hip) through the C ABI.  Every stream is taken apart: the bytes outside the IDAT payload must be what the
serial C restatement (tests/c/png_write_ref.c) writes around a payload of that length, zlib.decompress(payload) must be the
restatement's filtered stream (this checks the zlib header, every DEFLATE block and the Adler-32 at once), the canary bytes around
every stream must be intact and the length must stay inside the bound.  On top: shapes, layouts, block-size edges, match edge cases,
content classes, levels and filters, batch behaviour, the drop-in, round trips through the project's and the oracle's decoders, a
transcode, the Image mirror and the size conditions against zlib on the same filtered bytes."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest
import torch

import gen
import oracle_lib as O
import png_write_ref_c as PW
from gamut_amd import _capi, synth
from gamut_amd import image as gi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64
B = PW.BLOCK


def encode(hip, items):
    """items: dicts with px ((h, w, c) uint8 / uint16, or None for a NULL source) and optionally w / h / comp / is16 (overriding the
    array's), filter, level, extra (pitch - row bytes), neg (rows stored bottom-up, negative pitch), shift (misalignment of the first
    stored row), off (an explicit output offset).  -> (files (bytes or None), rc, statuses)."""
    dev = torch.device("cuda", 0)
    parts, metas, at = [], [], 0
    for it in items:
        px = it.get("px")
        if px is None:
            metas.append((None, 0)); continue
        h = px.shape[0]
        rows = np.ascontiguousarray(px).view(np.uint8).reshape(h, -1)
        rb = rows.shape[1]
        P = rb + it.get("extra", 0)
        shift = it.get("shift", 0)
        store = np.zeros(shift + P * h, np.uint8)
        for y in range(h):
            r = (h - 1 - y) if it.get("neg") else y
            store[shift + r * P: shift + r * P + rb] = rows[y]
        metas.append((at + shift + ((h - 1) * P if it.get("neg") else 0), -P if it.get("neg") else P))
        parts.append(store)
        at += store.size
        pad = (-at) % 16
        parts.append(np.zeros(pad + 16, np.uint8)); at += pad + 16
    blob = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(16, np.uint8)).to(dev)
    n = len(items)
    N = max(n, 1)
    src = (C.c_void_p * N)(); pitch = (C.c_int64 * N)(); offs = (C.c_int64 * N)(); lens = (C.c_int64 * N)()
    status = (C.c_int * N)(); W = (C.c_int * N)(); H = (C.c_int * N)(); CO = (C.c_int * N)(); S = (C.c_int * N)()
    F = (C.c_int * N)(); LV = (C.c_int * N)()
    total, bounds = GAP, []
    for i, it in enumerate(items):
        px = it.get("px")
        h, w, c = px.shape if px is not None else (1, 1, 3)
        is16 = int(px is not None and px.dtype.itemsize == 2)
        W[i], H[i], CO[i], S[i] = it.get("w", w), it.get("h", h), it.get("comp", c), it.get("is16", is16)
        F[i], LV[i] = it.get("filter", -1), it.get("level", 5)
        src[i] = blob.data_ptr() + metas[i][0] if metas[i][0] is not None else 0
        pitch[i] = metas[i][1]
        b = hip.gamut_hip_png_encode_bound(W[i], H[i], CO[i], S[i])
        bounds.append(b)
        offs[i] = it.get("off", total)
        total += b + GAP
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    farg = None if items and all("filter" not in it for it in items) else F
    larg = None if items and all("level" not in it for it in items) else LV
    rc = hip.gamut_hip_png_encode_batch_device(src, pitch, W, H, CO, S, farg, larg, n, offs, out.data_ptr(), lens, status,
                                               torch.cuda.current_stream().cuda_stream)
    o = out.cpu().numpy()
    keep = np.zeros(total, bool)
    files = []
    for i in range(n):
        assert 0 <= lens[i] <= max(bounds[i], 0), (i, lens[i], bounds[i])
        if lens[i]:
            keep[offs[i]: offs[i] + lens[i]] = True
        files.append(o[offs[i]: offs[i] + lens[i]].tobytes() if lens[i] else None)
    assert (o[~keep] == CANARY).all(), "bytes written outside the streams"
    return files, rc, list(status[:n])


def verify(it, data):
    """one file against the restatement; -> the IDAT payload"""
    px = it["px"]
    h, w, c, is16 = PW.geometry(px)
    payload = PW.split(data)
    assert data == PW.file_around(w, h, c, is16, payload), "container bytes"
    want = PW.filt(px, it.get("filter", -1))
    got = zlib.decompress(payload)
    assert got == want, ("filtered stream", px.shape, px.dtype, {k: v for k, v in it.items() if k != "px"})
    assert len(data) <= PW.bound(w, h, c, is16)
    return payload


def check(hip, items):
    files, rc, st = encode(hip, items)
    assert rc == _capi.OK and st == [0] * len(items), _capi.last_error()
    return [verify(it, f) for it, f in zip(items, files)]


def _rand(rng, h, w, c, dt=np.uint8):
    return rng.integers(0, 256 if dt == np.uint8 else 65536, (h, w, c)).astype(dt)


def _smooth(rng, h, w, c, dt=np.uint8):
    """gradients with a little noise: every filter gets chosen somewhere, matches exist"""
    y, x = np.mgrid[0:h, 0:w]
    top = 255 if dt == np.uint8 else 65535
    chans = [(x * (3 + k) + y * (5 - k)) * (top // 255) // 2 + rng.integers(0, 3, (h, w)) for k in range(c)]
    return (np.stack(chans, -1) % (top + 1)).astype(dt)


def _l8_stream(stream):
    """an l8 image of width len - 1 ... a filtered stream is type bytes + rows; for w x 1 with filter 0 the filtered stream is
    [0] + the row, so a chosen byte string (after its first byte) becomes the compressor's input exactly"""
    row = np.frombuffer(bytes(stream), np.uint8)
    return dict(px=row.reshape(1, -1, 1), filter=0)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

def test_shapes_comps_and_layouts(hip):
    rng = np.random.default_rng(1)
    items = []
    shapes = [(1, 1), (1, 9), (9, 1), (7, 9), (15, 17), (16, 16), (33, 40), (70, 61)]
    for k, (h, w) in enumerate(shapes):
        for c in (1, 2, 3, 4):
            for dt in (np.uint8, np.uint16):
                px = _smooth(rng, h, w, c, dt) if (k + c) % 2 else _rand(rng, h, w, c, dt)
                items.append(dict(px=px, extra=(k * 3 + c) % 7, neg=(k + c) % 3 == 0, shift=(k + c) % 5))
    check(hip, items)


def test_long_thin(hip):
    rng = np.random.default_rng(2)
    check(hip, [dict(px=_smooth(rng, 1, 65535, 3)), dict(px=_rand(rng, 65535, 1, 1)), dict(px=_smooth(rng, 65535, 1, 2, np.uint16), neg=True),
                dict(px=_smooth(rng, 2, 65535, 4, np.uint16))])


# ---- block and match edges --------------------------------------------------------------------------------------------------------

def test_filtered_lengths_around_the_block_size(hip):
    rng = np.random.default_rng(3)
    items = []
    for L in (1 + 1, 2 + 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 5 * B - 1, 5 * B, 5 * B + 1):
        w = L - 1                                                    # one l8 row: filtered length w + 1
        for kind in range(3):
            row = (rng.integers(0, 256, w) if kind == 0 else np.arange(w) // 7 % 256 if kind == 1 else rng.integers(0, 4, w) * 60)
            items.append(dict(px=row.astype(np.uint8).reshape(1, w, 1)))
    items.append(dict(px=np.zeros((1, 1, 1), np.uint8)))             # one block, two bytes
    check(hip, items)


def test_match_edge_cases(hip):
    rng = np.random.default_rng(4)
    items = []
    # a run that crosses a block boundary (distance 1) and a repeat at the row distance across it
    s = rng.integers(0, 256, 3 * B, dtype=np.uint8)
    s[B - 300: B + 300] = 77
    items.append(_l8_stream(s[1:]))
    # rows of width 32767: the row above is at distance exactly 32768, the far edge of the window
    r = rng.integers(0, 256, 32767, dtype=np.uint8)
    items.append(dict(px=np.stack([r, r, r ^ 1]).reshape(3, 32767, 1), filter=0))
    # rows of width 32768: distance 32769 is outside the window and must not be used
    r = rng.integers(0, 256, 32768, dtype=np.uint8)
    items.append(dict(px=np.stack([r, r]).reshape(2, 32768, 1), filter=0))
    # a match of 258 followed by one of 3, then noise; and every run length around 258 / 259 / 260 / 261
    for run in (3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 519):
        s = rng.integers(0, 256, 2000, dtype=np.uint8)
        s[100: 100 + run + 1] = 9                                    # 1 literal + a run of `run` at distance 1
        items.append(_l8_stream(s[1:]))
    # rgba rows repeating exactly: distance = stride
    px = np.tile(rng.integers(0, 256, (1, 300, 4), dtype=np.uint8), (40, 1, 1))
    items.append(dict(px=px, filter=0))
    payloads = check(hip, items)
    assert len(payloads[-1]) < px.size // 20                         # the repeats were found


# ---- content, levels, filters -------------------------------------------------------------------------------------------------------

def _contents(rng):
    h, w = 144, 192
    y, x = np.mgrid[0:h, 0:w]
    photo = synth.photo_rgb(w, h, 3)
    return {
        "noise": _rand(rng, h, w, 3),
        "flat": np.full((h, w, 4), 200, np.uint8),
        "gradient": np.stack([x * 2 % 256, y * 2 % 256, (x + y) % 256], -1).astype(np.uint8),
        "photo": np.ascontiguousarray(photo.reshape(h, w, 3)),
        "checker": (((x + y) % 2) * 255).astype(np.uint8)[:, :, None].repeat(3, 2),
        "ff16": np.full((h, w, 3), 0xFFFF, np.uint16),
        "grad16": _smooth(rng, h, w, 2, np.uint16),
    }


def test_content_classes_levels_and_filters(hip):
    rng = np.random.default_rng(5)
    for name, px in _contents(rng).items():
        items = [dict(px=px, level=lv) for lv in range(11)] + [dict(px=px, filter=f) for f in (-1, 0, 1, 2, 3, 4, 5, 9, -3)]
        payloads = check(hip, items)
        stored = len(payloads[0])
        L = len(PW.filt(px))
        assert stored == 6 + L + 5 * (-(-L // B)), name                # level 0: stored blocks only
        for lv in range(1, 11):
            assert len(payloads[lv]) <= stored, (name, lv)
        assert all(p[2:] == payloads[1][2:] for p in payloads[1:11]), name     # one effort behind levels 1..10 (the FLG byte differs)
        if name == "noise":
            assert len(payloads[5]) <= stored
        if name in ("flat", "checker", "ff16"):
            assert len(payloads[5]) < L // 50, (name, len(payloads[5]), L)


def test_large_frames(hip):
    rng = np.random.default_rng(6)
    px = np.ascontiguousarray(synth.photo_rgb(1920, 1080, 3).reshape(1080, 1920, 3))
    check(hip, [dict(px=px)])
    y, x = np.mgrid[0:4096, 0:4096]
    big = np.stack([(x + y) % 256, (x * 3) % 256, (y * 5) % 256, (x ^ y) % 256], -1).astype(np.uint8)
    check(hip, [dict(px=big)])


# ---- sizes against zlib on the same filtered bytes ------------------------------------------------------------------------------------

def _huffman_only(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    return co.compress(data) + co.flush()


def test_size_conditions(hip):
    rng = np.random.default_rng(7)
    flat = np.full((1080, 1920, 4), 123, np.uint8)
    (p,) = check(hip, [dict(px=flat, filter=1)])
    L = (1920 * 4 + 1) * 1080
    print("flat 1080p rgba8 filter 1: payload", len(p), "of", L)
    assert len(p) <= L // 100
    noise = _rand(rng, 256, 256, 4)
    p0, p5 = check(hip, [dict(px=noise, level=0), dict(px=noise)])
    print("noise: level 0", len(p0), "default", len(p5))
    assert len(p5) <= len(p0)


# The excess of the default-level payload over zlib.compress(filt, 1), by case, as measured (the encoder is deterministic; the figures
# were taken by executing the kernels' source, payload 3 763 766 / 3 601 596 / 1 121 216 bytes against zlib level 1's 3 418 395 /
# 3 273 504 / 1 121 110).  The guard allows two percentage points more: a different numpy may draw the synthetic image slightly
# differently.  zlib's Z_HUFFMAN_ONLY stream on the same bytes: 3 714 418 / 3 550 742 / 1 085 489 -- on the photo-like image the
# payload is 1.3-1.4 % ABOVE it (DESIGN.md 4.12 says why).
MEASURED_EXCESS = {"photo_f1": 0.1010, "photo_sel": 0.1002, "grad16_sel": 0.0001}


def test_size_against_zlib_level_1(hip):
    rng = np.random.default_rng(8)
    photo = np.ascontiguousarray(synth.photo_rgb(1920, 1080, 3).reshape(1080, 1920, 3))
    cases = {"photo_f1": dict(px=photo, filter=1), "photo_sel": dict(px=photo), "grad16_sel": dict(px=_smooth(rng, 540, 960, 3, np.uint16))}
    for name, it in cases.items():
        (p,) = check(hip, [it])
        f = PW.filt(it["px"], it.get("filter", -1))
        z1, zh = len(zlib.compress(f, 1)), len(_huffman_only(f))
        print(f"{name}: filtered {len(f)} payload {len(p)} zlib-1 {z1} huffman-only {zh} ratio-z1 {len(p) / z1:.4f} ratio-huff {len(p) / zh:.4f}")
        assert MEASURED_EXCESS[name] is not None, "no measured excess recorded"
        assert len(p) <= z1 * (1 + MEASURED_EXCESS[name] + 0.02), (name, len(p), z1)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------

def test_mixed_batch_with_invalid_entries(hip):
    rng = np.random.default_rng(9)
    good = [dict(px=_smooth(rng, 20 + k, 31 - k, 1 + k % 4, np.uint16 if k % 2 else np.uint8), level=k % 11, filter=k % 6 - 1) for k in range(8)]
    bad = [dict(px=None, level=5, filter=-1), dict(px=_rand(rng, 4, 4, 3), comp=5), dict(px=_rand(rng, 4, 4, 3), comp=0),
           dict(px=_rand(rng, 4, 4, 3), w=0), dict(px=_rand(rng, 4, 4, 3), h=-2), dict(px=_rand(rng, 4, 4, 3), level=11),
           dict(px=_rand(rng, 4, 4, 3), level=-1), dict(px=_rand(rng, 4, 4, 3), off=-8),
           dict(px=_rand(rng, 4, 4, 4), w=1 << 20, h=1 << 10, is16=1)]
    items = [good[0], bad[0], good[1], bad[1], bad[2], good[2], good[3], bad[3], bad[4], good[4], bad[5], bad[6], good[5], bad[7], good[6],
             bad[8], good[7]]
    runs = [encode(hip, items) for _ in range(2)]
    assert runs[0] == runs[1]                                        # deterministic
    files, rc, st = runs[0]
    assert rc == _capi.ERR_INVALID_ARG and b"image 1:" in hip.gamut_hip_last_error()
    for it, f, s in zip(items, files, st):
        if any(it is b_ for b_ in bad):
            assert f is None and s == _capi.ERR_INVALID_ARG
        else:
            assert s == _capi.OK
            verify(it, f)
    files, rc, st = encode(hip, [bad[5], good[0]])
    assert rc == _capi.ERR_INVALID_ARG and st == [_capi.ERR_INVALID_ARG, _capi.OK] and files[0] is None
    verify(good[0], files[1])


def test_empty_batch_and_null_arrays(hip):
    assert hip.gamut_hip_png_encode_batch_device(None, None, None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK
    rng = np.random.default_rng(10)
    px = _smooth(rng, 40, 50, 3)
    (a,), rc, st = encode(hip, [dict(px=px)])                        # NULL force_filter / level arrays: -1 and 5
    (b,), _, _ = encode(hip, [dict(px=px, filter=-1, level=5)])
    assert rc == _capi.OK and a == b
    verify(dict(px=px), a)


def test_drop_in_equals_batch(hip):
    rng = np.random.default_rng(11)
    for px, ff, lv, neg in ((_smooth(rng, 37, 45, 3), -1, 5, False), (_smooth(rng, 20, 33, 4, np.uint16), 4, 8, True),
                            (_rand(rng, 9, 9, 1), 2, 0, False), (_smooth(rng, 64, 64, 2), 7, 1, True)):
        h, w, c, is16 = PW.geometry(px)
        rows = np.ascontiguousarray(px).view(np.uint8).reshape(h, -1)
        rb = rows.shape[1]
        stride = rb + 5
        store = np.zeros(stride * h, np.uint8)
        for y in range(h):
            r = h - 1 - y if neg else y
            store[r * stride: r * stride + rb] = rows[y]
        n = C.c_int(0)
        first = store.ctypes.data + ((h - 1) * stride if neg else 0)
        p = hip.gamut_hip_png_write_to_mem(first, -stride if neg else stride, w, h, c, C.byref(n), is16, ff, lv)
        assert p, _capi.last_error()
        got = C.string_at(p, n.value)
        gi.lib().gamut_free_encoded_image(p)
        (want,), rc, _ = encode(hip, [dict(px=px, filter=ff, level=lv)])
        assert rc == _capi.OK and got == want
        verify(dict(px=px, filter=ff), got)
    n = C.c_int(-1)
    assert not hip.gamut_hip_png_write_to_mem(store.ctypes.data, 8, 2, 2, 3, C.byref(n), 0, -1, 11) and n.value == -1
    assert not hip.gamut_hip_png_write_to_mem(None, 8, 2, 2, 3, C.byref(n), 0, -1, 5)


# ---- round trips ------------------------------------------------------------------------------------------------------------------------

def _decode_png_batch(hip, files, bits):
    dev = torch.device("cuda", 0)
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    data = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
    infos = (_capi.PngInfo * n)(); status = (C.c_int * n)(); offs = (C.c_int64 * n)()
    total = 0
    sizes = []
    for i, b in enumerate(bufs):
        info = _capi.PngInfo()
        _capi.check(hip.gamut_hip_png_read_header(b.ctypes.data, b.size, C.byref(info)))
        sz = info.width * info.height * info.channels_in_file * (bits // 8)
        offs[i] = total; sizes.append(sz); total += (sz + 63) & ~63
    out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    _capi.check(hip.gamut_hip_png_decode_batch_device(data, lens, n, 0, bits, offs, out.data_ptr(), infos, status, 0,
                                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [o[offs[i]: offs[i] + sizes[i]] for i in range(n)], infos


def test_round_trips(hip):
    rng = np.random.default_rng(12)
    items = []
    for c in (1, 2, 3, 4):
        for dt in (np.uint8, np.uint16):
            items.append(dict(px=_smooth(rng, 41, 53, c, dt), filter=(c + dt().itemsize) % 6 - 1))
    files, rc, _ = encode(hip, items)
    assert rc == _capi.OK
    for it, f in zip(items, files):
        px = it["px"]
        sixteen = px.dtype == np.uint16
        got, n = O.stbi_load(f, 0, sixteen)                           # the oracle's decoder
        assert n == px.shape[2] and np.array_equal(got, px)
    for bits, dt in ((8, np.uint8), (16, np.uint16)):                 # the project's PNG decoder, as in the file
        sel = [(it, f) for it, f in zip(items, files) if it["px"].dtype == dt]
        outs, infos = _decode_png_batch(hip, [f for _, f in sel], bits)
        for (it, _), o, info in zip(sel, outs, infos):
            assert (info.width, info.height, info.channels, info.bits) == (53, 41, it["px"].shape[2], bits)
            assert np.array_equal(o.view(dt).reshape(it["px"].shape), it["px"])
    # the any-format entry: rgba8
    sel = [(it, f) for it, f in zip(items, files) if it["px"].dtype == np.uint8 and it["px"].shape[2] == 4]
    for it, f in sel:
        buf = np.frombuffer(f, np.uint8)
        data = (C.c_void_p * 1)(buf.ctypes.data); lens = (C.c_size_t * 1)(buf.size); offs = (C.c_int64 * 1)(0)
        info = (_capi.ImageInfo * 1)(); st = (C.c_int * 1)()
        out = torch.zeros(41 * 53 * 4, dtype=torch.uint8, device="cuda")
        _capi.check(hip.gamut_hip_decode_batch_device(data, lens, 1, 4, offs, out.data_ptr(), info, st, None))
        assert info[0].format == 1 and np.array_equal(out.cpu().numpy().reshape(41, 53, 4), it["px"])
    from PIL import Image
    for it, f in zip(items, files):
        im = Image.open(io.BytesIO(f)); im.load()
        assert im.size == (53, 41)


def test_transcode_from_jpeg_and_qoi(hip):
    """JPEG / QOI files -> decoded rgba8 in HBM -> PNG from those pixels, never leaving the device in between"""
    import jpeg_write_ref_c as JW
    rng = np.random.default_rng(13)
    base = _smooth(rng, 48, 64, 3)
    jpg = JW.encode(base, 90)
    img = gi.Image()
    assert img.createView(np.ascontiguousarray(np.dstack([base, np.full((48, 64), 255, np.uint8)])), 64, 48, 12, 64 * 4)
    qoi = None
    for f in (jpg, "qoi"):
        if f == "qoi":
            f = img.save_to_memory(gi.FORMAT_QOI)
            assert f
        buf = np.frombuffer(f, np.uint8)
        data = (C.c_void_p * 1)(buf.ctypes.data); lens = (C.c_size_t * 1)(buf.size); offs = (C.c_int64 * 1)(0)
        info = (_capi.ImageInfo * 1)(); st = (C.c_int * 1)()
        dec = torch.zeros(48 * 64 * 4, dtype=torch.uint8, device="cuda")
        _capi.check(hip.gamut_hip_decode_batch_device(data, lens, 1, 4, offs, dec.data_ptr(), info, st, None))
        src = (C.c_void_p * 1)(dec.data_ptr()); pitch = (C.c_int64 * 1)(64 * 4); W = (C.c_int * 1)(64); H = (C.c_int * 1)(48)
        CO = (C.c_int * 1)(4); S = (C.c_int * 1)(0); ln = (C.c_int64 * 1)(); ooff = (C.c_int64 * 1)(0)
        out = torch.zeros(hip.gamut_hip_png_encode_bound(64, 48, 4, 0), dtype=torch.uint8, device="cuda")
        _capi.check(hip.gamut_hip_png_encode_batch_device(src, pitch, W, H, CO, S, None, None, 1, ooff, out.data_ptr(), ln, None, None))
        png = out.cpu().numpy()[:ln[0]].tobytes()
        px = dec.cpu().numpy().reshape(48, 64, 4)
        verify(dict(px=px), png)
        got, n = O.stbi_load(png, 0)
        assert n == 4 and np.array_equal(got, px)


# ---- the Image mirror ------------------------------------------------------------------------------------------------------------------

TYPES = {(1, 1): 0, (1, 2): 1, (2, 1): 3, (2, 2): 4, (3, 1): 9, (3, 2): 10, (4, 1): 12, (4, 2): 13}     # (channels, bytes) -> PixelType


def _filter_types(png, px):
    h, w, c, is16 = PW.geometry(px)
    f = zlib.decompress(PW.split(png))
    return f[::w * c * (2 if is16 else 1) + 1]


def test_image_mirror(hip, tmp_path):
    rng = np.random.default_rng(14)
    for c in (1, 2, 3, 4):
        for dt in (np.uint8, np.uint16):
            px = _smooth(rng, 30, 44, c, dt)
            rows = np.ascontiguousarray(px).view(np.uint8).reshape(30, -1)
            host = gi.Image()
            assert host.createView(rows, 44, 30, TYPES[(c, px.dtype.itemsize)], rows.shape[1])
            png = host.save_png_to_memory()
            assert png is not None and host.isValid
            verify(dict(px=px), png)
            dev = gi.Image(device=True)
            assert dev.loadFromMemory(png) and dev.isDevice and dev.type == TYPES[(c, px.dtype.itemsize)]
            assert dev.save_png_to_memory() == png                     # straight from HBM: the same bytes
            # flipped: negative pitch passed through, rows come out in logical order
            assert host.flipVertical() and host.pitchInBytes < 0
            verify(dict(px=px[::-1]), host.save_png_to_memory())
            assert dev.flipVertical()
            verify(dict(px=px[::-1]), dev.save_png_to_memory())
    # flags
    px = _smooth(rng, 50, 70, 3)
    rows = px.reshape(50, -1)
    img = gi.Image()
    assert img.createView(rows, 70, 50, 9, rows.shape[1])
    fast = img.save_png_to_memory(gi.ENCODE_PNG_FILTER_FAST)
    verify(dict(px=px, filter=0), fast)
    assert set(_filter_types(fast, px)) == {0}
    stored = img.save_png_to_memory(gi.ENCODE_PNG_COMPRESSION_0)
    verify(dict(px=px), stored)
    L = (70 * 3 + 1) * 50
    assert len(stored) == 57 + 6 + L + 5 * (-(-L // B))
    assert img.save_png_to_memory(gi.ENCODE_PNG_COMPRESSION_10 | gi.ENCODE_PNG_FILTER_FAST) is not None
    for lv in (12, 13, 14, 15):
        assert img.save_png_to_memory(lv) is None and img.save_png_to_memory(lv | 16) is None
        assert img.isValid and img.errorMessage is None
    path = tmp_path / "out.png"
    assert img.savePNGToFile(path) and path.read_bytes() == img.save_png_to_memory()
    assert not img.savePNGToFile(tmp_path / "none" / "out.png")
    # refused types: fp32 and premultiplied
    for type_, bpp in ((2, 4), (11, 12), (14, 16), (15, 4), (6, 2), (16, 8)):
        bad = gi.Image()
        assert bad.createView(np.zeros((3, 3 * bpp), np.uint8), 3, 3, type_, 3 * bpp)
        assert bad.save_png_to_memory() is None and bad.isValid
    # layer 0 of a layered image; rgb16 after convertTo16Bit on the device
    lay = gi.Image(device=True)
    assert lay.createLayered(20, 10, 3, 12)
    verify(dict(px=lay.pixels(0).reshape(10, 20, 4)), lay.save_png_to_memory())
    d16 = gi.Image(device=True)
    assert d16.loadFromMemory(fast) and d16.convertTo16Bit() and d16.type == 10
    want = d16.pixels().view(np.uint16).reshape(50, 70, 3)
    assert np.array_equal(want, px.astype(np.uint16) * 257)
    verify(dict(px=want), d16.save_png_to_memory())
    # the generic entry does not dispatch PNG yet
    assert img.save_to_memory(gi.FORMAT_PNG) is None
