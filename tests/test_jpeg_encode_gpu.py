"""GPU JPEG encode (jpeg_encode.hip) through the C ABI: byte-exact against the serial C restatement (tests/c/jpeg_write_ref.c) on edge
shapes, adversarial content and large frames, batch behaviour with invalid entries and canary bytes, the drop-ins, round trips and a
decode -> encode transcode, and the Image mirror."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import gen
import jpeg_write_ref_c as JW
import oracle_lib as O
from gamut_amd import _capi, synth
from gamut_amd import image as gi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64


def encode(hip, items):
    """items: dicts with px ((h, w, c) uint8, or None for a NULL source), and optionally w / h / comp (overriding the array's),
    quality, extra (pitch - row bytes), neg (rows stored bottom-up, negative pitch), shift (misalignment of the first stored row),
    off (an explicit output offset).  -> (streams (bytes or None), rc, statuses).  Every output byte outside the streams must still
    hold the canary."""
    dev = torch.device("cuda", 0)
    parts, metas, at = [], [], 0
    for it in items:
        px = it.get("px")
        if px is None:
            metas.append((None, 0)); continue
        h, w, c = px.shape
        P = w * c + it.get("extra", 0)
        shift = it.get("shift", 0)
        store = np.zeros(shift + P * h, np.uint8)
        for y in range(h):
            r = (h - 1 - y) if it.get("neg") else y
            store[shift + r * P: shift + r * P + w * c] = px[y].reshape(-1)
        metas.append((at + shift + ((h - 1) * P if it.get("neg") else 0), -P if it.get("neg") else P))
        parts.append(store)
        at += store.size
        pad = (-at) % 16
        parts.append(np.zeros(pad + 16, np.uint8)); at += pad + 16
    blob = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(16, np.uint8)).to(dev)
    n = len(items)
    N = max(n, 1)
    src = (C.c_void_p * N)(); pitch = (C.c_int64 * N)(); offs = (C.c_int64 * N)(); lens = (C.c_int64 * N)()
    status = (C.c_int * N)(); W = (C.c_int * N)(); H = (C.c_int * N)(); CO = (C.c_int * N)(); Q = (C.c_int * N)()
    total, bounds = GAP, []
    for i, it in enumerate(items):
        px = it.get("px")
        h, w, c = px.shape if px is not None else (1, 1, 3)
        W[i], H[i], CO[i], Q[i] = it.get("w", w), it.get("h", h), it.get("comp", c), it.get("quality", 90)
        src[i] = blob.data_ptr() + metas[i][0] if metas[i][0] is not None else 0
        pitch[i] = metas[i][1]
        b = hip.gamut_hip_jpeg_encode_bound(W[i], H[i], CO[i], Q[i])
        bounds.append(b)
        offs[i] = it.get("off", total)
        total += b + GAP
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    qarg = None if items and all(it.get("quality") is None for it in items) else Q
    rc = hip.gamut_hip_jpeg_encode_batch_device(src, pitch, W, H, CO, qarg, n, offs, out.data_ptr(), lens, status,
                                                torch.cuda.current_stream().cuda_stream)
    o = out.cpu().numpy()
    keep = np.zeros(total, bool)
    streams = []
    for i in range(n):
        assert 0 <= lens[i] <= max(bounds[i], 0)
        if lens[i]:
            keep[offs[i]: offs[i] + lens[i]] = True
        streams.append(o[offs[i]: offs[i] + lens[i]].tobytes() if lens[i] else None)
    assert (o[~keep] == CANARY).all(), "bytes written outside the streams"
    return streams, rc, list(status[:n])


def check(hip, items):
    streams, rc, st = encode(hip, items)
    assert rc == _capi.OK and st == [0] * len(items), _capi.last_error()
    for it, s in zip(items, streams):
        assert s == JW.encode(it["px"], it.get("quality", 90)), (it["px"].shape, {k: v for k, v in it.items() if k != "px"})
    return streams


def _rand(rng, h, w, c):
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


# ---- shapes -------------------------------------------------------------------------------------------------------------------

def test_shapes_comps_and_layouts(hip):
    rng = np.random.default_rng(1)
    items = []
    shapes = [(1, 1), (1, 9), (9, 1), (7, 9), (15, 17), (16, 16), (17, 15), (33, 40)]
    for k, (h, w) in enumerate(shapes):
        for c in (1, 2, 3, 4):
            for q in (90, 95):
                items.append(dict(px=_rand(rng, h, w, c), quality=q, extra=(k * 3 + c) % 7, neg=(k + c) % 3 == 0, shift=(k + q) % 5))
    check(hip, items)


def test_long_thin(hip):
    rng = np.random.default_rng(2)
    check(hip, [dict(px=_rand(rng, 1, 65535, 3), quality=90), dict(px=_rand(rng, 65535, 1, 1), quality=95),
                dict(px=_rand(rng, 2, 65535, 4), quality=50, neg=True)])


# ---- adversarial content --------------------------------------------------------------------------------------------------------

def test_extremes_at_quality_100(hip):
    """0/255 checkerboards and stripes: the largest categories and the closest approach to the bound"""
    y, x = np.mgrid[0:64, 0:80]
    items = []
    for pat in ((x + y) % 2, x % 2, y % 2, (x // 2 + y // 3) % 2, (x // 8 + y // 8) % 2):
        g = (pat * 255).astype(np.uint8)
        for c in (1, 3):
            px = np.repeat(g[:, :, None], c, 2) if c == 1 else np.stack([g, 255 - g, g], -1)
            items.append(dict(px=px, quality=100))
            items.append(dict(px=px, quality=90))
    streams = check(hip, items)
    assert max(len(s) for s in streams) > 10000


def test_zero_runs_and_isolated_coefficients(hip):
    """blocks whose only content is one DCT basis function: a single coefficient at any zig-zag position (63 included) after runs
    of 16, 32, 48 and more zeros (ZRL)"""
    k = np.arange(8)
    items = []
    for u, v in ((7, 7), (0, 7), (7, 0), (3, 5), (1, 0), (4, 4), (2, 6)):
        basis = np.outer(np.cos((2 * k + 1) * u * np.pi / 16), np.cos((2 * k + 1) * v * np.pi / 16))
        for amp in (30, 90):
            g = np.clip(128 + amp * np.tile(basis, (3, 4)), 0, 255).astype(np.uint8)
            items.append(dict(px=g[:, :, None], quality=100))
            items.append(dict(px=np.stack([g, g, 255 - g], -1), quality=95))
            items.append(dict(px=np.stack([g, g, g], -1), quality=75))
    check(hip, items)


def test_flat_images(hip):
    """EOB-only blocks: many blocks per 32-bit word of the raw stream"""
    items = [dict(px=np.full((h, w, c), v, np.uint8), quality=q) for (h, w) in ((64, 64), (200, 123), (1, 300))
             for c in (1, 3) for v in (0, 128, 255) for q in (10, 90, 100)]
    check(hip, items)


def test_ff_dense_content(hip):
    """content whose stream is dense in 0xFF data bytes, and images whose padded last data byte is 0xFF"""
    rng = np.random.default_rng(5)
    items = []
    for t in range(60):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        items.append(dict(px=_rand(rng, h, w, 3), quality=int(rng.choice([1, 5, 100]))))
    streams = check(hip, items)
    ends_ff = sum(s[-4:-2] == b"\xFF\x00" for s in streams)
    assert ends_ff >= 1, "no stream ended with a stuffed 0xFF data byte: widen the search"
    assert sum(s[607:-2].count(b"\xFF\x00") for s in streams) > 100


# ---- size ----------------------------------------------------------------------------------------------------------------------

def test_1080p_photo_and_4096(hip):
    photo = synth.photo_rgb(1920, 1080, 3)
    big = np.ascontiguousarray(np.tile(synth.photo_rgb(1024, 1024, 4), (4, 4, 1)))
    check(hip, [dict(px=photo, quality=90), dict(px=photo, quality=95)])
    check(hip, [dict(px=big, quality=90)])
    check(hip, [dict(px=big, quality=97)])


# ---- batches -------------------------------------------------------------------------------------------------------------------

def test_mixed_batch_with_invalid_entries(hip):
    rng = np.random.default_rng(9)
    good = [dict(px=_rand(rng, 23, 41, 3), quality=90), dict(px=synth.photo_rgb(170, 130, 2), quality=95),
            dict(px=_rand(rng, 8, 8, 1), quality=0), dict(px=_rand(rng, 17, 33, 4), quality=91, neg=True),
            dict(px=_rand(rng, 40, 3, 2), quality=30)]
    bad = [dict(px=None), dict(px=_rand(rng, 4, 4, 3), w=0), dict(px=_rand(rng, 4, 4, 3), comp=5),
           dict(px=_rand(rng, 4, 4, 3), w=70000), dict(px=_rand(rng, 4, 4, 3), off=-1)]
    items = [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3], bad[3], good[4], bad[4]]
    streams, rc, st = encode(hip, items)
    assert rc == _capi.ERR_INVALID_ARG
    assert st == [0, _capi.ERR_INVALID_ARG] * 5
    for k, s in enumerate(streams):
        assert s == (JW.encode(items[k]["px"], items[k]["quality"]) if k % 2 == 0 else None)
    # run to run: the same batch twice gives the same bytes, whatever order the atomics land in
    again, _, _ = encode(hip, items)
    assert again == streams


def test_null_quality_means_90(hip):
    rng = np.random.default_rng(4)
    items = [dict(px=_rand(rng, 19, 29, 3)), dict(px=_rand(rng, 33, 17, 1))]
    streams, rc, st = encode(hip, items)
    assert rc == _capi.OK and st == [0, 0]
    assert streams == [JW.encode(it["px"], 90) for it in items]


def test_empty_batch(hip):
    assert hip.gamut_hip_jpeg_encode_batch_device(None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK


# ---- drop-ins, round trips, transcode -----------------------------------------------------------------------------------------

def test_drop_ins(hip):
    rng = np.random.default_rng(8)
    for (h, w, c, q) in ((37, 53, 3, 90), (20, 31, 1, 95), (9, 70, 4, 75), (16, 16, 2, 100)):
        px = _rand(rng, h, w, c) // 8 * 8
        exp = JW.encode(px, q)
        for pad, neg in ((0, False), (5, False), (3, True)):
            P = w * c + pad
            store = np.zeros((h, P), np.uint8)
            for y in range(h):
                store[h - 1 - y if neg else y, : w * c] = px[y].reshape(-1)
            ptr = store.ctypes.data + ((h - 1) * P if neg else 0)
            n = C.c_int(0)
            p = hip.gamut_hip_jpeg_encode(ptr, w, h, c, -P if neg else P, q, C.byref(n))
            assert p, _capi.last_error()
            assert C.string_at(p, n.value) == exp
            C.CDLL(None).free(C.c_void_p(p))
            chunks = []
            cb = _capi.JPEG_WRITE_FUNC(lambda ctx, data, size: chunks.append(C.string_at(data, size)))
            assert hip.gamut_hip_jpeg_write_to_func(C.cast(cb, C.c_void_p), None, w, h, c, ptr, -P if neg else P, q) == 1
            assert b"".join(chunks) == exp
    calls = []
    cb = _capi.JPEG_WRITE_FUNC(lambda ctx, data, size: calls.append(size))
    px = np.zeros(300, np.uint8)
    for args in ((10, 10, 0), (10, 10, 5), (0, 10, 3), (70000, 1, 1)):
        assert hip.gamut_hip_jpeg_write_to_func(C.cast(cb, C.c_void_p), None, *args, px.ctypes.data, 30, 90) == 0
    assert calls == []


def test_round_trip_through_the_decoders(hip):
    """GPU decode of GPU-encoded streams == the oracle's decode of the same bytes, pixel for pixel"""
    imgs = [synth.photo_rgb(257, 131, 4), synth.photo_rgb(176, 128, 6), np.ascontiguousarray(synth.photo_rgb(300, 200, 5)[:, :299])]
    items = [dict(px=imgs[0], quality=90), dict(px=imgs[1], quality=95), dict(px=imgs[2], quality=60)]
    streams = check(hip, items)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    n = len(bufs)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
    offs, total = [], 0
    for px in imgs:
        offs.append(total); total += px.shape[0] * px.shape[1] * 4
    out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    info = (_capi.ImageInfo * n)(); st = (C.c_int * n)()
    _capi.check(hip.gamut_hip_decode_batch_device(ptrs, lens, n, 4, (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None))
    o = out.cpu().numpy()
    for px, off, s in zip(imgs, offs, streams):
        exp = O.decompress_jpeg(s, 4)[0].reshape(-1)
        assert np.array_equal(o[off: off + exp.size], exp)


def test_transcode_from_decoded_pixels(hip):
    """JPEG, PNG and QOI files -> gamut_hip_decode_batch_device (rgba8 in HBM) -> the encoder with comp 4 straight from those
    pixels == the C restatement on the same pixels"""
    from PIL import Image
    photo = synth.photo_rgb(161, 127, 11)
    jb = io.BytesIO(); Image.fromarray(photo).save(jb, format="JPEG", quality=85)
    pb = io.BytesIO(); Image.fromarray(photo[:80, :120]).save(pb, format="PNG")
    files = [jb.getvalue(), pb.getvalue(), gen.qoi_encode(np.concatenate([photo[:50, :70], np.full((50, 70, 1), 200, np.uint8)], -1))]
    dims = [(127, 161), (80, 120), (50, 70)]
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
    offs, total = [], 0
    for h, w in dims:
        offs.append(total); total += h * w * 4 + 64
    dec = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    info = (_capi.ImageInfo * n)(); st = (C.c_int * n)()
    _capi.check(hip.gamut_hip_decode_batch_device(ptrs, lens, n, 4, (C.c_int64 * n)(*offs), dec.data_ptr(), info, st, None))
    torch.cuda.synchronize()
    src = (C.c_void_p * n)(*[dec.data_ptr() + o for o in offs]); pitch = (C.c_int64 * n)(*[w * 4 for h, w in dims])
    W = (C.c_int * n)(*[w for h, w in dims]); H = (C.c_int * n)(*[h for h, w in dims]); CO = (C.c_int * n)(4, 4, 4)
    Q = (C.c_int * n)(90, 95, 75)
    bnd = [hip.gamut_hip_jpeg_encode_bound(w, h, 4, q) for (h, w), q in zip(dims, Q)]
    eoffs = np.cumsum([0] + bnd[:-1]).astype(np.int64)
    out = torch.zeros(sum(bnd), dtype=torch.uint8, device="cuda:0")
    lens_o = (C.c_int64 * n)(); st2 = (C.c_int * n)()
    _capi.check(hip.gamut_hip_jpeg_encode_batch_device(src, pitch, W, H, CO, Q, n, (C.c_int64 * n)(*eoffs), out.data_ptr(), lens_o, st2,
                                                       torch.cuda.current_stream().cuda_stream))
    d, o = dec.cpu().numpy(), out.cpu().numpy()
    for k, ((h, w), q) in enumerate(zip(dims, Q)):
        pix = d[offs[k]: offs[k] + h * w * 4].reshape(h, w, 4)
        assert o[eoffs[k]: eoffs[k] + lens_o[k]].tobytes() == JW.encode(pix, q)


# ---- the Image mirror -------------------------------------------------------------------------------------------------------------

def _fill(img, px, layer=None):
    h = px.shape[0]
    for y in range(h):
        row = np.ascontiguousarray(px[y])
        C.memmove(img.scanptr(y) if layer is None else img.layerptr(layer, y), row.ctypes.data, row.nbytes)


def test_image_save_jpeg(hip, tmp_path):
    rng = np.random.default_rng(21)
    rgb = np.ascontiguousarray(synth.photo_rgb(170, 130, 8)[:37, :45])
    grey = rgb[:, :, 1].copy()
    for px, type_ in ((rgb, 9), (grey, 0)):
        exp = JW.encode(px, 90)
        flip = JW.encode(np.ascontiguousarray(px[::-1]), 90)
        host = gi.Image()
        assert host.create(45, 37, type_)
        _fill(host, px)
        data = host.save_to_memory(gi.FORMAT_JPEG)
        assert data == exp
        assert host.flipVertical() and host.isStoredUpsideDown                   # logical flip: negative pitch
        assert host.save_to_memory(gi.FORMAT_JPEG) == flip
        assert host.flipVertical()
        p = tmp_path / f"x{type_}.jpg"
        assert host.saveToFile(gi.FORMAT_JPEG, p) and p.read_bytes() == exp
        assert host.isValid and host.errorMessage is None
        back = gi.Image()
        assert back.loadFromMemory(data) and back.width == 45 and back.height == 37
        assert (back.pixelAspectRatio, back.dotsPerInchY) == (1.0, -1.0)                # JFIF, no units, 1:1
    # device-resident: rgb8 loaded straight into HBM (a QOI file), and its l8 conversion there; saved from HBM
    dev = gi.Image(device=True)
    assert dev.loadFromMemory(gen.qoi_encode(rgb)) and dev.isDevice and dev.type == 9
    assert dev.save_to_memory(gi.FORMAT_JPEG) == JW.encode(rgb, 90)
    assert dev.flipVertical()
    assert dev.save_to_memory(gi.FORMAT_JPEG) == JW.encode(np.ascontiguousarray(rgb[::-1]), 90)
    assert dev.convertToGreyscale() and dev.isDevice and dev.type == 0
    g = dev.pixels()
    assert dev.save_to_memory(gi.FORMAT_JPEG) == JW.encode(g, 90)
    p = tmp_path / "dev.jpg"
    assert dev.saveToFile(gi.FORMAT_JPEG, p) and p.read_bytes() == JW.encode(g, 90)
    # layer 0 of a multi-layer image
    lay = gi.Image()
    assert lay.createLayered(45, 37, 3, 9)
    for k in range(3):
        _fill(lay, (rgb.astype(np.int32) + 40 * k).clip(0, 255).astype(np.uint8), layer=k)
    assert lay.save_to_memory(gi.FORMAT_JPEG) == JW.encode(rgb, 90)
