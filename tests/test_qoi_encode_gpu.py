"""GPU QOI encode (qoi_encode.hip) through the C ABI: byte-exact against tests/gen.py's serial encoder (small images) and Pillow's QOI
writer's payload plus the spec header (large ones), batch behaviour, round trips through the decoders, and the Image mirror."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import gen
import oracle_lib as O
from gamut_amd import _capi, synth
from gamut_amd import image as gi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64


def _desc(w, h, ch, cs=0):
    d = _capi.QoiDesc()
    d.width, d.height, d.channels, d.colorspace = w, h, ch, cs
    return d


def encode(hip, items):
    """items: dicts with px ((h, w, ch) uint8, or None with a desc given), and optionally extra (pitch - row bytes), neg (rows stored
    bottom-up, negative pitch), shift (bytes of misalignment of the first stored row), desc, cs.  -> (streams (bytes or None), rc,
    statuses).  Every byte of the output buffer outside the streams must still hold the canary."""
    dev = torch.device("cuda", 0)
    blob_parts, metas, at = [], [], 0
    for it in items:
        px = it.get("px")
        if px is None:
            metas.append((0, 0)); continue
        h, w, ch = px.shape
        P = w * ch + it.get("extra", 0)
        shift = it.get("shift", 0)
        store = np.zeros(shift + P * h, np.uint8)
        for y in range(h):
            r = (h - 1 - y) if it.get("neg") else y
            store[shift + r * P: shift + r * P + w * ch] = px[y].reshape(-1)
        first = at + shift + ((h - 1) * P if it.get("neg") else 0)
        metas.append((first, -P if it.get("neg") else P))
        blob_parts.append(store)
        at += store.size
        pad = (-at) % 16
        blob_parts.append(np.zeros(pad + 16, np.uint8)); at += pad + 16
    blob = torch.from_numpy(np.concatenate(blob_parts) if blob_parts else np.zeros(16, np.uint8)).to(dev)
    n = len(items)
    descs = (_capi.QoiDesc * max(n, 1))()
    src = (C.c_void_p * max(n, 1))(); pitch = (C.c_int64 * max(n, 1))(); offs = (C.c_int64 * max(n, 1))()
    lens = (C.c_int64 * max(n, 1))(); status = (C.c_int * max(n, 1))()
    total = GAP
    bounds = []
    for i, it in enumerate(items):
        px = it.get("px")
        d = it.get("desc") or _desc(px.shape[1], px.shape[0], px.shape[2], it.get("cs", 0))
        descs[i] = d
        src[i] = blob.data_ptr() + metas[i][0] if px is not None else 0
        pitch[i] = metas[i][1]
        b = hip.gamut_hip_qoi_encode_bound(C.byref(d))
        bounds.append(b)
        offs[i] = total
        total += b + GAP
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    rc = hip.gamut_hip_qoi_encode_batch_device(src, pitch, descs, n, offs, out.data_ptr(), lens, status,
                                               torch.cuda.current_stream().cuda_stream)
    o = out.cpu().numpy()
    keep = np.zeros(total, bool)
    streams = []
    for i in range(n):
        assert 0 <= lens[i] <= bounds[i]
        keep[offs[i]: offs[i] + lens[i]] = True
        streams.append(o[offs[i]: offs[i] + lens[i]].tobytes() if lens[i] else None)
    assert (o[~keep] == CANARY).all(), "bytes written outside the streams"
    return streams, rc, list(status[:n])


def enc1(hip, px, **kw):
    s, rc, st = encode(hip, [dict(px=px, **kw)])
    assert rc == _capi.OK and st == [0], _capi.last_error()
    return s[0]


def rgba(pixels, h=None):
    a = np.array(pixels, np.uint8).reshape(1 if h is None else h, -1, 4)
    return a


def _pillow(px):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, "RGBA" if px.shape[2] == 4 else "RGB").save(b, format="QOI")
    return b.getvalue()


def _spec_header(px, cs=0):
    h, w, ch = px.shape
    return b"qoif" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([ch, cs])


def check_small(hip, px, **kw):
    got = enc1(hip, px, **kw)
    assert got == gen.qoi_encode(px), (px.shape, kw)
    return got


# ---- byte-exact against gen.qoi_encode ------------------------------------------------------------------------------------

def test_tiny_shapes(hip):
    rng = np.random.default_rng(1)
    for ch in (3, 4):
        for h, w in [(1, 1), (1, 2), (1, 1023), (1, 1024), (1, 1025), (1, 3001), (3001, 1), (1025, 1), (2, 1)]:
            check_small(hip, rng.integers(0, 256, (h, w, ch), dtype=np.uint8))
    check_small(hip, np.array([[[0, 0, 0, 255]]], np.uint8))                 # the start state: a run of one
    check_small(hip, np.array([[[0, 0, 0]]], np.uint8))


def test_leading_start_state_pixels_never_enter_the_table(hip):
    px = rgba([(0, 0, 0, 255), (1, 1, 1, 255), (0, 0, 0, 255)])
    got = check_small(hip, px)
    assert got[14:-8] == bytes([0xC0, 0x7F, 0x55])                          # RUN 1, DIFF, DIFF -- not INDEX 53
    px = rgba([(0, 0, 0, 0), (0, 0, 0, 0), (5, 5, 5, 0)])                    # INDEX 0 on the zeroed table, then a run
    got = check_small(hip, px)
    assert got[14] == 0x00
    # the same across tile boundaries: a long leading start-state run, then the start-state value again far later
    a = np.zeros((1, 5000, 4), np.uint8); a[..., 3] = 255
    a[0, 3000] = (9, 9, 9, 255)
    check_small(hip, a)


@pytest.mark.parametrize("ch", [3, 4])
def test_runs(hip, ch):
    rng = np.random.default_rng(ch)
    for L in (61, 62, 63, 124, 125, 1023, 1024, 1025, 2048 + 62, 3000):
        for lead in (0, 1, 1000, 1023):
            base = rng.integers(0, 256, (lead + L + 5, ch), dtype=np.uint8)
            base[lead: lead + L] = base[lead]
            check_small(hip, base.reshape(1, -1, ch))
            check_small(hip, base[: lead + L].reshape(1, -1, ch))             # a run that ends the image
            w = 37                                                            # runs across rows
            n = (base.shape[0] // w) * w
            if n:
                check_small(hip, base[:n].reshape(-1, w, ch))


def test_alpha_changes_and_palette_content(hip):
    rng = np.random.default_rng(7)
    for it in range(40):
        ch = 4 if it % 2 else 3
        pal = rng.integers(0, 256, (int(rng.integers(1, 9)), ch), dtype=np.uint8)
        if it % 3 == 0:
            pal[0] = (0, 0, 0, 255)[:ch]
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 90))
        px = pal[rng.integers(0, len(pal), (h, w))]
        if it % 4 == 0:                                                       # small deltas: DIFF / LUMA ops
            px = np.cumsum(rng.integers(-3, 3, (h, w, ch)), axis=1).astype(np.uint8)
        check_small(hip, px)


def test_index_carried_many_tiles_back_and_all_slots(hip):
    rng = np.random.default_rng(11)
    # one value early, then a long stretch that never touches its slot, then the value again: INDEX from many tiles back
    v = np.array([200, 10, 77, 255], np.uint8)
    hv = (200 * 3 + 10 * 5 + 77 * 7 + 255 * 11) % 64
    filler = []
    while len(filler) < 20000:
        c = rng.integers(0, 256, 4, dtype=np.uint8); c[3] = 255
        if (int(c[0]) * 3 + int(c[1]) * 5 + int(c[2]) * 7 + 255 * 11) % 64 != hv:
            filler.append(c)
    px = np.stack([v] + filler + [v])[None]
    got = check_small(hip, px)
    assert got[-9] == hv                                                      # the last op is QOI_OP_INDEX hv
    # all 64 slots filled in one tile, then looked up in the next ones
    vals = []
    while len(vals) < 64:
        c = rng.integers(0, 256, 4, dtype=np.uint8)
        if all((int(c[0]) * 3 + int(c[1]) * 5 + int(c[2]) * 7 + int(c[3]) * 11) % 64 != (int(u[0]) * 3 + int(u[1]) * 5 + int(u[2]) * 7 + int(u[3]) * 11) % 64 for u in vals):
            vals.append(c)
    vals = np.stack(vals)
    seq = np.concatenate([vals, np.repeat(vals[:1], 1000 - 64, 0), vals[rng.permutation(64)], vals[rng.integers(0, 64, 3000)]])
    check_small(hip, seq[None])


def test_geometry(hip):
    rng = np.random.default_rng(5)
    for ch in (3, 4):
        for w in (1, 3, 5, 33, 301):
            h = 23
            px = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
            px[5:9] = px[5, :1]                                               # runs across rows
            exp = gen.qoi_encode(px)
            for kw in (dict(), dict(extra=1), dict(extra=17), dict(neg=True), dict(neg=True, extra=3), dict(shift=1), dict(shift=3, extra=5),
                       dict(shift=2, neg=True)):
                assert enc1(hip, px, **kw) == exp, (ch, w, kw)
    px = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
    got = enc1(hip, px, cs=1)
    assert got[13] == 1 and got[14:] == gen.qoi_encode(px)[14:]


# ---- byte-exact against Pillow's payload + the spec header -------------------------------------------------------------

def test_1080p_photo_with_alpha(hip):
    pytest.importorskip("PIL")
    rgb = synth.photo_rgb(1920, 1080, 3)
    a = np.clip(np.linspace(0, 3, 1920)[None, :] * 255, 0, 255).astype(np.uint8).repeat(1080, 0)
    a[::7] = 255
    px = np.ascontiguousarray(np.concatenate([rgb, a[..., None]], 2))
    got = enc1(hip, px)
    assert got[:14] == _spec_header(px) and got[14:] == _pillow(px)[14:]
    got3 = enc1(hip, np.ascontiguousarray(rgb), extra=3)
    assert got3[:14] == _spec_header(rgb) and got3[14:] == _pillow(np.ascontiguousarray(rgb))[14:]


def test_flat_ui_content(hip):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(9)
    px = np.full((720, 1280, 4), 240, np.uint8); px[..., 3] = 255
    for _ in range(60):
        y, x = rng.integers(0, 700), rng.integers(0, 1200)
        px[y: y + rng.integers(4, 200), x: x + rng.integers(4, 300)] = (*rng.integers(0, 256, 3), 255)
    px[100:110, 100:400, 3] = 128
    got = enc1(hip, px)
    assert got[:14] == _spec_header(px) and got[14:] == _pillow(px)[14:]


def test_4096_constant_image(hip):
    px = np.empty((4096, 4096, 4), np.uint8); px[:] = (12, 34, 56, 255)
    got = enc1(hip, px)
    n = 4096 * 4096 - 1                                                       # one RGB op, then runs of 62 crossing every tile
    body = bytes([0xFE, 12, 34, 56]) + bytes([0xC0 | 61]) * (n // 62) + (bytes([0xC0 | (n % 62 - 1)]) if n % 62 else b"")
    assert got == _spec_header(px) + body + bytes([0, 0, 0, 0, 0, 0, 0, 1])


# ---- batch behaviour ------------------------------------------------------------------------------------------------------

def test_mixed_batch_with_invalid_descs(hip):
    rng = np.random.default_rng(3)
    items = []
    for i in range(2000):
        ch = 3 + i % 2
        items.append(dict(px=rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), ch), dtype=np.uint8) // 64 * 64))
    big = [synth.photo_rgb(640, 480, s) for s in (1, 2)]
    items.insert(7, dict(px=big[0]))
    items.insert(1500, dict(px=big[1], neg=True))
    items.insert(3, dict(px=None, desc=_desc(0, 5, 4)))
    items.insert(900, dict(px=None, desc=_desc(5, 5, 2)))
    items.insert(1200, dict(px=items[1199]["px"], desc=_desc(8, 8, 4, 3)))
    streams, rc, status = encode(hip, items)
    assert rc == _capi.ERR_INVALID_ARG
    for i, it in enumerate(items):
        if i in (3, 900, 1200):
            assert status[i] == _capi.ERR_INVALID_ARG and streams[i] is None
        else:
            assert status[i] == 0 and streams[i] == gen.qoi_encode(it["px"]), i


def test_empty_batch(hip):
    assert hip.gamut_hip_qoi_encode_batch_device(None, None, None, 0, None, None, None, None, None) == _capi.OK


# ---- round trips -----------------------------------------------------------------------------------------------------------

def test_round_trip_and_drop_in(hip):
    rng = np.random.default_rng(13)
    imgs = [synth.photo_rgb(257, 131, 4), rng.integers(0, 256, (40, 61, 4), dtype=np.uint8) // 32 * 32,
            np.ascontiguousarray(synth.photo_rgb(300, 200, 5)[:, :299])]
    streams, rc, _ = encode(hip, [dict(px=p) for p in imgs])
    assert rc == _capi.OK
    for px, s in zip(imgs, streams):
        h, w, ch = px.shape
        exp, fc, cs = O.qoi_decode(s, 0)
        assert fc == ch and np.array_equal(exp.reshape(h, w, ch), px)
        buf = np.frombuffer(s, np.uint8); d = _capi.QoiDesc()
        p = hip.gamut_hip_qoi_decode(buf.ctypes.data, buf.size, C.byref(d), 0)
        assert p, _capi.last_error()
        got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h * w * ch,)).copy()
        C.CDLL(None).free(C.c_void_p(p))
        assert np.array_equal(got.reshape(h, w, ch), px)
        # the host drop-in: rows of a larger pitch, and upside down (negative pitch, pointer at row 0)
        for pad, neg in ((0, False), (5, False), (3, True)):
            P = w * ch + pad
            store = np.zeros((h, P), np.uint8)
            for y in range(h):
                store[h - 1 - y if neg else y, : w * ch] = px[y].reshape(-1)
            ptr = store.ctypes.data + ((h - 1) * P if neg else 0)
            n = C.c_int(0)
            q = hip.gamut_hip_qoi_encode(ptr, C.byref(_desc(w, h, ch)), -P if neg else P, C.byref(n))
            assert q, _capi.last_error()
            assert C.string_at(q, n.value) == s
            C.CDLL(None).free(C.c_void_p(q))
    # the GPU decoder's batch entry on the encoder's streams
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data for b in bufs]); sizes = (C.c_int * 3)(*[b.size for b in bufs])
    offs, total = [], 0
    for px in imgs:
        offs.append(total); total += px.size
    out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    descs = (_capi.QoiDesc * 3)(); st = (C.c_int * 3)()
    _capi.check(hip.gamut_hip_qoi_decode_batch_device(ptrs, sizes, 3, 0, (C.c_int64 * 3)(*offs), out.data_ptr(), descs, st, None))
    o = out.cpu().numpy()
    for px, off in zip(imgs, offs):
        assert np.array_equal(o[off: off + px.size], px.reshape(-1))


# ---- the Image mirror -------------------------------------------------------------------------------------------------------

def test_image_check_encode_scenario(hip, tmp_path):
    """image.d:2126-2175 checkEncode: a 3x1 rgb8 image saved as QOI and loaded back gives the same pixels"""
    img = gi.Image()
    assert img.create(3, 1, 9)
    pixels = np.array([255, 0, 0, 15, 64, 255, 0, 255, 255], np.uint8)
    C.memmove(img.scanptr(0), pixels.ctypes.data, 9)
    data = img.save_to_memory(gi.FORMAT_QOI)
    assert data == gen.qoi_encode(pixels.reshape(1, 3, 3))
    back = gi.Image()
    assert back.loadFromMemory(data) and back.type == 9 and back.width == 3 and back.height == 1
    assert np.array_equal(back.pixels()[0], pixels)
    p = tmp_path / "x.qoi"
    assert img.saveToFile(gi.FORMAT_QOI, p) and p.read_bytes() == data
    assert img.isValid and img.errorMessage is None


def test_image_upside_down_device_and_layers(hip):
    rng = np.random.default_rng(21)
    px = rng.integers(0, 256, (37, 29, 4), dtype=np.uint8) // 16 * 16
    exp = gen.qoi_encode(px)
    host = gi.Image()
    assert host.create(29, 37, 12)
    for y in range(37):
        C.memmove(host.scanptr(y), px[y].ctypes.data, 29 * 4)
    assert host.save_to_memory(gi.FORMAT_QOI) == exp
    assert host.flipVertical() and host.isStoredUpsideDown                   # logical flip: negative pitch
    assert host.save_to_memory(gi.FORMAT_QOI) == gen.qoi_encode(np.ascontiguousarray(px[::-1]))
    assert host.flipVertical()
    devimg = gi.Image(device=True)
    assert devimg.loadFromMemory(exp) and devimg.isDevice
    assert devimg.save_to_memory(gi.FORMAT_QOI) == exp                      # HBM-resident: same bytes as the host twin
    assert devimg.flipVertical()
    assert devimg.save_to_memory(gi.FORMAT_QOI) == gen.qoi_encode(np.ascontiguousarray(px[::-1]))
    rgb = gi.Image(device=True)
    assert rgb.loadFromMemory(gen.qoi_encode(px[..., :3].copy())) and rgb.type == 9
    assert rgb.save_to_memory(gi.FORMAT_QOI) == gen.qoi_encode(px[..., :3].copy())
    lay = gi.Image()
    assert lay.createLayered(29, 37, 3, 12)
    for k in range(3):
        for y in range(37):
            C.memmove(lay.layerptr(k, y), np.ascontiguousarray(px[y] + k).ctypes.data, 29 * 4)
    assert lay.save_to_memory(gi.FORMAT_QOI) == exp                          # layer 0 only
