"""GIF encode without a GPU: the new exports and their argument rules, the two readings of the reference (tests/c/gif_encode_ref.c and
tests/gif_encode_ref.py) against each other on every named case, the reference's files read back by the GIF decoder's reference and by
Pillow, and the Image layer's refusals."""
import ctypes as C
import io

import numpy as np

import gif_encode_cases as cases
import gif_encode_ref as ref_py
import gif_encode_ref_c as ref_c
import gif_ref_c
from gamut_amd import _capi


def test_exports_bound_and_refusals():
    L = _capi.lib()
    for name in ("gamut_hip_gif_encode_bound", "gamut_hip_gif_encode_batch_device", "gamut_hip_gif_write_to_mem", "gamut_hip_gif_last_encode_kernel_ms"):
        assert name in _capi.SIGNATURES and getattr(L, name)
    for w, h, f in [(1, 1, 1), (5, 3, 2), (480, 270, 16), (65535, 1, 1), (1, 65535, 3), (23170, 23170, 1)]:
        assert L.gamut_hip_gif_encode_bound(w, h, f) == 32 + f * (32 + 768 + w * h * 3 // 2 + 256) + 1 == ref_c.bound(w, h, f)
    for w, h, f in [(0, 1, 1), (1, 0, 1), (-3, 4, 1), (65536, 1, 1), (1, 65536, 1), (4, 4, 0), (4, 4, -1), (23171, 23171, 1), (65535, 65535, 1)]:
        assert L.gamut_hip_gif_encode_bound(w, h, f) == 0                   # 23171^2 * 4 > INT_MAX: the reference's int sizes wrap
    assert L.gamut_hip_gif_last_encode_kernel_ms(0) == -1.0 and L.gamut_hip_gif_last_encode_kernel_ms(9) == -1.0


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    assert L.gamut_hip_gif_encode_batch_device(None, None, None, None, None, None, None, None, None, 0, None, None, None, None, None) == _capi.OK
    assert L.gamut_hip_gif_encode_batch_device(None, None, None, None, None, None, None, None, None, -1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_gif_encode_batch_device(None, None, None, None, None, None, None, None, None, 2, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert b"bad arguments" in L.gamut_hip_last_error()
    px = np.zeros(64, np.uint8); n = C.c_int(77)
    for args in [(None, 16, 64, 4, 4, 1), (px.ctypes.data, 16, 64, 0, 4, 1), (px.ctypes.data, 16, 64, 4, 4, 0), (px.ctypes.data, 16, 64, 65536, 1, 1)]:
        assert not L.gamut_hip_gif_write_to_mem(*args, 7, 16, 10, C.byref(n)) and n.value == 77
        assert b"invalid arguments" in L.gamut_hip_last_error()
    assert not L.gamut_hip_gif_write_to_mem(px.ctypes.data, 16, 64, 4, 4, 1, 7, 16, 10, None)


def test_no_gpu_is_a_loud_failure_with_the_output_untouched():
    L = _capi.lib()
    if L.gamut_hip_device_count() > 0:
        return                                                              # (with a GPU the same call is checked in test_gif_encode_gpu.py)
    px = np.zeros(4 * 4 * 4, np.uint8); out = np.full(4096, 0xA5, np.uint8)
    src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(16); lo = (C.c_int64 * 1)(64); w = (C.c_int32 * 1)(4); f = (C.c_int32 * 1)(1)
    off = (C.c_int64 * 1)(0); olen = (C.c_int64 * 1)(99); st = (C.c_int * 1)(55)
    assert L.gamut_hip_gif_encode_batch_device(src, pitch, lo, w, w, f, None, None, None, 1, off, out.ctypes.data, olen, st, None) == _capi.ERR_NO_DEVICE
    assert b"no HIP device" in L.gamut_hip_last_error()
    assert (out == 0xA5).all() and olen[0] == 99 and st[0] == 55
    n = C.c_int(77)
    assert not L.gamut_hip_gif_write_to_mem(px.ctypes.data, 16, 64, 4, 4, 1, 7, 16, 10, C.byref(n)) and n.value == 77


def test_vector_body_and_scalar_tail_cook_alike():
    """msf_cook_frame's 4-pixel body (16-bit lanes: wrapping multiply, saturating add) and its scalar tail, restated separately in the C
    reference, give the same value for every channel level at every depth and dither position, and the numpy reading gives it too"""
    levels = np.arange(256, dtype=np.uint8)
    for depth in range(1, 17):
        for y in range(4):
            for x in range(4):
                img = np.zeros((y + 1, x + 1, 4), np.uint8)
                for v in (0, 1, 7, 8, 127, 128, 129, 200, 247, 248, 254, 255):
                    px = np.array([v, 255 - v, (v * 7) & 255, 255], np.uint8)
                    a, b = ref_c.cook_both(px, x, y, depth, 10)
                    img[y, x] = px
                    assert a == b == int(ref_py.cook(img, depth, 10)[y, x]), (depth, x, y, v)
    rng = np.random.default_rng(1)
    for _ in range(3000):
        px = rng.integers(0, 256, 4, dtype=np.uint8); d = int(rng.integers(1, 17)); x, y = map(int, rng.integers(0, 9, 2))
        a, b = ref_c.cook_both(px, x, y, d, 10)
        assert a == b
    assert levels.size == 256


def test_the_two_readings_agree_on_every_case():
    names = set()
    for name, frames, kw, data, rep in cases.all_cases():
        assert ref_py.encode(frames, **kw) == data, name
        assert len(data) <= ref_c.bound(frames.shape[2], frames.shape[1], frames.shape[0]), name
        names.add(name)
    assert len(names) == len(cases.all_cases()) >= 40


def test_cases_cover_what_the_encoder_can_do():
    reps = {name: rep for name, _, _, _, rep in cases.all_cases()}
    assert {r["table_bits"] for rep in reps.values() for r in rep} == {2, 3, 4, 5, 6, 7, 8}
    assert {ref_c.LAST_PARTIAL, ref_c.LAST_NONE_AFTER_ROLLOVER, ref_c.LAST_EXACTLY_FULL} == {r["last_kind"] for rep in reps.values() for r in rep}
    assert any(r["resets"] for rep in reps.values() for r in rep)
    assert len({r["depth"] for rep in reps.values() for r in rep}) >= 6


def _expected_layers(frames, kw, rep):
    """what a decoder must show: every pixel the palette colour of its cooked value at the frame's depth, alpha 255; alpha 0 where cooked transparent"""
    out = np.zeros(frames.shape, np.uint8)
    for f, r in enumerate(rep):
        d = r["depth"]
        v = ref_py.cook(frames[f], d, kw.get("alpha_threshold", 10))
        rb, gb, bb = ref_py.RBITS[d], ref_py.GBITS[d], ref_py.BBITS[d]
        rep8 = np.vectorize(ref_py.replicate)
        out[f, ..., 0] = rep8(v & ((1 << rb) - 1), rb)
        out[f, ..., 1] = rep8(v >> rb & ((1 << gb) - 1), gb)
        out[f, ..., 2] = rep8(v >> (rb + gb) & ((1 << bb) - 1) if bb else v * 0, bb)
        out[f, ..., 3] = 255
        out[f][v == 1 << d] = 0
    return out


def test_the_references_files_read_back():
    from PIL import Image, ImageSequence
    L = _capi.lib()
    n_pillow = 0
    for name, frames, kw, data, rep in cases.all_cases():
        info = _capi.GifInfo()
        buf = np.frombuffer(data, np.uint8)
        assert L.gamut_hip_gif_read_header(buf.ctypes.data, buf.size, C.byref(info)) == _capi.OK, name
        assert (info.width, info.height, info.layers, info.is_gif89) == (frames.shape[2], frames.shape[1], frames.shape[0], 1), name
        got = gif_ref_c.load(data)
        assert got is not None, name
        want = _expected_layers(frames, kw, rep)
        transparent = any(r["has_transparent"] for r in rep)
        if not transparent:
            assert np.array_equal(got[0], want), name
            with Image.open(io.BytesIO(data)) as im:
                seq = [np.asarray(fr.convert("RGBA")) for fr in ImageSequence.Iterator(im)]
            assert len(seq) == frames.shape[0] and all(np.array_equal(s, w) for s, w in zip(seq, want)), name
            n_pillow += 1
        else:
            opaque = want[..., 3] == 255
            assert np.array_equal(got[0][opaque], want[opaque]), name
            assert (got[0][~opaque][:, 3] == 0).all(), name
    assert n_pillow >= 30


def test_image_save_gif_refusals(tmp_path):
    from gamut_amd import image as gi
    a = np.zeros((2, 3, 4 * 8), np.uint8)
    l8, rgb8, rgba16, blank, zero, bad = gi.Image(), gi.Image(), gi.Image(), gi.Image(), gi.Image(), gi.Image()
    assert l8.createView(a, 4, 3, 0, 4) and rgb8.createView(a, 4, 3, 9, 12) and rgba16.createView(a, 4, 3, 13, 32)
    assert zero.createLayered(4, 3, 0, 12) and zero.layers == 0
    assert not bad.loadFromMemory(b"GIF89a garbage")
    path = tmp_path / "never_written.gif"
    for im, typ in ((l8, 0), (rgb8, 9), (rgba16, 13), (blank, -1), (zero, 12), (bad, -1)):
        before = (im.type, im.width, im.height, im.layers, im.isValid, im.errorMessage)
        assert before[0] == typ
        assert im.save_to_memory(gi.FORMAT_GIF) is None and not im.saveToFile(gi.FORMAT_GIF, path) and not path.exists()
        assert (im.type, im.width, im.height, im.layers, im.isValid, im.errorMessage) == before      # no side effect on the image
    n = C.c_size_t(5)
    assert not gi.lib().gamut_image_save_to_memory(l8.h, gi.FORMAT_GIF, 0, C.byref(n)) and n.value == 0
    assert gi.FORMAT_GIF == 6
