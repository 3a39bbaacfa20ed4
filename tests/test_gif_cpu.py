"""GIF without a GPU: the serial restatement of the reference (tests/c/gif_ref.c) against Pillow where the two agree by construction;
the host parser and code walk gamut_hip_gif_read_header against the restatement on every generated case and on 20 000 mutated files;
the struct's layout; argument checks; format detection; the Image layer's refusal of a malformed file."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest

import gif_cases
import gif_gen
import gif_ref_c
from gamut_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = open(os.path.join(HERE, "golden", "gif", "animated_loop.gif"), "rb").read()


def lib_header(data):
    """gamut_hip_gif_read_header -> None when refused, else the six fields"""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    info = _capi.GifInfo()
    rc = _capi.lib().gamut_hip_gif_read_header(buf.ctypes.data, len(data), C.byref(info))
    if rc != _capi.OK:
        assert rc == _capi.ERR_DECODE, rc
        assert (info.width, info.height, info.layers, info.is_gif89, info.fps) == (0, 0, 0, 0, 0.0) and info.pixel_aspect_ratio == -1.0
        return None
    return info.width, info.height, info.layers, info.is_gif89, np.float32(info.pixel_aspect_ratio), np.float32(info.fps)


def ref_header(data):
    r = gif_ref_c.header(data)
    return None if r is None else (r[0]["width"], r[0]["height"], r[0]["layers"], r[0]["is_gif89"], r[1][0], r[1][1])


def _pillow_frames(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    return np.stack([np.asarray(f.convert("RGBA")) for f in ImageSequence.Iterator(im)])


def test_fixture_fields():
    assert len(FIXTURE) == 873
    px, info, f = gif_ref_c.load(FIXTURE)
    assert info == {"width": 100, "height": 100, "layers": 4, "is_gif89": 1} and px.shape == (4, 100, 100, 4)
    assert f[0] == -1.0 and f[1] == np.float32(4 * 1000.0 / 4000.0)
    assert lib_header(FIXTURE) == ref_header(FIXTURE)


def test_pillow_agrees_where_it_performs_the_same_transformation():
    """the restatement is not its own only witness: disposal 0 / 1, no transparency, frames inside the screen"""
    from PIL import Image
    files = [("fixture", FIXTURE)] + [(n, f) for n, f, pillow in gif_cases.cases() if pillow]
    rng = np.random.default_rng(9)
    frames = [np.clip(gif_gen.photo_like(rng, 96, 48).reshape(48, 96) // 8 + k * 3, 0, 255).astype(np.uint8) for k in range(2)]
    frames.append(np.repeat(np.repeat(rng.integers(0, 6, (6, 12), dtype=np.uint8) * 40, 8, 0), 8, 1))
    frames.insert(1, rng.integers(0, 256, (48, 96), dtype=np.uint8))
    for disposal in (0, 1):
        b = io.BytesIO()
        ims = [Image.fromarray(a, "L") for a in frames]
        ims[0].save(b, "GIF", save_all=True, append_images=ims[1:], duration=[40, 80, 120, 30], disposal=disposal, optimize=False)
        files.append((f"pillow_written_{disposal}", b.getvalue()))
    assert len(files) >= 20
    for name, f in files:
        ref = gif_ref_c.load(f)
        assert ref is not None, name
        got = _pillow_frames(f)
        assert got.shape == ref[0].shape and np.array_equal(got, ref[0]), name


def test_read_header_on_every_generated_case():
    cases = [(n, f) for n, f, _ in gif_cases.cases()] + [("three_frames", gif_cases.three_frames()), ("fixture", FIXTURE), ("empty", b""),
                                                       ("signature_only", b"GIF89a"), ("not_a_gif", b"GIF88a" + bytes(20))]
    n_ok = n_bad = 0
    for name, f in cases:
        a, b = ref_header(f), lib_header(f)
        assert a == b, (name, a, b)
        n_ok += a is not None; n_bad += a is None
    assert n_ok >= 60 and n_bad >= 15, (n_ok, n_bad)
    by_name = dict(cases)
    assert ref_header(by_name["zero_frames"]) == (40, 30, 0, 1, np.float32(-1), np.float32(10))
    assert ref_header(by_name["zero_frames_gif87"])[3:5] == (0, np.float32(1.0))
    assert ref_header(by_name["first_frame_sees_last_gce"])[5] == np.float32(5 * 1000.0 / (4 * 100 + 300))
    for refused in ("deferred_clear_crossing_8192", "no_clear_at_start", "avail_after_clear", "truncated_in_subblock", "overhang_right", "no_colour_table"):
        assert ref_header(by_name[refused]) is None, refused
    for accepted in ("deferred_clear_under_8192", "overhang_bottom", "data_after_end_code", "no_end_code", "frame_w0", "index_past_every_table"):
        assert ref_header(by_name[accepted]) is not None, accepted


def test_read_header_on_20000_mutated_files():
    files = gif_cases.mutated(20000, seed=5)
    n_ok = n_bad = 0
    for k, f in enumerate(files):
        a, b = ref_header(f), lib_header(f)
        assert a == b, (k, f.hex(), a, b)
        n_ok += a is not None; n_bad += a is None
    assert n_ok >= 2000 and n_bad >= 2000, (n_ok, n_bad)


def test_gif_info_layout_in_the_d_binding(tmp_path):
    """gamut_hip_gif_info: the C compiler's layout (tests/c/gif_abi_layout.c), the static assert in bindings/gamut_hip.d, the layout the D
    declaration yields, and the ctypes mirror"""
    exe = str(tmp_path / "gif_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "gif_abi_layout.c"), "-o", exe])
    f = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert f[0] == "gamut_hip_gif_info"
    c_size, c_fields = int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    assert c_size == 24 and list(c_fields) == ["width", "height", "layers", "is_gif89", "pixel_aspect_ratio", "fps"]
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    m = re.search(r"static assert\((\d+) == gamut_hip_gif_info\.sizeof(.*?)\);", dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n: int(v) for v, n in re.findall(r"(\d+) == gamut_hip_gif_info\.(\w+)\.offsetof", m.group(2))} == c_fields
    decl = re.search(r"struct gamut_hip_gif_info\s*\{(.*?)\}", dsrc, flags=re.S).group(1)
    off, fields = 0, {}
    for part in [x.strip() for x in decl.split(";") if x.strip()]:
        typ, names = part.split(None, 1)
        assert typ in ("int", "float")
        for n in names.split(","):
            fields[n.strip()] = off; off += 4
    assert (off, fields) == (c_size, c_fields)
    assert C.sizeof(_capi.GifInfo) == c_size and {n: getattr(_capi.GifInfo, n).offset for n, _ in _capi.GifInfo._fields_} == c_fields


def test_argument_validation_needs_no_device():
    L = _capi.lib()
    assert L.gamut_hip_gif_read_header(None, 0, None) == _capi.ERR_INVALID_ARG
    info = _capi.GifInfo()
    assert L.gamut_hip_gif_read_header(None, 100, C.byref(info)) == _capi.ERR_DECODE
    assert L.gamut_hip_gif_decode_batch_device(None, None, -1, None, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_gif_decode_batch_device(None, None, 2, None, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_gif_decode_batch_device(None, None, 0, None, None, None, None, None, None) == _capi.OK
    f = np.frombuffer(FIXTURE, np.uint8)
    ptrs = (C.c_void_p * 1)(f.ctypes.data); lens = (C.c_size_t * 1)(f.size); off = (C.c_int64 * 1)(0); cap = (C.c_int64 * 1)(1 << 20)
    out = np.full(64, 0xA5, np.uint8)
    for args in ((None, lens, 1, off, cap, out.ctypes.data), (ptrs, None, 1, off, cap, out.ctypes.data), (ptrs, lens, 1, None, cap, out.ctypes.data),
                 (ptrs, lens, 1, off, None, out.ctypes.data), (ptrs, lens, 1, off, cap, None)):
        assert L.gamut_hip_gif_decode_batch_device(*args, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_gif_last_kernel_ms(2) == -1.0
    if L.gamut_hip_device_count() == 0:                                    # no GPU: a loud failure, outputs untouched
        st = (C.c_int * 1)(55)
        assert L.gamut_hip_gif_decode_batch_device(ptrs, lens, 1, off, cap, out.ctypes.data, None, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and st[0] == 55 and b"no HIP device" in L.gamut_hip_last_error()
    else:                                                                  # a negative offset is the file's own refusal
        neg = (C.c_int64 * 1)(-4); st = (C.c_int * 1)(55)
        assert L.gamut_hip_gif_decode_batch_device(ptrs, lens, 1, neg, cap, out.ctypes.data, None, st, None) == _capi.ERR_INVALID_ARG
        assert st[0] == _capi.ERR_INVALID_ARG and (out == 0xA5).all()


def test_identify_format_gif():
    from gamut_amd import image as gi
    L = gi.lib()

    def ident(data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return L.gamut_identify_format_from_memory(buf.ctypes.data, len(data)), L.gamut_hip_identify_format(buf.ctypes.data, len(data))
    assert gi.FORMAT_GIF == 6
    assert ident(FIXTURE) == (6, -1) and ident(b"GIF87a") == (6, -1) and ident(b"GIF89a" + bytes(9)) == (6, -1)
    assert ident(b"GIF88a" + bytes(9)) == (-1, -1) and ident(b"GIF89") == (-1, -1) and ident(b"") == (-1, -1)


@pytest.mark.parametrize("device", [False])
def test_image_refuses_a_malformed_gif_without_a_gpu(device):
    from gamut_amd import image as gi
    by_name = {n: f for n, f, _ in gif_cases.cases()}
    for name in ("truncated_in_subblock", "avail_after_clear", "overhang_right", "no_colour_table", "unknown_extension"):
        im = gi.Image(device=device)
        assert not im.loadFromMemory(by_name[name]), name
        assert im.isError and im.errorMessage == "Image decoding failed" and im.type == -1, name
    im = gi.Image()
    assert not im.loadFromMemory(b"GIF89a")
    assert im.errorMessage == "Image decoding failed"
    assert not im.loadFromMemory(b"GIF88a" + bytes(30)) and im.errorMessage != "Image decoding failed"      # not identified at all
