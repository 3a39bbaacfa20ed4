"""The Image mirror before and after a change to its plumbing, byte for byte: every save entry on every pixel type it takes (and a few it
refuses), from a host image and from a device image; every produced file loaded back into both residencies under two sets of flags; and
one truncated copy of every file.  What is observed is compared with tests/golden/image_roundtrip.json, which is recorded by

    python -m tests.test_image_roundtrip_gpu --record [--commit ID]

on the MI355X from the commit whose behaviour is to be kept, and never by pytest.  The host digest and the device digest of a file are
recorded side by side; nothing here says they are equal."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import tempfile
import zlib

import numpy as np
import pytest

from gamut_amd import _capi
from gamut_amd import image as gi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_roundtrip.json")
W, H = 9, 8                                                    # an odd width: no pitch is aligned by accident; 8 is the smallest side SQZ takes
L8, L16, LA8, RGB8, RGBA8, RGBA16, RGBAP8 = 0, 1, 3, 9, 12, 13, 15
PIXEL_BYTES = {L8: 1, L16: 2, LA8: 2, RGB8: 3, RGBA8: 4, RGBA16: 8, RGBAP8: 4}
LOAD_FLAGS = (0, gi.LOAD_RGB | gi.LOAD_ALPHA | gi.LOAD_16BIT | gi.LAYOUT_VERT_FLIPPED)
RESIDENCIES = ("host", "device")

# name -> (type, layers, layout constraints); the pixels are drawn in this order from one generator
SOURCES = {
    "l8": (L8, 1, 0), "la8": (LA8, 1, 0), "rgb8": (RGB8, 1, 0), "rgba8": (RGBA8, 1, 0), "rgbap8": (RGBAP8, 1, 0),
    "l16": (L16, 1, 0), "rgba16": (RGBA16, 1, 0), "rgba8x3": (RGBA8, 3, 0),
    "rgb8_flipped": (RGB8, 1, gi.LAYOUT_VERT_FLIPPED | gi.LAYOUT_ALIGNED[16]),      # a negative pitch and padded rows
}


def _generic(fif):
    return (lambda im, flags: im.save_to_memory(fif, flags), lambda im, path, flags: im.saveToFile(fif, path, flags))


# entry -> (to memory, to file)
ENTRIES = {
    "qoi": _generic(gi.FORMAT_QOI), "jpeg": _generic(gi.FORMAT_JPEG), "gif": _generic(gi.FORMAT_GIF),
    "generic_png": _generic(gi.FORMAT_PNG), "generic_bmp": _generic(gi.FORMAT_BMP), "generic_tga": _generic(gi.FORMAT_TGA),
    "generic_qoix": _generic(gi.FORMAT_QOIX), "generic_dds": _generic(gi.FORMAT_DDS), "generic_sqz": _generic(gi.FORMAT_SQZ),
    "png": (gi.Image.save_png_to_memory, gi.Image.savePNGToFile), "bmp": (gi.Image.save_bmp_to_memory, gi.Image.saveBMPToFile),
    "tga": (gi.Image.save_tga_to_memory, gi.Image.saveTGAToFile), "qoix": (gi.Image.save_qoix_to_memory, gi.Image.saveQOIXToFile),
    "dds": (gi.Image.save_dds_to_memory, gi.Image.saveDDSToFile), "sqz": (gi.Image.save_sqz_to_memory, gi.Image.saveSQZToFile),
}
# entry -> [(source, flags)]: every type the saver takes, the flipped rgb8 image where it takes rgb8, and at the end what it refuses
CASES = {
    "qoi": [("rgb8", 0), ("rgba8", 0), ("rgb8_flipped", 0), ("l8", 0)],
    "jpeg": [("l8", 0), ("rgb8", 0), ("rgb8_flipped", 0), ("rgba8", 0), ("la8", 0)],
    "gif": [("rgba8", 0), ("rgba8x3", 0), ("rgb8", 0)],
    "generic_png": [("rgb8", 0)], "generic_bmp": [("rgb8", 0)], "generic_tga": [("rgb8", 0)], "generic_qoix": [("rgb8", 0)],
    "generic_dds": [("rgb8", 0)], "generic_sqz": [("rgb8", 0)],
    "png": [("l8", 0), ("la8", 0), ("rgb8", 0), ("rgba8", 0), ("l16", 0), ("rgba16", 0), ("rgb8_flipped", 0), ("rgba8x3", 0), ("rgb8_density", 0),
            ("rgb8", gi.ENCODE_PNG_COMPRESSION_2 | gi.ENCODE_PNG_FILTER_FAST), ("rgbap8", 0), ("rgb8", 12)],
    "bmp": [("rgb8", 0), ("rgba8", 0), ("rgb8_flipped", 0), ("rgb8_density", 0), ("l8", 0), ("rgba8x3", 0)],
    "tga": [("l8", 0), ("la8", 0), ("rgb8", 0), ("rgba8", 0), ("rgb8_flipped", 0), ("rgba8x3", 0), ("l16", 0)],
    "qoix": [("rgb8", 0), ("rgba8", 0), ("rgbap8", 0), ("rgb8_flipped", 0), ("rgb8_density", 0), ("l8", 0)],
    "dds": [("l8", 0), ("la8", 0), ("rgb8", 0), ("rgba8", 0), ("rgb8_flipped", 0), ("l16", 0)],
    "sqz": [("rgb8", 0), ("rgb8_flipped", 0), ("rgb8", gi.ENCODE_SQZ_QUALITY_BPP1_0), ("rgba8", 0), ("l8", 0)],
}
SQZ_TO_DEVICE = [("rgb8", 0), ("rgb8_flipped", 0), ("rgb8", gi.ENCODE_SQZ_QUALITY_BPP1_0), ("rgba8", 0)]
NOT_READ = ("dds",)


def _sha(data):
    return None if data is None else hashlib.sha256(bytes(data)).hexdigest()


def _png_with_density(rows):
    """an rgb8 PNG of W x H with a pHYs chunk (3000 x 2000 pixels per metre): the one way a density gets into an image"""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"pHYs", struct.pack(">IIB", 3000, 2000, 1)) +
            chunk(b"IDAT", zlib.compress(b"".join(b"\0" + r.tobytes() for r in rows))) + chunk(b"IEND", b""))


def _images(L):
    """({source: {residency: Image}}, the PNG behind "rgb8_density"): the same fixed pixels in host memory and in HBM; "rgb8_density" is
    loaded from a PNG that states a density, so that the savers which write one (BMP, QOIX) have one to write"""
    rng = np.random.default_rng(20261021)
    out = {}
    for name, (type_, layers, layout) in SOURCES.items():
        row = W * PIXEL_BYTES[type_]
        px = rng.integers(0, 256, (layers, H, row), dtype=np.uint8)
        out[name] = {}
        for res in RESIDENCIES:
            im = gi.Image(device=res == "device")
            assert im.createLayered(W, H, layers, type_, layout) and im.layers == layers and im.scanlineInBytes == row
            for l in range(layers):
                for y in range(H):
                    if res == "device":
                        _capi.check(L.gamut_hip_memcpy_h2d(im.layerptr(l, y), px[l, y].ctypes.data, row, None))
                    else:
                        C.memmove(im.layerptr(l, y), px[l, y].ctypes.data, row)
            _capi.check(L.gamut_hip_stream_synchronize(None))
            assert all(np.array_equal(im.pixels(l), px[l]) for l in range(layers))
            out[name][res] = im
    flipped = out["rgb8_flipped"]
    assert all(im.pitchInBytes == -32 and im.isStoredUpsideDown for im in flipped.values())
    png = _png_with_density(rng.integers(0, 256, (H, W * 3), dtype=np.uint8))
    out["rgb8_density"] = {res: gi.Image(device=res == "device") for res in RESIDENCIES}
    assert all(im.loadFromMemory(png) and im.type == RGB8 and im.dotsPerInchY > 0 for im in out["rgb8_density"].values())
    return out, png


def _loaded(im):
    ok = im.isValid and im.hasData
    pixels = hashlib.sha256(b"".join(im.pixels(l).tobytes() for l in range(im.layers))).hexdigest() if ok else None
    return [im.type, im.width, im.height, im.layers, im.pitchInBytes, im.layerOffsetInBytes, im.layoutConstraints,
            float(im.pixelAspectRatio), float(im.dotsPerInchY), im.errorMessage, pixels]


def observe(L):
    """everything the fixture holds, observed on the library as it is built now"""
    images, png = _images(L)
    saves, files = {}, {_sha(png): (png, "png")}               # files: digest -> (bytes, entry), every distinct produced file once
    with tempfile.TemporaryDirectory() as tmp:
        for entry, cases in CASES.items():
            to_memory, to_file = ENTRIES[entry]
            for source, flags in cases:
                seen = saves[f"{entry}/{source}/{flags}"] = {}
                for res in RESIDENCIES:
                    im = images[source][res]
                    data = to_memory(im, flags)
                    path = os.path.join(tmp, "out.bin")
                    wrote = to_file(im, path, flags)
                    on_disk = None
                    if os.path.exists(path):
                        with open(path, "rb") as f:
                            on_disk = f.read()
                        os.remove(path)
                    assert wrote == (on_disk is not None), "a refused save leaves no file, a successful one leaves one"
                    seen[res] = {"memory": _sha(data), "file": _sha(on_disk)}
                    assert im.isValid and im.errorMessage is None
                    for produced in (data, on_disk):
                        if produced is not None:
                            files.setdefault(_sha(produced), (produced, entry))
    for source, flags in SQZ_TO_DEVICE:
        seen = saves[f"sqz_to_device/{source}/{flags}"] = {}
        for res in RESIDENCIES:
            got = images[source][res].save_sqz_to_device(flags)
            if got is not None:
                buf = np.zeros(got[1], np.uint8)
                _capi.check(L.gamut_hip_memcpy_d2h(buf.ctypes.data, got[0], got[1], None))
                _capi.check(L.gamut_hip_stream_synchronize(None))
                files.setdefault(_sha(buf.tobytes()), (buf.tobytes(), "sqz"))
                got = _sha(buf.tobytes())
            seen[res] = {"device_file": got}
    loads, truncated = {}, {}
    for digest, (data, entry) in files.items():
        if entry in NOT_READ:
            continue
        loads[digest], truncated[digest] = {}, {}
        for res in RESIDENCIES:
            for flags in LOAD_FLAGS:
                im = gi.Image(device=res == "device")
                im.loadFromMemory(data, flags)
                loads[digest][f"{res}/{flags}"] = _loaded(im)
            im = gi.Image(device=res == "device")
            im.loadFromMemory(data[:len(data) // 2], 0)
            truncated[digest][res] = [im.isValid, im.errorMessage, im.hasData]
    return {"saves": saves, "loads": loads, "truncated": truncated}


def _library():
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    return L


def record(commit):
    seen = observe(_library())
    seen["recorded_on"] = {"commit": commit, "device": "MI355X"}
    with open(GOLDEN, "w") as f:
        json.dump(seen, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(seen['saves'])} saves, {len(seen['loads'])} files loaded back -> {GOLDEN}")


@pytest.fixture(scope="module")
def seen(hip):
    return json.loads(json.dumps(observe(hip)))               # through JSON, as the fixture went: tuples and floats compare alike


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _differences(want, got):
    return {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}


def test_every_save_entry_writes_the_recorded_file_or_refuses(seen, golden):
    assert set(golden["saves"]) == set(seen["saves"])
    for refused in ("jpeg/rgba8/0", "sqz/rgba8/0", "generic_png/rgb8/0"):
        assert all(v is None for r in golden["saves"][refused].values() for v in r.values())
    assert not _differences(golden["saves"], seen["saves"])


def test_every_file_loads_back_to_the_recorded_image(seen, golden):
    """[type, width, height, layers, pitchInBytes, layerOffsetInBytes, layoutConstraints, pixelAspectRatio, dotsPerInchY, errorMessage,
    sha256 of the pixels of all layers] for each file x residency x load flags"""
    assert golden["loads"] and not _differences(golden["loads"], seen["loads"])


def test_truncated_files_fail_as_recorded(seen, golden):
    """[isValid, errorMessage, hasData] for the first half of each file, in both residencies"""
    assert golden["truncated"] and not _differences(golden["truncated"], seen["truncated"])


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_image_roundtrip_gpu --record [--commit ID]")
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None)
