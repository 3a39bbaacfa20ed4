"""GIF encode on the GPU against the serial C restatement of the reference (tests/c/gif_encode_ref.c), byte for byte: every named case
of tests/gif_encode_cases.py in batched calls with guards around every slot, independence from the batch, refusals inside a batch,
source layouts, the host drop-in, the Image layer, and one 200 x 150 x 4 animation."""
import ctypes as C

import numpy as np
import pytest
import torch

import gif_encode_cases as cases
import gif_encode_ref_c as ref_c
from gamut_amd import _capi
from test_gif_cpu import FIXTURE

pytestmark = pytest.mark.gpu
GUARD = 257                                                                 # at least this many guard bytes in front of and behind every slot


@pytest.fixture(scope="module")
def L(hip):
    return hip


def _place(frames, layout):
    """frames (n, h, w, 4) -> (host buffer, byte offset of layer 0 row 0, pitch, layer offset) in the named source layout"""
    n, h, w, _ = frames.shape
    row = w * 4
    if layout == "tight":
        return frames.reshape(-1).copy(), 0, row, row * h
    if layout == "padded":                                                  # rows 12 bytes apart more than they need, layers further apart than tight
        pitch, lo = row + 12, (row + 12) * h + 40
        buf = np.full(lo * n, 0xEE, np.uint8)
        for l in range(n):
            for y in range(h):
                buf[l * lo + y * pitch:l * lo + y * pitch + row] = frames[l, y].reshape(-1)
        return buf, 0, pitch, lo
    if layout == "upside_down":                                             # negative pitch: row 0 is the last one in memory
        buf = frames[:, ::-1].reshape(-1).copy()
        return buf, (h - 1) * row, -row, row * h
    if layout == "unaligned":                                               # odd address, odd pitch, odd layer offset
        pitch, lo = row + 3, (row + 3) * h + 5
        buf = np.full(1 + lo * n, 0xEE, np.uint8)
        for l in range(n):
            for y in range(h):
                buf[1 + l * lo + y * pitch:1 + l * lo + y * pitch + row] = frames[l, y].reshape(-1)
        return buf, 1, pitch, lo
    raise ValueError(layout)


def encode_batch(L, anims, refuse=None):
    """anims: [(frames, kwargs, layout)].  refuse: {index: dict of overrides (w, h, frames, src, off)} for animations that must be refused.
    -> (rc, statuses, lengths, whole output allocation, offsets, expected allocation)"""
    refuse = refuse or {}
    n = len(anims)
    keep, srcs, pitches, los, ws, hs, fs, cs, md, at, offs = [], [], [], [], [], [], [], [], [], [], []
    refs, pos = [], GUARD
    for i, (frames, kw, layout) in enumerate(anims):
        buf, at0, pitch, lo = _place(frames, layout)
        dev = torch.from_numpy(buf).cuda()
        keep.append(dev)
        ov = refuse.get(i, {})
        nfr, h, w, _ = frames.shape
        srcs.append(ov.get("src", dev.data_ptr() + at0)); pitches.append(pitch); los.append(lo)
        ws.append(ov.get("w", w)); hs.append(ov.get("h", h)); fs.append(ov.get("frames", nfr))
        cs.append(kw.get("centiseconds", 7)); md.append(kw.get("max_bit_depth", 16)); at.append(kw.get("alpha_threshold", 10))
        refs.append(None if i in refuse else ref_c.encode(frames, **kw)[0])
        assert pos % 2 == 1                                                 # EVERY slot starts at an odd byte offset
        offs.append(ov.get("off", pos))
        pos = (pos + ref_c.bound(w, h, nfr) + GUARD) | 1
    expect = np.full(pos, 0xA5, np.uint8)
    for r, o in zip(refs, offs):
        if r is not None:
            expect[o:o + len(r)] = np.frombuffer(r, np.uint8)
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    i32 = lambda v: (C.c_int32 * n)(*v)
    i64 = lambda v: (C.c_int64 * n)(*v)
    olen = (C.c_int64 * n)(*([-5] * n)); st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_gif_encode_batch_device((C.c_void_p * n)(*srcs), i64(pitches), i64(los), i32(ws), i32(hs), i32(fs), i32(cs), i32(md), i32(at), n,
                                             i64(offs), out.data_ptr(), olen, st, None)
    return rc, list(st), list(olen), out.cpu().numpy(), refs, expect


def check_batch(L, anims, names):
    rc, st, olen, got, refs, expect = encode_batch(L, anims)
    assert rc == 0 and st == [0] * len(anims), (rc, st, L.gamut_hip_last_error())
    assert olen == [len(r) for r in refs], [(nm, a, len(r)) for nm, a, r in zip(names, olen, refs) if a != len(r)]
    if not np.array_equal(got, expect):                                     # the WHOLE allocation, guards included
        at = int(np.flatnonzero(got != expect)[0])
        raise AssertionError(f"first difference at byte {at} of the allocation; lengths {olen}; cases {names}")


ALL = cases.all_cases()


@pytest.mark.parametrize("part", range(3))
def test_all_cases_batched(L, part):
    """mixed geometries and frame counts in one call; the whole allocation is compared"""
    mine = ALL[part::3]
    layouts = ("tight", "padded", "upside_down", "unaligned")
    check_batch(L, [(fr, kw, layouts[(k + part) % 4] if part == 2 else "tight") for k, (_, fr, kw, _, _) in enumerate(mine)], [c[0] for c in mine])


def test_each_alone_gives_the_same_bytes(L):
    by_name = {c[0]: c for c in ALL}
    for name in ("size_65x2", "noise_128x96", "transparent_in_frame_2_of_3", "one_changed_row", "nothing_left_after_rollover", "noise_then_few"):
        _, fr, kw, data, _ = by_name[name]
        check_batch(L, [(fr, kw, "tight")], [name])


def test_refusals_inside_a_batch(L):
    by_name = {c[0]: c for c in ALL}
    picks = ["size_5x3", "few_then_noise", "size_7x4", "identical_frames", "colours_16", "alpha_9_and_10", "size_3x1"]
    anims = [(by_name[p][1], by_name[p][2], "tight") for p in picks]
    refuse = {0: {"w": 0}, 2: {"w": 65536}, 3: {"frames": 0}, 4: {"src": None}, 5: {"off": -1}}
    rc, st, olen, got, refs, expect = encode_batch(L, anims, refuse)
    want = [_capi.ERR_INVALID_ARG if i in refuse else 0 for i in range(len(anims))]
    assert st == want and rc == _capi.ERR_INVALID_ARG and b"image 0" in L.gamut_hip_last_error()
    assert olen == [0 if r is None else len(r) for r in refs]
    assert np.array_equal(got, expect)                                      # neighbours encoded, refused slots and guards untouched


@pytest.mark.parametrize("layout", ["padded", "upside_down", "unaligned"])
def test_source_layouts(L, layout):
    by_name = {c[0]: c for c in ALL}
    picks = ["size_257x3", "bit_splits_differ", "transparent_in_frame_2_of_3", "size_1x5"]
    check_batch(L, [(by_name[p][1], by_name[p][2], layout) for p in picks], picks)


def test_host_drop_in(L):
    by_name = {c[0]: c for c in ALL}
    for name in ("few_then_noise", "size_65x2", "centiseconds_70000", "max_bit_depth_5"):
        _, fr, kw, data, _ = by_name[name]
        for layout in ("tight", "upside_down", "padded"):
            buf, at0, pitch, lo = _place(fr, layout)
            n = C.c_int(0)
            p = L.gamut_hip_gif_write_to_mem(buf.ctypes.data + at0, pitch, lo, fr.shape[2], fr.shape[1], fr.shape[0], kw.get("centiseconds", 7),
                                             kw.get("max_bit_depth", 16), kw.get("alpha_threshold", 10), C.byref(n))
            assert p, L.gamut_hip_last_error()
            try:
                assert C.string_at(p, n.value) == data, (name, layout)
            finally:
                C.CDLL(None).free(C.c_void_p(p))


def test_image_layer(L, tmp_path):
    from gamut_amd import image as gi
    host, dev = gi.Image(), gi.Image(device=True)
    assert host.loadFromMemory(FIXTURE) and dev.loadFromMemory(FIXTURE) and dev.isDevice and host.type == 12 and host.layers > 1
    w, h, n = host.width, host.height, host.layers
    px = np.stack([host.pixels(l).reshape(h, w, 4) for l in range(n)])
    want = ref_c.encode(px)[0]                                              # saveGIF: 7 centiseconds, depth 16, threshold 10
    a, b = host.save_to_memory(gi.FORMAT_GIF), dev.save_to_memory(gi.FORMAT_GIF)
    assert a == want and b == want
    again = gi.Image()
    assert again.loadFromMemory(a) and (again.width, again.height, again.layers, again.type) == (w, h, n, 12)
    path = tmp_path / "saved.gif"
    assert dev.saveToFile(gi.FORMAT_GIF, path) and path.read_bytes() == want
    assert (dev.isValid, dev.layers, dev.width) == (True, n, w)             # the image is as it was
    # an upside-down view encodes as its flipped twin
    small = cases.photo_like(23, 9, 2, seed=4)
    flipped = np.ascontiguousarray(small[:, ::-1])
    view = gi.Image()
    assert view.createLayeredView(flipped.reshape(-1), 23, 9, 2, 12, -23 * 4, 23 * 9 * 4) and view.isStoredUpsideDown
    assert view.save_to_memory(gi.FORMAT_GIF) == ref_c.encode(small)[0]
    one = gi.Image()
    assert one.createView(small[0].reshape(-1), 23, 9, 12, 23 * 4) and one.save_to_memory(gi.FORMAT_GIF) == ref_c.encode(small[:1])[0]


def test_moderately_sized_animation(L):
    fr = cases.photo_like(200, 150, 4, seed=9)
    data, rep = ref_c.encode(fr)
    assert any(r["resets"] for r in rep) and any(r["depth"] < 16 for r in rep)
    check_batch(L, [(fr, {}, "tight")], ["photo_200x150x4"])


_TIMED_CHILD = """
import ctypes as C, numpy as np, torch
from gamut_amd import _capi
L = _capi.lib(); _capi.check(L.gamut_hip_init(0))
px = torch.from_numpy((np.arange(9 * 5 * 4) * 7).astype(np.uint8)).cuda(); out = torch.zeros(4096, dtype=torch.uint8, device='cuda')
one = lambda t, v: (t * 1)(v)
n = one(C.c_int64, 0); st = one(C.c_int, 9)
rc = L.gamut_hip_gif_encode_batch_device(one(C.c_void_p, px.data_ptr()), one(C.c_int64, 36), one(C.c_int64, 180), one(C.c_int32, 9), one(C.c_int32, 5),
                                         one(C.c_int32, 1), None, None, None, 1, one(C.c_int64, 0), out.data_ptr(), n, st, None)
ms = [L.gamut_hip_gif_last_encode_kernel_ms(k) for k in range(5)]
assert rc == 0 and st[0] == 0 and n[0] > 32 and all(0.0 <= m < 1000.0 for m in ms), (rc, ms)
assert L.gamut_hip_gif_last_encode_kernel_ms(5) == -1.0 and L.gamut_hip_gif_last_encode_kernel_ms(-1) == -1.0
print('timing ok', ms)
"""


def test_timing_aid_follows_the_environment(L):
    """GAMUT_HIP_GIF_TIMING is read once, at the process's first encode call: this process reports what its own environment says, and a
    fresh child process with the variable set reports a time for each of the five kernels"""
    import os
    import subprocess
    import sys
    check_batch(L, [(ALL[0][1], ALL[0][2], "tight")], [ALL[0][0]])
    e = os.environ.get("GAMUT_HIP_GIF_TIMING", "")
    try:
        on = int(e) != 0                                                    # (the library reads it with atoi)
    except ValueError:
        on = False
    ms = [L.gamut_hip_gif_last_encode_kernel_ms(k) for k in range(5)]
    assert all((m >= 0.0) if on else (m == -1.0) for m in ms), ms
    assert L.gamut_hip_gif_last_encode_kernel_ms(-1) == -1.0 and L.gamut_hip_gif_last_encode_kernel_ms(5) == -1.0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAMUT_HIP_GIF_TIMING="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _TIMED_CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "timing ok" in r.stdout, r.stdout[-2000:]
