"""QOI-Plane (QOIX grey files) on the GPU against the serial C restatement of the reference (tests/c/qoiplane_ref.c, deviation P1
included), byte for byte, with gamut_hip_qoix_set_plane(1): every named case in one call per channel count, batches that mix colour
and grey files, the channel-family statuses, the switch turned off again, refused files among good neighbours, stored-only and LZ4-only
batches, the shapes at which k_qoix_plane takes another path (they are named cases: tests/qoiplane_cases.py groups() and geometry()),
rows on either side of the LDS row capacity, more waves than one round of the grid, every output alignment, the Image layer and the
host drop-in.  Each file sits at the end of its host buffer; output allocations are filled with 0xA5, carry 4 KiB guards and are
compared whole.  The switch is process-wide: every test runs inside a fixture that restores the value it found."""
import ctypes as C

import numpy as np
import pytest
import torch

import qoiplane_cases as K
import qoiplane_gen as P
import qoiplane_ref_c
import qoix_cases
import qoix_ref_c
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 4096
RC = {qoix_ref_c.REFUSED: _capi.ERR_DECODE, qoix_ref_c.UNSUPPORTED: _capi.ERR_UNSUPPORTED}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


@pytest.fixture(autouse=True)
def plane_on(L):
    prev = L.gamut_hip_qoix_set_plane(1)
    yield
    L.gamut_hip_qoix_set_plane(prev)


@pytest.fixture(scope="module")
def CAP(L):
    return L.gamut_hip_qoix_plane_row_capacity()


def _info_words(info):
    return {k: int(v) for k, v in zip(qoix_ref_c.INFO_FIELDS, np.frombuffer(bytes(info), np.int32))}


@pytest.fixture(scope="module")
def expected():
    """the restatement's verdict and pixels per (reference, file, channels), computed once and shared"""
    cache = {}

    def get(f, ch, ref=qoiplane_ref_c):
        key = (ref.__name__, f, ch)
        if key not in cache:
            verdict, hd = ref.header(f)
            mismatch = verdict == ref.OK and ch != 0 and (ch < 3) != (hd["channels"] < 3)        # a channel count of the other family
            cache[key] = ((verdict, hd), None if mismatch else ref.load(f, ch), mismatch)
            if cache[key][1] is not None:
                cache[key][1][0].setflags(write=False)
        return cache[key]
    return get


def decode_batch(L, expected, files, ch, offsets=None, ref=qoiplane_ref_c):
    """one gamut_hip_qoix_decode_batch_device call -> (rc, statuses, infos, whole output allocation, offsets, expected allocation, wanted statuses, mask, exp)
    mask: False over the own bytes of a file that is refused on the device (it may leave anything there)"""
    n = len(files)
    exp = [expected(f, ch, ref) for f in files]
    sizes, want = [], []
    for f, ((verdict, hd), loaded, mismatch) in zip(files, exp):
        early = verdict == ref.OK and hd["compression"] == 1 and hd["orig"] > 255 * (len(f) - 29)            # refused on the host: writes nothing
        mismatch = mismatch and not early                                   # (the header's verdict comes first, the early refusal is part of it)
        want.append(_capi.ERR_INVALID_ARG if mismatch else 0 if loaded is not None else RC.get(verdict, _capi.ERR_DECODE))
        on_device = verdict == ref.OK and not early and not mismatch
        sizes.append((hd["width"] * hd["height"] * (ch or hd["channels"]), True) if on_device else (64, False))
    offs, pos = [], GUARD
    for k, (s, _) in enumerate(sizes):
        if offsets is None:
            pos += 1 + 2 * (k % 8)                                          # odd byte positions, every odd residue mod 16 among them
        else:
            pos = (pos + 15) // 16 * 16 + offsets[k]
        offs.append(pos)
        pos += s + GUARD
        pos += pos & 1
    expect = np.full(pos, 0xA5, np.uint8)
    mask = np.ones(pos, bool)
    for (_, loaded, _), o, (s, on_device) in zip(exp, offs, sizes):
        if loaded is not None:
            expect[o:o + s] = loaded[0].reshape(-1)
        elif on_device:
            mask[o:o + s] = False
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs])
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.QoixInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_qoix_decode_batch_device(ptrs, lens, n, ch, (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    return rc, list(st), info, out.cpu().numpy(), offs, expect, want, mask, exp


def check_batch(L, expected, files, ch, names=None, offsets=None, ref=qoiplane_ref_c):
    rc, st, info, got, offs, expect, want, mask, exp = decode_batch(L, expected, files, ch, offsets, ref)
    bad = [i for i, w in enumerate(want) if w]
    assert rc == (want[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for i in range(len(files)):
        assert st[i] == want[i], (i, names[i] if names else None, st[i], want[i])
        assert _info_words(info[i]) == exp[i][0][1], (i, names[i] if names else None)
    same = (got == expect) | ~mask
    if not same.all():                                                      # the WHOLE allocation, guards included
        first = int(np.flatnonzero(~same)[0])
        k = max([i for i in range(len(offs)) if offs[i] - GUARD <= first], default=0)
        assert False, ("channels", ch, "image", k, names[k] if names else None, "first difference at", first - offs[k],
                       "got", got[first:first + 8].tolist(), "want", expect[first:first + 8].tolist())
    return want


@pytest.mark.parametrize("ch", [0, 1, 2])
def test_every_named_case_in_one_batch(L, expected, ch):
    """the shapes at which the kernel can go wrong are among them: widths 1, 2, 3, 63, 64, 65; an LA starting at nibbles 58..63 of a
    group; DIFF chains of 64 and 65 ops; REPEAT2 of 258 and to-the-end runs across row and group ends at either nibble phase; ADIFF in
    front of REPEAT; a three-ADIFF chain; with ch 1 / 2 every 2-channel file at 1 channel and every 1-channel file at 2"""
    cases = K.small_cases()
    want = check_batch(L, expected, [f for _, f, _ in cases], ch, [n for n, _, _ in cases])
    assert [w == 0 for w in want] == [e == "ok" for _, _, e in cases]
    assert sum(w == _capi.ERR_DECODE for w in want) >= 20 and sum(w == 0 for w in want) >= 90


def _mixed():
    colour = [(n, f) for n, f, e in qoix_cases.small_cases() if len(f) < 2000][::5]
    grey = [(n, f) for n, f, e in K.small_cases() if len(f) < 2000][::3]
    files, names = [], []
    for k in range(max(len(colour), len(grey))):
        for part in (colour, grey):
            if k < len(part):
                names.append(part[k][0]); files.append(part[k][1])
    return files, names


def test_a_batch_that_mixes_colour_and_grey_files(L, expected):
    files, names = _mixed()
    want = check_batch(L, expected, files, 0, names)
    grey = [qoiplane_ref_c.header(f)[1]["channels"] < 3 for f in files]
    assert sum(w == 0 and g for w, g in zip(want, grey)) > 20 and sum(w == 0 and not g for w, g in zip(want, grey)) > 15
    for ch in (1, 4):                                                       # the other family: INVALID_ARG per file, nothing written, neighbours decoded
        want = check_batch(L, expected, files, ch, names)
        other = [(ch < 3) != g for g in grey]
        assert sum(w == _capi.ERR_INVALID_ARG for w in want) > 15 and sum(w == 0 for w in want) > 15
        assert all(o or w != _capi.ERR_INVALID_ARG for o, w in zip(other, want))


def test_the_same_batch_with_the_switch_off_is_unsupported_as_before(L, expected):
    files, names = _mixed()
    assert L.gamut_hip_qoix_set_plane(0) == 1
    try:
        want = check_batch(L, expected, files, 0, names, ref=qoix_ref_c)
        for f, w in zip(files, want):
            hd = qoix_ref_c.header(f)
            if hd[0] != qoix_ref_c.REFUSED and hd[1]["bitdepth"] == 8 and hd[1]["channels"] < 3:
                assert w == _capi.ERR_UNSUPPORTED
        assert sum(w == _capi.ERR_UNSUPPORTED for w in want) > 20 and sum(w == 0 for w in want) > 15
        out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        f = np.frombuffer(files[1], np.uint8)
        for ch in (1, 2):
            assert L.gamut_hip_qoix_decode_batch_device((C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), 1, ch, (C.c_int64 * 1)(0), out.data_ptr(), None, None, None) == _capi.ERR_INVALID_ARG
        assert (out.cpu().numpy() == 0xA5).all()
    finally:
        assert L.gamut_hip_qoix_set_plane(1) == 0


def test_refused_files_between_good_neighbours(L, expected):
    cases = K.small_cases()
    good = [(n, f) for n, f, e in cases if e == "ok" and len(f) < 2000][::7]
    refused = [(n, f) for n, f, e in cases if e != "ok"]
    assert len(refused) >= 20
    files, names = [], []
    for k, (n, f) in enumerate(refused):
        files += [good[k % len(good)][1], f]; names += [good[k % len(good)][0], n]
    files.append(good[0][1]); names.append(good[0][0])
    for ch in (0, 2):
        want = check_batch(L, expected, files, ch, names)
        assert [w != 0 for w in want] == [bool(k & 1) for k in range(len(files))]
    want = check_batch(L, expected, [f for _, f in refused], 1, [n for n, _ in refused])           # nothing but refused files
    assert all(want)


def test_stored_only_lz4_only_and_single_file_batches(L, expected):
    cases = [(n, f) for n, f, e in K.small_cases() if e == "ok" and len(f) < 3000]
    stored = [(n, f) for n, f in cases if f[16] == 0]
    lz = [(n, f) for n, f in cases if f[16] == 1]
    assert len(stored) > 40 and len(lz) > 10
    for part in (stored, lz, lz[:1], stored[:1]):
        for ch in (0, 1, 2):
            assert not any(check_batch(L, expected, [f for _, f in part], ch, [n for n, _ in part]))


def test_600_tiny_files_are_more_waves_than_one_round_of_the_grid(L, expected):
    rng = np.random.default_rng(11)
    files = []
    for k in range(600):
        w, h, ch = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(1, 3))
        files.append(P.encode(P.noisy(w, h, ch, k), lz4=k % 3 == 0))
    files[100] = P.stored(9, 9, P.DIRECT(5) + P.DIFF1(1) * 30, 1, closing=[4] * 8)          # one P1 file in the crowd
    want = check_batch(L, expected, files, 2)
    assert [i for i, w in enumerate(want) if w] == [100]
    assert not any(check_batch(L, expected, files[:100] + files[101:], 0))


def test_rows_at_the_lds_capacity_and_one_pixel_wider(L, expected, CAP):
    cases = K.row_capacity(CAP)
    assert sorted({qoiplane_ref_c.header(f)[1]["width"] for _, f, _ in cases}) == [CAP, CAP + 1]
    for ch in (0, 1, 2):
        assert not any(check_batch(L, expected, [f for _, f, _ in cases], ch, [n for n, _, _ in cases]))


def test_all_16_output_residues_in_one_batch(L, expected):
    """rows of 1, 5, 21, 65 and 300 pixels (shorter than a 16-byte piece, head and tail only, several pieces) x out_offset residues 0..15,
    1- and 2-channel output"""
    files, offsets = [], []
    for r in range(16):
        for w in (1, 5, 21, 65, 300)[r % 2::2] if r < 14 else (1, 5, 21, 65, 300):
            files.append(P.encode(P.noisy(w, 3, 1 + (r + w) % 2, r * 1000 + w)))
            offsets.append(r)
    assert {o for o in offsets} == set(range(16))
    assert not any(check_batch(L, expected, files, 1, offsets=offsets))
    assert not any(check_batch(L, expected, files, 2, offsets=offsets))


@pytest.mark.parametrize("device", [False, True])
def test_image_load(L, device):
    import oracle_lib as O
    from gamut_amd import image as gi
    d = {n: f for n, f, _ in K.small_cases()}
    d["lz4_offset_0_deviation_2"] = next(f for n, f, _ in K.small_cases() if n.startswith("lz4_offset_0_deviation_2"))
    names = {0: "l8", 3: "la8"}
    files = [d["geometry_65x3_1ch"], d["geometry_65x3_2ch_lz4"], d["alpha_ops_in_a_1_channel_file_asked_for_2"], d["header_par_and_dpi_bits_are_kept"],
             d["photo_like_201x149_l8_lz4"], d["alpha_ramp_77x31_stored"], P.stored(5, 4, P.LA(200, 128) + P.REPEAT2(9) + P.DIRECT(7), 2, par=1.5, dpi=300.0)]
    for f in files:
        ref, info = qoiplane_ref_c.load(f, 0)
        src = names[info["pixel_type"]]
        for flags in (0, gi.LOAD_GREYSCALE, gi.LOAD_ALPHA, gi.LOAD_RGB | gi.LOAD_NO_ALPHA, gi.LOAD_16BIT, gi.LOAD_GREYSCALE | gi.LOAD_NO_ALPHA, gi.LOAD_NO_PREMUL):
            im = gi.Image(device=device)
            assert im.loadFromMemory(f, flags), im.errorMessage
            want_type = L.gamut_apply_load_flags(O.PT[src], flags)
            assert (im.type, im.width, im.height, im.isDevice) == (want_type, info["width"], info["height"], device)
            if flags == 0:
                assert im.type == info["pixel_type"] and im.pitchInBytes == info["width"] * info["channels"]
            exp = O.scanlines_convert(src, ref.reshape(-1), O.PIXEL_TYPES[want_type], info["width"], info["height"]) if want_type != O.PT[src] else ref
            assert np.array_equal(np.asarray(im.pixels()).reshape(-1).view(np.uint8), np.asarray(exp).reshape(-1).view(np.uint8)), (src, flags)
            bits = np.array([im.pixelAspectRatio, im.dotsPerInchY], np.float32).view(np.int32)
            want_bits = np.array([info["pixel_aspect_ratio"], info["resolution_y"]], np.int32)
            assert np.array_equal(bits, want_bits) or (np.isnan(im.pixelAspectRatio) and info["pixel_aspect_ratio"] == 0x7fc01234), (bits, want_bits)
    for name in ("colorspace_2_with_2_channels_is_lap8_and_refused_by_the_sub_codec", "deviation_p1_stream_of_diffs_runs_out", "header_width_0",
                 "lz4_offset_0_deviation_2", "ten_bit_1_channel_is_still_unsupported"):
        im = gi.Image(device=device)
        assert not im.loadFromMemory(d[name]) and im.errorMessage == "Image decoding failed", name
    im = gi.Image(device=device)
    assert not im.loadFromMemory(files[0], gi.LOAD_RGB | gi.LOAD_GREYSCALE) and im.errorMessage == "Invalid image decoding flags"


def test_the_drop_in_against_the_restatement(L):
    cases = [(n, f, e) for n, f, e in K.small_cases() if len(f) < 3000][::3]
    assert sum(e == "ok" for _, _, e in cases) > 20 and sum(e != "ok" for _, _, e in cases) > 5
    for name, f, e in cases:
        buf = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            buf[64:] = np.frombuffer(f, np.uint8)
        info, typ = _capi.QoixInfo(), C.c_int(99)
        p = L.gamut_hip_qoix_lz4_decode(buf.ctypes.data + 64, len(f), C.byref(info), 0, C.byref(typ))
        ref = qoiplane_ref_c.load(f, 0)
        assert (p is not None) == (ref is not None) == (e == "ok"), name
        assert _info_words(info) == qoiplane_ref_c.header(f)[1], name
        if p is not None:
            got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (ref[0].size,)).copy()
            C.CDLL(None).free(C.c_void_p(p))
            assert np.array_equal(got, ref[0].reshape(-1)) and typ.value == ref[1]["pixel_type"] and typ.value in (0, 3), name
        else:
            assert typ.value == -1


def test_plane_kernel_timing_getter(L):
    """-1 unless GAMUT_HIP_QOIX_TIMING=1 was set when the library first decoded; the two earlier getters do not include the plane kernel"""
    import os
    f = np.frombuffer(K.small_cases()[0][1], np.uint8)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.gamut_hip_qoix_decode_batch_device((C.c_void_p * 1)(f.ctypes.data), (C.c_size_t * 1)(f.size), 1, 0, (C.c_int64 * 1)(0), out.data_ptr(), None, None, None) == 0
    a, b, t, p = L.gamut_hip_qoix_last_decode_stage_ms(0), L.gamut_hip_qoix_last_decode_stage_ms(1), L.gamut_hip_qoix_last_decode_kernel_ms(), L.gamut_hip_qoix_last_plane_kernel_ms()
    if os.environ.get("GAMUT_HIP_QOIX_TIMING") == "1":
        assert a >= 0 and b >= 0 and p > 0 and abs(t - (a + b)) < 1e-3
    else:
        assert (a, b, t, p) == (-1.0, -1.0, -1.0, -1.0)
