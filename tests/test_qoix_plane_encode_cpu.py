"""QOI-Plane encode without a device.  The serial C restatement of qoiplane_encode (tests/c/qoiplane_write_ref.c), which is the oracle of
the GPU tests, is checked against things that are not itself: the Python restatement (tests/qoiplane_gen.py encode), both QOI-Plane
decoders, and op streams worked out by hand.  Then the bound with the QOI-Plane switch on and off, argument validation, the loud failure
when there is no GPU, the Image mirror's refusals, the boundary cases of the container choice and the coverage of the GPU suite's images.
The switch is process-wide: every test runs inside a fixture that restores the value it found."""
import ctypes as C

import numpy as np
import pytest

import qoiplane_encode_cases as cases
import qoiplane_gen as P
import qoiplane_ref_c
import qoiplane_write_ref_c as ref
import qoix_gen
from gamut_amd import _capi
from gamut_amd import image as gi


@pytest.fixture(scope="module")
def L():
    return _capi.lib()


@pytest.fixture(autouse=True)
def plane_on(L):
    prev = L.gamut_hip_qoix_set_plane(1)
    yield
    L.gamut_hip_qoix_set_plane(prev)


@pytest.fixture(scope="module")
def S(L):
    s = L.gamut_hip_qoix_plane_encode_segment()
    assert s > 0 and s % 64 == 0
    return s


def test_the_two_restatements_agree_on_every_named_case(S):
    items = cases.named(S)
    assert len(items) > 150 and len({n for n, _ in items}) == len(items)
    for k, (name, im) in enumerate(items):
        kw = dict(colorspace=k % 2, par=1.5, dpi=300.0)
        assert ref.stored(im, **kw) == P.encode(im, **kw), name


def test_the_two_restatements_agree_on_random_small_images():
    rng = np.random.default_rng(2024)
    worst = 0
    for k in range(3000):
        w, h, ch = int(rng.integers(1, 24)), int(rng.integers(1, 9)), 1 + k % 2
        kind = k % 5
        if kind == 0:
            im = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        elif kind == 1:
            im = P.few_levels(w, h, ch, k, 2 + k % 4)
        elif kind == 2:                                                     # small steps with wraps: DIFF1 / DIFF2 / ADIFF
            im = (np.cumsum(rng.integers(-9, 10, (h, w, ch)), axis=1) + rng.integers(0, 256)).astype(np.uint8)
        elif kind == 3:
            im = P.flat_image(w, h, ch, k)
        else:
            im = np.repeat(rng.integers(0, 256, (h, (w + 2) // 3, ch), dtype=np.uint8), 3, axis=1)[:, :w]
        f = ref.stored(im)
        assert f == P.encode(im), (k, w, h, ch)
        assert len(f) - 25 <= ref.datalen_max(w, h, ch)
        worst = max(worst, len(f) - 25 - ref.datalen_max(w, h, ch))
    assert worst <= 0


def test_hand_worked_streams():
    for name, im, stream in cases.HAND_WORKED:
        h, w, ch = im.shape
        for mode in (0, 1):
            f = ref.encode(im, mode)
            assert f[16] == 0 and f[25:].hex() == stream, name              # an LZ4 block of so few bytes is no shorter: stored
            assert f[:25] == qoix_gen.header(w, h, ch), name
        assert P.pack(P.encode_nibbles(im)).hex() == stream, name


def test_every_case_file_decodes_to_its_source(S):
    packed = 0
    for name, im in cases.named(S):
        for mode in (0, 1):
            f = ref.encode(im, mode)
            packed += f[16]
            got = qoiplane_ref_c.load(f)
            assert got is not None and np.array_equal(np.asarray(got[0]).reshape(im.shape), im), name
    assert packed >= 20


def test_the_suite_holds_every_op_kind_and_both_parities(S):
    kinds, after_adiff, parities = set(), set(), set()
    for name, im in cases.named(S):
        h, w, ch = im.shape
        ks, nibbles = cases.parse_ops(ref.stored(im)[25:], w * h, ch)
        kinds |= set(ks)
        after_adiff |= {b for a, b in zip(ks, ks[1:]) if a == "ADIFF"}
        parities.add(nibbles & 1)
        assert len(ref.stored(im)) - 25 == (nibbles + 10) // 2, name        # nine closing nibbles, one more for an even count in front
    assert kinds == {"DIFF1", "DIFF2", "DIRECT", "ADIFF", "LA", "REPEAT1", "REPEAT2"}
    assert after_adiff == {"DIFF1", "DIFF2", "DIRECT"}                      # ADIFF is followed by a luminance op, never by anything else
    assert parities == {0, 1}


def test_shared_byte_cases_have_odd_segment_boundaries(S):
    """the nibbles of a one-row image's first S pixels are those of the image cut there, but for the cut image's closing nibbles"""
    for name, im in cases.shared_bytes(S):
        assert im.shape[0] == 1
        _, n = cases.parse_ops(ref.stored(im[:, :S])[25:], S, im.shape[2])
        assert (n & 1) == (0 if name.startswith("even") else 1), name


def desc(w, h, ch=1, cs=0, mode=0):
    return _capi.QoixDesc(w, h, ch, cs, mode, 1.0, 96.0)


def formula(w, h, ch):
    datalen_max = (w * h * (3 if ch == 1 else 6) + 10) // 2
    return 25 + 4 + datalen_max + datalen_max // 255 + 16


def test_encode_bound_with_the_switch_on(L):
    b = lambda *a: L.gamut_hip_qoix_encode_bound(C.byref(desc(*a)))
    for w, h in ((1, 1), (3, 7), (1920, 1080), (65, 2), (5, 5)):
        for ch in (1, 2):
            assert b(w, h, ch) == formula(w, h, ch) == ref.bound(w, h, ch)
            assert ref.datalen_max(w, h, ch) == (w * h * (3 if ch == 1 else 6) + 10) // 2
    for cs in (0, 1, 2):
        assert b(7, 3, 2, cs) == formula(7, 3, 2) and b(7, 3, 1, cs, 1) == formula(7, 3, 1)
    assert b(5, 5, 2, 3) == -1 and b(5, 5, 1, -1) == -1 and b(5, 5, 1, 0, 2) == -1
    assert b(0, 5) == -1 and b(5, 0) == -1 and b(-1, 5) == -1 and b(5, -1) == -1
    assert b(5, 5, 0) == -1 and b(5, 5, 5) == -1
    assert b(5, 5, 3) == 29 + 104 + 0 + 16 and b(5, 5, 4, 2) == 29 + 129 + 0 + 16            # colour is what it was
    w = 20000                                                               # height >= 400000000 / width
    for ch in (1, 2):
        assert b(w, 400000000 // w, ch) == -1 and ref.bound(w, 400000000 // w, ch) == -1
        assert b(7, 57142857, ch) == -1 and b(7, 57142856, ch) == (formula(7, 57142856, ch) if ch == 1 else -1)
    assert b(w, 400000000 // w - 1, 1) == formula(w, 400000000 // w - 1, 1) == ref.bound(w, 400000000 // w - 1, 1)
    # deviation G2: w * h * 6 above 2^31 - 1 is refused, 357913941 pixels are the most
    assert 357913941 * 6 <= 2 ** 31 - 1 < 357913942 * 6
    assert b(1, 357913941, 2) == formula(1, 357913941, 2) == ref.bound(1, 357913941, 2) < 2 ** 31
    assert b(1, 357913942, 2) == -1 == ref.bound(1, 357913942, 2)
    assert b(1, 357913942, 1) == formula(1, 357913942, 1) and b(1, 399999999, 1) == formula(1, 399999999, 1) < 2 ** 31
    assert L.gamut_hip_qoix_plane_encode_segment() % 64 == 0


def test_worst_case_images_reach_datalen_max_and_overrun_the_reference_allocation():
    """deviation G1: 1 x n images alternating 100 / 200 take the worst op at every pixel"""
    over = {1: 0, 2: 0}
    for n in range(1, 40):
        for ch in (1, 2):
            im = np.zeros((1, n, ch), np.uint8)
            im[0, :, 0] = [100 + 100 * (k & 1) for k in range(n)]
            if ch == 2:
                im[0, :, 1] = [200 - 100 * (k & 1) for k in range(n)]       # alpha steps of -55, then -100 and +100: an LA at every pixel
            f = ref.stored(im)
            assert len(f) - 25 == ref.datalen_max(n, 1, ch), (n, ch)
            assert f == P.encode(im)
            over[ch] += len(f) > ref.reference_alloc(n, 1, ch)
            assert len(f) - ref.reference_alloc(n, 1, ch) == (1 if (n * (3 if ch == 1 else 6)) % 2 == 0 else 0)
    assert over == {1: 19, 2: 39}


def test_encode_bound_with_the_switch_off_is_what_it_was(L):
    assert L.gamut_hip_qoix_set_plane(0) == 1
    b = lambda *a: L.gamut_hip_qoix_encode_bound(C.byref(desc(*a)))
    assert b(5, 5, 1) == -1 and b(5, 5, 2) == -1 and b(5, 5, 2, 2) == -1 and b(1920, 1080, 1, 0, 1) == -1
    assert b(5, 5, 3) == 29 + 104 + 0 + 16
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 8, C.byref(desc(4, 4, 2)), C.byref(n)) and n.value == -1
    assert b"invalid arguments" in L.gamut_hip_last_error()
    for type_, bpp in ((0, 1), (3, 2), (6, 2)):                              # l8, la8, lap8: refused before any device is asked for
        v = gi.Image()
        assert v.createView(np.zeros((3, 4 * bpp), np.uint8), 4, 3, type_, 4 * bpp)
        assert v.save_qoix_to_memory() is None and v.isValid and v.errorMessage is None


def test_argument_validation_without_device(L):
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    assert not L.gamut_hip_qoix_write_to_mem(None, 4, C.byref(desc(4, 4)), C.byref(n))
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4, None, C.byref(n))
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4, C.byref(desc(4, 4)), None)
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4, C.byref(desc(4, 4, 1, 3)), C.byref(n))
    assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4, C.byref(desc(1, 357913942, 2)), C.byref(n))
    assert b"invalid arguments" in L.gamut_hip_last_error() and n.value == -1
    assert L.gamut_hip_qoix_encode_batch_device(None, None, None, 1, None, None, None, None, None) == _capi.ERR_INVALID_ARG
    for stage in (-1, 3, 7):
        assert L.gamut_hip_qoix_last_plane_encode_stage_ms(stage) == -1.0
    for stage in (0, 1, 2):                                                 # nothing was encoded by this thread with timing on
        assert L.gamut_hip_qoix_last_plane_encode_stage_ms(stage) == -1.0


def test_no_device_is_a_loud_failure(L):
    if L.gamut_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    px = np.zeros(64, np.uint8); n = C.c_int(-1)
    for ch in (1, 2):
        assert not L.gamut_hip_qoix_write_to_mem(px.ctypes.data, 4 * ch, C.byref(desc(4, 4, ch)), C.byref(n)) and n.value == -1
        d = (_capi.QoixDesc * 1)(desc(4, 4, ch))
        src = (C.c_void_p * 1)(px.ctypes.data); pitch = (C.c_int64 * 1)(4 * ch); off = (C.c_int64 * 1)(0); ln = (C.c_int64 * 1)(-1)
        out = np.full(256, 0xA5, np.uint8); st = (C.c_int * 1)(-7)
        assert L.gamut_hip_qoix_encode_batch_device(src, pitch, d, 1, off, out.ctypes.data, ln, st, None) == _capi.ERR_NO_DEVICE
        assert (out == 0xA5).all() and ln[0] == -1 and st[0] == -7
    for type_, bpp in ((0, 1), (3, 2), (6, 2)):                              # accepted types, and no device to encode them
        img = gi.Image()
        assert img.createView(np.zeros((4, 4 * bpp), np.uint8), 4, 4, type_, 4 * bpp)
        assert img.save_qoix_to_memory() is None
        assert img.isValid and img.errorMessage is None


def test_image_save_refusals_that_need_no_device(L, tmp_path):
    img = gi.Image()
    assert img.save_qoix_to_memory() is None and img.errorMessage == "Uninitialized image"
    for type_ in (0, 3, 6):
        nodata = gi.Image()
        assert nodata.createWithNoData(4, 3, type_) and nodata.save_qoix_to_memory() is None and nodata.isValid
    for type_, bpp in ((1, 2), (4, 4), (7, 4), (2, 4)):                      # l16, la16, lap16, lf32: still no codec
        v = gi.Image()
        assert v.createView(np.zeros((3, 4 * bpp), np.uint8), 4, 3, type_, 4 * bpp)
        assert v.save_qoix_to_memory() is None and not v.saveQOIXToFile(tmp_path / "no.qoix") and not (tmp_path / "no.qoix").exists()
        assert v.isValid and v.type == type_ and v.errorMessage is None
    grey = gi.Image()
    assert grey.createView(np.zeros((3, 4), np.uint8), 4, 3, 0, 4)
    assert grey.save_to_memory(gi.FORMAT_QOIX) is None                      # the generic entry does not dispatch QOIX


def test_boundary_cases_are_boundary_cases():
    """lz4Size + 4 - datalen of the committed seeds: -1 packs, 0 and +1 do not"""
    items, diffs = cases.boundary_images(), cases.boundary_diffs()
    assert {(d, im.shape[2]) for (_, im), d in zip(items, diffs)} == {(d, ch) for d in (-1, 0, 1) for ch in (1, 2)}
    for (name, im), diff in zip(items, diffs):
        f, got = ref.encode_ex(im, 0)
        assert got == diff, name
        assert f[16] == (1 if diff < 0 else 0), name
        stored = ref.encode(im, 1)
        assert (len(f) == len(stored) + diff) if diff < 0 else (f == stored), name
        if diff < 0:
            assert f[25:29] == (len(stored) - 25).to_bytes(4, "big") and f[:16] + b"\0" + f[17:25] == stored[:25]
    name, big = cases.byu32_image()
    assert big.shape == (184, 256, 1) and len(ref.encode(big, 1)) - 25 >= 65547       # LZ4's byU32 form
