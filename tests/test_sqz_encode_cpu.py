"""SQZ encode without a GPU: the two restatements of the reference's encoder (tests/c/sqz_ref.c with its forward steps exported by
tests/c/sqz_ref_fwd.c, and tests/sqz_encode_ref.py, written separately from the D text) against each other, coefficients and files;
the library's host writer gamut_hip_sqz_encode_coeffs against both, byte for byte; the embedded property; the decode round trip;
hand-made coefficient buffers; the budget arithmetic; the ABI layout, the level clamp and the refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sqz_cases
import sqz_encode_ref as P
import sqz_ref_c as R
import sqz_ref_fwd_c as F
from gamut_amd import _capi
from gamut_amd import image as gi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUDGETS = (7, 8, 9, 16, 40, 100, 300, 1000, None)
GEOMETRIES = ((16, 16, 1), (17, 16, 1), (16, 17, 1), (19, 23, 1), (31, 33, 1), (32, 33, 2), (47, 32, 2), (64, 40, 2), (64, 40, 3), (128, 72, 4), (256, 256, 5), (300, 130, 5))


@pytest.fixture(scope="module")
def L():
    return _capi.lib()


def desc(w, h, mode, levels, scan, ss, budget):
    d = _capi.SqzEncodeDesc()
    d.width, d.height, d.color_mode, d.levels, d.scan_order, d.subsampling, d.budget = w, h, mode, levels, scan, ss, budget
    return d


def lossless_budget(w, h, mode):
    return 64 + w * h * (1 if mode == 0 else 3) * 3                         # what sqz_ref_c.encode takes as "enough"


def host_encode(L, co, w, h, mode, levels, scan, ss, budget):
    """-> (rc, file bytes); the destination has exactly `budget` bytes in front of a sentinel, and is dirty before the call"""
    co = np.ascontiguousarray(co, np.int16)
    before = co.copy()
    dst = np.full(budget + 32, 0xC3, np.uint8)
    n = C.c_int64(-5)
    d = desc(w, h, mode, levels, scan, ss, budget)
    rc = L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, C.byref(d), dst.ctypes.data, C.byref(n))
    assert (dst[budget:] == 0xC3).all() and np.array_equal(co, before)
    assert d.levels == levels                                               # the caller's desc is not written to
    if rc:
        assert n.value == 0
        return rc, None
    assert 7 <= n.value <= budget and (dst[n.value:budget] == 0).all()     # cleared first, as saveSQZ clears it
    return rc, dst[:n.value].tobytes()


def host_decode(L, f):
    info = _capi.SqzInfo()
    buf = np.frombuffer(f + b"\0", np.uint8)
    assert L.gamut_hip_sqz_read_header(buf.ctypes.data, len(f), C.byref(info)) == 0
    out = np.zeros(info.planes * info.width * info.height, np.int16)
    assert L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, len(f), out.ctypes.data, out.size, C.byref(info)) == 0
    return out


def check_case(L, px, mode, levels, scan, ss, budgets, python=True):
    h, w = px.shape[:2]
    co = F.analyze(px, mode, levels)
    if python:
        assert np.array_equal(P.analyze(px, mode, P.clamp_levels(w, h, levels)), co)      # the two readings, coefficients
    for b in budgets:
        budget = lossless_budget(w, h, mode) if b is None else b
        want = R.encode(px, mode, levels, scan, ss, budget)
        if python:
            assert P.encode(px, mode, levels, scan, ss, budget) == want                   # the two readings, files
        rc, got = host_encode(L, co, w, h, mode, levels, scan, ss, budget)
        assert rc == 0 and got == want, (w, h, mode, levels, scan, ss, b)
        if b is None:
            assert len(got) < budget
        assert np.array_equal(host_decode(L, got), R.coeffs(want)[0])                     # and back


@pytest.mark.parametrize("mode", range(4))
def test_every_mode_scan_and_subsampling_at_16x16(L, mode):
    px = sqz_cases.picture(16, 16, 1 if mode == 0 else 3, 40 + mode)
    for scan in range(4):
        for ss in (0, 1):
            check_case(L, px, mode, 1, scan, ss, BUDGETS)


@pytest.mark.parametrize("w,h,levels", GEOMETRIES)
def test_geometries(L, w, h, levels):
    k = GEOMETRIES.index((w, h, levels))
    for mode in ((0, 1, 2, 3) if w * h < 2000 else (k % 4, 2)):
        px = sqz_cases.picture(w, h, 1 if mode == 0 else 3, 200 + k)
        check_case(L, px, mode, levels, (k + mode) % 4, k & 1, (100, 1000, None) if w * h < 2000 else (1000, None))


def test_a_budget_of_six_bytes_is_refused(L):
    co = F.analyze(sqz_cases.picture(16, 16, 1, 1), 0, 1)
    for budget in (0, 1, 5, 6, -3):
        d = desc(16, 16, 0, 1, 0, 0, budget)
        dst = np.full(64, 0xC3, np.uint8)
        n = C.c_int64(9)
        assert L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, C.byref(d), dst.ctypes.data + 16, C.byref(n)) == _capi.ERR_INVALID_ARG
        assert n.value == 0 and (dst == 0xC3).all()
    assert P.encode_coeffs(co, 16, 16, 0, 1, 0, 0, 6) is None               # SQZ_BUFFER_TOO_SMALL: eob behind the header's last bit
    assert host_encode(L, co, 16, 16, 0, 1, 0, 0, 7)[0] == 0


@pytest.mark.parametrize("which", (0, 1))
def test_every_budget_gives_the_prefix_of_the_lossless_file(L, which):
    (w, h, mode, scan, ss, seed) = ((16, 16, R.GREY, R.HILBERT, 0, 31), (16, 17, R.OKLAB, R.SNAKE, 1, 32))[which]
    px = sqz_cases.picture(w, h, 1 if mode == 0 else 3, seed)
    assert R.encode(px, mode, 1, scan, ss) == sqz_cases.prefix_files()[which]
    co = F.analyze(px, mode, 1)
    full = host_encode(L, co, w, h, mode, 1, scan, ss, lossless_budget(w, h, mode))[1]
    assert full == sqz_cases.prefix_files()[which] and full == P.encode(px, mode, 1, scan, ss)
    for b in range(7, len(full) + 1):
        assert host_encode(L, co, w, h, mode, 1, scan, ss, b)[1] == full[:b], b
    for b in range(7, len(full) + 1, 13):
        assert P.encode_coeffs(co, w, h, mode, 1, scan, ss, b) == full[:b], b


def sm(v):
    """two's complement -> sign-magnitude as SQZ_dwt_convert_to_sign_magnitude stores it (a short)"""
    v = np.asarray(v, np.int64)
    return np.where(v < 0, (-2 * v) | 1, 2 * v).astype(np.int16)


def check_hand(L, co, w, h, levels=1, scan=0, budget=None):
    """library == Python reading, and the file decodes to the coefficients (lossless budgets only)"""
    budget = budget or 64 + 3 * co.size
    rc, got = host_encode(L, co, w, h, 0, levels, scan, 0, budget)
    assert rc == 0 and got == P.encode_coeffs(co, w, h, 0, levels, scan, 0, budget)
    return got


def test_hand_made_an_all_zero_band_and_one_coefficient_on_plane_14(L):
    co = np.zeros(16 * 16, np.int16)
    f = check_hand(L, co, 16, 16)
    assert np.array_equal(host_decode(L, f), co)
    assert f[6:] == bytes([0, 0])                                           # four bands, each nothing but a 4-bit max_bitplane of 0
    for value in (8192, -8192, 16383, -16383, 12345):
        co = np.zeros(16 * 16, np.int16)
        co[8 + 32 * 3 + 2] = sm(value)                                      # band 1 (horizontal high, vertical low): columns 8.., its row 3 is row 6
        f = check_hand(L, co, 16, 16)
        assert f[6] == 0x0E                                                 # LL's nibble 0 in round 0, then this band's 14 opens round 1
        assert np.array_equal(host_decode(L, f), co)


def test_hand_made_a_run_longer_than_65535(L):
    """600 x 512 grey, one level: the LL band has 300 x 256 = 76800 coefficients; one of them, near the end of the raster scan, is not
    zero, so the first run of its top bit plane is 70001: cost = SQZ_ilog2(run) - 1 = 16, the widest ONE-part code (32 bits, and bit 16 of
    the run is the implied top bit that SQZ_interleave_u16_to_u32 masks away).  SQZ_encode_write_wdr_run's two-part code starts at
    cost 17, a run of 131072: 1200 x 512 has an LL band of 153600, and a run of 150001 takes it."""
    for w, h, at, cut in ((600, 512, 70000, 9), (1200, 512, 150000, 9)):
        co = np.zeros(w * h, np.int16)
        y, x = divmod(at, w // 2)
        co[(2 * y) * w + x] = sm(-5)
        f = check_hand(L, co, w, h)
        assert np.array_equal(host_decode(L, f), co)
        bits = "".join("{:08b}".format(b) for b in f[6:])
        assert bits[:4] == "0011" and bits[4] == "1"                        # the LL band's max_bitplane 3, then the first coefficient's sign
        assert bits[5:].startswith("".join("0" + c for c in bin(at + 1)[3:]) + "1")
        g = check_hand(L, co, w, h, budget=cut)                             # cut inside the run's code (inside its second part for the long one)
        assert g == f[:cut]


def test_hand_made_coefficients_of_magnitude_16384_and_more(L):
    """a sign-magnitude value of 32768 and more is a negative short.  SQZ_dwt_get_max compares shorts: beside one value that is not
    negative such values never are the maximum, the band's top bit plane comes from the others, and everything is defined -- reproduced.
    A band of nothing but such values has a negative maximum, SQZ_ilog2 of it is 32 and the reference shifts 1u by 32: refused."""
    co = np.zeros(16 * 16, np.int16)
    co[0] = sm(16384 + 77)                                                  # 32922 as a ushort: a negative short
    co[1] = sm(-300)
    co[16 * 2 + 5] = sm(20000)
    assert co[0] < 0 and co[16 * 2 + 5] < 0
    f = check_hand(L, co, 16, 16)
    assert (f[6] >> 4) == 9                                                 # ilog2(601 >> 1): the large values are not seen
    back = host_decode(L, f)
    assert back[1] == co[1] and back[0] == (co[0] & 0x3FF) != 0 and back[16 * 2 + 5] == (co[16 * 2 + 5] & 0x3FF) != 0   # their bits from the band's top plane down
    co[:] = 0
    ll = np.arange(8)[:, None] * 32 + np.arange(8)[None, :]                 # the 8 x 8 LL band of a 16 x 16 image, one level
    co[ll.reshape(-1)] = sm(-16384)
    rc, _ = host_encode(L, co, 16, 16, 0, 1, 0, 0, 400)
    assert rc == _capi.ERR_INVALID_ARG and b"1u << 32" in L.gamut_hip_last_error()
    with pytest.raises(P.Undefined):
        P.encode_coeffs(co, 16, 16, 0, 1, 0, 0, 400)


def test_budget_from_flags(L):
    values = [0] + [v << 5 for v in range(0x20, 0x80, 8)] + [0xff << 5, 1 << 5]
    assert values[:14] == [gi.ENCODE_SQZ_QUALITY_DEFAULT, gi.ENCODE_SQZ_QUALITY_BPP1_0, gi.ENCODE_SQZ_QUALITY_BPP1_25, gi.ENCODE_SQZ_QUALITY_BPP1_5,
                           gi.ENCODE_SQZ_QUALITY_BPP1_75, gi.ENCODE_SQZ_QUALITY_BPP2_0, gi.ENCODE_SQZ_QUALITY_BPP2_25, gi.ENCODE_SQZ_QUALITY_BPP2_5,
                           gi.ENCODE_SQZ_QUALITY_BPP2_75, gi.ENCODE_SQZ_QUALITY_BPP3_0, gi.ENCODE_SQZ_QUALITY_BPP3_25, gi.ENCODE_SQZ_QUALITY_BPP3_5,
                           gi.ENCODE_SQZ_QUALITY_BPP3_75, gi.ENCODE_SQZ_QUALITY_MAX]
    header = open(os.path.join(ROOT, "include", "gamut_image.h")).read()
    for name in ("DEFAULT", "BPP1_0", "BPP1_25", "BPP1_5", "BPP1_75", "BPP2_0", "BPP2_25", "BPP2_5", "BPP2_75", "BPP3_0", "BPP3_25", "BPP3_5", "BPP3_75", "MAX"):
        m = re.search(r"GAMUT_ENCODE_SQZ_QUALITY_%s = (0x[0-9a-f]+ << 5|0)\b" % name, header)
        assert m and eval(m.group(1)) == getattr(gi, "ENCODE_SQZ_QUALITY_" + name)
    for w, h in ((8, 8), (1920, 1080), (65535, 65535)):
        for flags in values:
            for extra in (0, 31, 1 << 13, 0x10000):                        # bits outside the field change nothing
                bpp8 = (flags >> 5) & 0xff or 0x50
                bpp = float(np.float32(bpp8) / np.float32(32.0))
                want = 6 + int(float(w) * h * bpp / 8.0)
                assert L.gamut_hip_sqz_budget_from_flags(w, h, flags | extra) == want, (w, h, flags, extra)
    assert L.gamut_hip_sqz_budget_from_flags(1920, 1080, 0) == 6 + 648000


def test_struct_layout(tmp_path):
    """gamut_hip_sqz_encode_desc three ways: the C compiler's layout (tests/c/sqz_encode_abi_layout.c), the static assert in
    bindings/gamut_hip.d and the ctypes mirror"""
    exe = str(tmp_path / "sqz_encode_abi_layout")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "sqz_encode_abi_layout.c"), "-o", exe])
    dsrc = open(os.path.join(ROOT, "bindings", "gamut_hip.d")).read()
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(lines) == 1
    f = lines[0].split()
    name, c_size, c_fields = f[0], int(f[1]), {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[2:]}
    assert name == "gamut_hip_sqz_encode_desc" and c_size == 32
    m = re.search(r"static assert\((\d+) == %s\.sizeof(.*?)\);" % name, dsrc, flags=re.S)
    assert m and int(m.group(1)) == c_size
    assert {n: int(v) for v, n in re.findall(r"(\d+) == %s\.(\w+)\.offsetof" % name, m.group(2))} == c_fields
    mirror = _capi.SqzEncodeDesc
    assert C.sizeof(mirror) == c_size and {n: getattr(mirror, n).offset for n, _ in mirror._fields_} == c_fields
    assert list(c_fields) == ["width", "height", "color_mode", "levels", "scan_order", "subsampling", "budget"]
    for entry in ("budget_from_flags", "analyze_batch_device", "dwt_batch_device", "encode_coeffs", "encode_batch_device", "write_to_mem", "last_encode_stage_ms"):
        assert "gamut_hip_sqz_" + entry + "(" in dsrc and "gamut_hip_sqz_" + entry in _capi.SIGNATURES


def test_the_level_clamp_and_the_refusals(L):
    px = sqz_cases.picture(16, 16, 1, 3)
    co = F.analyze(px, 0, 7)                                                # clamped to 2 by the binding, as every reading clamps
    rc, f = host_encode(L, co, 16, 16, 0, 7, 1, 0, 2000)
    assert rc == 0 and f == R.encode(px, 0, 7, 1, 0, 2000) == R.encode(px, 0, 2, 1, 0, 2000)
    assert R.header(f)[1]["levels"] == 2 and ((f[5] >> 3) & 7) == 1
    assert P.encode(px, 0, 7, 1, 0, 2000) == f
    big = np.zeros(8, np.int16)
    for (w, h, mode, levels, scan) in ((7, 16, 0, 1, 0), (16, 7, 0, 1, 0), (65536, 16, 0, 1, 0), (16, 65536, 0, 1, 0), (16, 16, 4, 1, 0), (16, 16, -1, 1, 0),
                                       (16, 16, 0, 1, 4), (16, 16, 0, 1, -1), (16, 16, 0, 0, 0), (16, 16, 0, 9, 0)):
        d = desc(w, h, mode, levels, scan, 0, 100)
        dst = np.full(128, 0xC3, np.uint8)
        n = C.c_int64(3)
        assert L.gamut_hip_sqz_encode_coeffs(big.ctypes.data, C.byref(d), dst.ctypes.data, C.byref(n)) == _capi.ERR_INVALID_ARG, (w, h, mode, levels, scan)
        assert n.value == 0 and (dst == 0xC3).all()
    d = desc(16, 16, 0, 1, 0, 0, 100)
    n = C.c_int64(0)
    dst = np.zeros(100, np.uint8)
    assert L.gamut_hip_sqz_encode_coeffs(None, C.byref(d), dst.ctypes.data, C.byref(n)) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, None, dst.ctypes.data, C.byref(n)) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, C.byref(d), None, C.byref(n)) == _capi.ERR_INVALID_ARG
    assert L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, C.byref(d), dst.ctypes.data, None) == _capi.ERR_INVALID_ARG


def test_the_image_entries_refuse_without_an_image():
    Li = gi.lib()
    n = C.c_size_t(5)
    assert not Li.gamut_image_save_sqz_to_memory(None, 0, C.byref(n)) and n.value == 0
    assert not Li.gamut_image_save_sqz_to_file(None, b"/nonexistent/x.sqz", 0)
    assert gi.FORMAT_SQZ == 9
