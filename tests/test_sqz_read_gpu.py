"""The SQZ device reader (gamut_hip_sqz_read_batch_device) against the unchanged host front end (gamut_hip_sqz_decode_coeffs), and on
the named cases against the serial C restatement (tests/c/sqz_ref.c) too: every coefficient, bit for bit.  Each file sits at the end of
its host buffer; the coefficient allocation is filled with 0x5A5A, every image's coefficients lie at an odd element offset between
guards, and the allocation is compared whole.  Expected values are computed once per file and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import sqz_cases
import sqz_read_model as M
import sqz_ref_c as R
from gamut_amd import _capi

pytestmark = pytest.mark.gpu
GUARD = 512                                                                 # int16 elements
FILL = 0x5A5A
_cache = {}


@pytest.fixture(scope="module")
def L():
    lib = _capi.lib()
    _capi.check(lib.gamut_hip_init(0))
    return lib


def _info_words(info):
    return {k: int(v) for k, v in zip(R.INFO_FIELDS, np.frombuffer(bytes(info), np.int32))}


def expected(f):
    """the host front end's (status, info, coefficients or None) per file"""
    if f not in _cache:
        L = _capi.lib()
        buf = np.frombuffer(f + b"\0", np.uint8)
        info = _capi.SqzInfo()
        rc = L.gamut_hip_sqz_read_header(buf.ctypes.data, len(f), C.byref(info))
        co = None
        if rc == 0:
            co = np.zeros(info.width * info.height * info.planes, np.int16)
            assert L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, len(f), co.ctypes.data, co.size, None) == 0
            co.setflags(write=False)
        _cache[f] = (rc, _info_words(info), co)
    return _cache[f]


def host_buffers(files):
    bufs = []
    for f in files:                                                         # each file at the END of its host buffer: nothing readable behind it
        b = np.zeros(len(f) + 64, np.uint8)
        if len(f):
            b[64:] = np.frombuffer(f, np.uint8)
        bufs.append(b)
    n = len(files)
    return bufs, (C.c_void_p * n)(*[b.ctypes.data + 64 for b in bufs]), (C.c_size_t * n)(*[len(f) for f in files])


def read_files(L, files, names=None, stream=None):
    """one gamut_hip_sqz_read_batch_device call, everything compared; -> (the statuses wanted, the coefficient allocation as read)"""
    n = len(files)
    exp = [expected(f) for f in files]
    want = [rc for rc, _, _ in exp]
    offs, pos = [], GUARD
    for k, (_, _, co) in enumerate(exp):
        pos += 1 + 2 * (k % 4)                                              # odd element offsets
        offs.append(pos)
        pos += (co.size if co is not None else 16) + GUARD
    expect = np.full(pos, FILL, np.uint16).view(np.int16)
    for (_, _, co), o in zip(exp, offs):
        if co is not None:
            expect[o:o + co.size] = co
    bufs, ptrs, lens = host_buffers(files)
    dco = torch.from_numpy(np.full(pos, FILL, np.uint16).view(np.int16)).cuda()
    info = (_capi.SqzInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_read_batch_device(ptrs, lens, n, dco.data_ptr(), (C.c_int64 * n)(*offs), info, st, stream)
    torch.cuda.synchronize()
    bad = [i for i, w in enumerate(want) if w]
    assert rc == (want[bad[0]] if bad else 0), (rc, L.gamut_hip_last_error())
    if bad:
        assert L.gamut_hip_last_error().startswith(b"image %d:" % bad[0]), L.gamut_hip_last_error()
    for i in range(n):
        assert st[i] == want[i], (i, names[i] if names else None, st[i], want[i])
        assert _info_words(info[i]) == exp[i][1], (i, names[i] if names else None)
    got = dco.cpu().numpy()
    if not np.array_equal(got, expect):                                     # the WHOLE allocation, guards included
        first = int(np.flatnonzero(got != expect)[0])
        k = max([i for i in range(n) if offs[i] - GUARD <= first], default=0)
        assert False, ("image", k, names[k] if names else None, len(files[k]), "bytes; first difference at", first - offs[k], "got", got[first:first + 8].tolist(),
                       "want", expect[first:first + 8].tolist())
    return want, got


# ---- 1. named cases and golden files ----
def test_every_named_case_in_one_batch(L):
    cases = sqz_cases.small_cases()
    for name, f, e in cases:                                                # the host front end is the restatement's equal here
        rc, info, co = expected(f)
        ref = R.coeffs(f)
        assert (rc == 0) == (e == "ok") == (ref is not None), name
        if ref is not None:
            assert info == ref[1] and np.array_equal(co, ref[0]), name
    want, _ = read_files(L, [f for _, f, _ in cases], [n for n, _, _ in cases])
    assert sum(w == _capi.ERR_DECODE for w in want) >= 15 and sum(w == 0 for w in want) >= 70


def test_refused_headers_between_good_neighbours_and_alone(L):
    cases = sqz_cases.small_cases()
    good = [(n, f) for n, f, e in cases if e == "ok" and len(f) < 3000][::5]
    refused = [(n, f) for n, f, e in cases if e != "ok"]
    files, names = [], []
    for k, (n, f) in enumerate(refused):
        files += [good[k % len(good)][1], f]; names += [good[k % len(good)][0], n]
    files.append(good[0][1]); names.append(good[0][0])
    want, _ = read_files(L, files, names)
    assert [w != 0 for w in want] == [bool(k & 1) for k in range(len(files))]
    assert all(read_files(L, [f for _, f in refused], [n for n, _ in refused])[0])      # nothing but refused files
    read_files(L, files[:1])                                                # a batch of one


def test_a_negative_offset_is_refused_and_the_neighbours_are_read(L):
    files = [f for _, f, e in sqz_cases.small_cases() if e == "ok"][:3]
    exp = [expected(f) for f in files]
    offs = [GUARD + 1, -4, GUARD + 1 + exp[0][2].size + GUARD]
    total = offs[2] + exp[2][2].size + GUARD
    expect = np.full(total, FILL, np.uint16).view(np.int16)
    for k in (0, 2):
        expect[offs[k]:offs[k] + exp[k][2].size] = exp[k][2]
    bufs, ptrs, lens = host_buffers(files)
    dco = torch.from_numpy(np.full(total, FILL, np.uint16).view(np.int16)).cuda()
    st = (C.c_int * 3)(77, 77, 77)
    rc = L.gamut_hip_sqz_read_batch_device(ptrs, lens, 3, dco.data_ptr(), (C.c_int64 * 3)(*offs), None, st, None)
    torch.cuda.synchronize()
    assert rc == _capi.ERR_INVALID_ARG and list(st) == [0, _capi.ERR_INVALID_ARG, 0] and L.gamut_hip_last_error().startswith(b"image 1:")
    assert np.array_equal(dco.cpu().numpy(), expect)


def test_the_golden_files(L):
    import glob
    import os
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sqz", "*.sqz")))
    assert len(paths) == 8
    files = [open(p, "rb").read() for p in paths]
    for f in files:
        assert np.array_equal(expected(f)[2], R.coeffs(f)[0])
    assert not any(read_files(L, files, [os.path.basename(p) for p in paths])[0])


# ---- 2. prefixes ----
@pytest.mark.parametrize("which", [0, 1])
def test_every_prefix(L, which):
    files = sqz_cases.prefixes(sqz_cases.prefix_files()[which])
    for a in range(0, len(files), 400):
        assert not any(read_files(L, files[a:a + 400])[0])


# ---- 3. hand-built streams ----
def rec(sign, run):
    return [sign] + sqz_cases.run_code(run)


def long_rec(sign, pairs, run):
    """a record of `pairs` >= 32 (0, b) pairs: only the last 32 data bits count, and they are `run` mod 2^32"""
    assert pairs >= 32
    out = [sign]
    for b in [0] * (pairs - 32) + [(run >> (31 - i)) & 1 for i in range(32)]:
        out += [0, b]
    return out + [1]


def hand_streams(W, side):
    """side x side grey, one level, raster: round 0 is the LL band alone (n = (side / 2)^2 entries, its pass starts at bit 52, an even
    offset in its byte and in the file); the `odd` prefix completes two planes of LL with one significant coefficient, so one refinement
    bit later the HL band's pass starts at an odd bit.  Flags of a pass sit at ODD offsets from its start, so of the window offsets
    W - 1, W, W + 1 a record can close at W - 1 and at W + 1; at W lies the next record's sign (case closes_at_W-1) or a data bit of
    a record that closes at W + 1."""
    n = (side // 2) ** 2
    far = n + 36
    hd = sqz_cases.header_bits(side, side, 0, 1, 0, 0)
    rng = np.random.default_rng(side)
    tail = lambda k: [int(b) for b in rng.integers(0, 2, k)]
    even = hd + sqz_cases.nibble(6)
    odd = hd + sqz_cases.nibble(6) + rec(1, 3) + rec(0, far) + rec(0, far) + [1] + sqz_cases.nibble(7)
    assert len(even) % 2 == 0 and len(odd) % 2 == 1
    out = []
    add = lambda name, bits, tail_bytes=b"": out.append((name, sqz_cases.pack(bits) + tail_bytes))
    for pname, p in (("even", even), ("odd", odd)):
        add(f"{pname}_start_plain", p + rec(1, 2) + rec(0, 3) + rec(1, 1) + rec(0, far) + tail(200))
        for f in (W - 3, W - 1, W + 1, W + 3):                              # the first record's flag at offset f from the pass's start
            add(f"{pname}_closes_at_W{f - W:+d}", p + long_rec(1, (f - 1) // 2, 3) + rec(0, 2) + rec(1, far) + tail(64))
            add(f"{pname}_closes_at_W{f - W:+d}_then_ends", p + long_rec(1, (f - 1) // 2, 3))
        add(f"{pname}_longer_than_one_window", p + long_rec(0, W // 2 + 3, 5) + rec(1, 2) + rec(0, far) + tail(64))
        add(f"{pname}_longer_than_two_windows", p + rec(1, 2) + long_rec(0, W + 5, 7) + rec(1, far) + tail(64))
        add(f"{pname}_two_windows_all_ones", p + [1] + [0, 1] * (W + 5) + [1] + rec(1, 1) + tail(64))           # run 2^32 - 1: past any LIP
        add(f"{pname}_run_2^32+3", p + rec(1, 2 ** 32 + 3) + rec(0, 2) + rec(1, 2 ** 33 + 2 ** 32 + 7) + rec(0, far) + tail(64))
        add(f"{pname}_run_2^32", p + rec(1, 2) + rec(1, 2 ** 32) + tail(64))                                   # run 0: an advance of 2^32 ends the pass
        add(f"{pname}_long_run_0", p + rec(1, 2) + long_rec(0, W // 2 + 3, 0) + tail(64))
        for fill in (0x00, 0xFF, 0x55, 0xAA):
            for m in (1, 2, 3):
                add(f"{pname}_tail_{fill:02x}_{m}W", p + rec(1, 2), bytes([fill]) * (m * W // 8))
    # ---- the ends of the stream.  N - s is odd only for an odd start: the end rule needs the odd prefix
    for j0, name in ((0, "in_range"), (20, "overshooting")):
        for j in range(j0, j0 + 4):
            bits = odd + rec(1, 2) + [0] + [0, 1 if j0 else 0] * j
            if len(bits) % 8 == 0:
                add(f"ends_at_a_flag_position_{name}", bits)
    add("ends_at_a_sign_position", even + rec(1, 2))
    add("ends_at_a_data_position", even + rec(1, 1) + [1, 0])
    assert all(len(b) % 8 == 0 for b in (even + rec(1, 2), even + rec(1, 1) + [1, 0]))
    bits = even + rec(1, 2)
    while (len(bits) + len(rec(0, far))) % 8:
        bits += rec(0, 1)
    add("ends_behind_a_sorting_pass", bits + rec(0, far))                   # the refinement is skipped, the NSP stays unmerged
    for cut, name in ((0, "ends_behind_a_refinement_pass"), (2, "ends_inside_a_refinement_pass")):
        k = 5
        while True:
            bits = even
            for i in range(k):
                bits = bits + rec(i & 1, 2)
            bits = bits + rec(0, far) + rec(1, 4) + rec(0, far) + [1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0][:k - cut]
            if len(bits) % 8 == 0:
                break
            k += 1
        add(name, bits)
    k = 1
    while True:                                                             # round 1's first new band reads its nibble across the file's last byte
        bits = hd + sqz_cases.nibble(6)
        for i in range(k):
            bits = bits + rec(i & 1, 2)
        bits = bits + rec(0, far) + rec(0, far) + [1, 0, 1, 1, 0, 1][:k]
        if len(bits) % 8 > 4:
            break
        k += 1
    add("nibble_straddles_the_last_byte", bits + [1])
    add("max_bitplane_15", hd + sqz_cases.nibble(15) + rec(1, 1) + rec(0, 5) + rec(1, 2) + rec(0, far) + tail(400))
    add("max_bitplane_0", hd + sqz_cases.nibble(0) + tail(400))
    return out


def test_hand_built_streams_16x16(L):
    W = L.gamut_hip_sqz_read_window()
    cases = hand_streams(W, 16)
    names = [n for n, _ in cases]
    for must in ("ends_at_a_flag_position_in_range", "ends_at_a_flag_position_overshooting", "ends_at_a_sign_position", "ends_at_a_data_position",
                 "ends_behind_a_sorting_pass", "ends_behind_a_refinement_pass", "ends_inside_a_refinement_pass", "nibble_straddles_the_last_byte"):
        assert must in names, must
    assert not any(read_files(L, [f for _, f in cases], names)[0])
    d = dict(cases)                                                         # what the names promise, on the expectation
    co = expected(d["even_closes_at_W-1"])[2]
    assert co[2] & 0x41 == 0x41 and np.count_nonzero(co) >= 2      # the long record's run is 3: the third LL entry, negative
    for name, length in (("even_run_2^32", 66), ("even_long_run_0", 2 * (W // 2 + 3) + 2)):      # run 0 advances 2^32: the pass ends behind that record
        t, _, pos, closed = M.sorting_pass(np.unpackbits(np.frombuffer(d[name], np.uint8)), 52, 64)
        assert t.tolist() == [1] and closed and pos == 52 + 4 + length, name
    a, b = expected(d["ends_at_a_flag_position_in_range"])[2], expected(d["ends_at_a_flag_position_overshooting"])[2]
    assert np.count_nonzero(a) == np.count_nonzero(b) + 1                   # the record the end of the stream closed was applied
    assert np.count_nonzero(expected(d["nibble_straddles_the_last_byte"])[2]) >= 1


def test_hand_built_streams_with_a_band_larger_than_a_window(L):
    W = L.gamut_hip_sqz_read_window()
    side = 512
    assert (side // 2) ** 2 > W
    cases = hand_streams(W, side)
    assert not any(read_files(L, [f for _, f in cases], [n for n, _ in cases])[0])
    co = expected(dict(cases)["even_tail_ff_3W"])[2]
    assert np.count_nonzero(co) > W // 2                                    # a record per two bits: more than a window's worth of takes


# ---- 4. bands larger than the workgroup and the window ----
def test_large_bands_every_scan(L):
    files, names = [], []
    for scan in range(4):
        files.append(sqz_cases.make(256, 192, R.GREY, 1, scan, 0, seed=300 + scan)); names.append(f"256x192 scan {scan}")
        files.append(sqz_cases.make(300, 130, scan, 5, scan, scan & 1, seed=310 + scan)); names.append(f"300x130 scan {scan}")
    assert not any(read_files(L, files, names)[0])


def lossless_random(L, w, h, mode, levels, scan, seed):
    """random full-range sign-magnitude planes through the host writer: every band's sorting passes take about half of what is left"""
    planes = 1 if mode == 0 else 3
    rng = np.random.default_rng(seed)
    co = rng.integers(0, 1 << 15, planes * w * h, dtype=np.uint16).view(np.int16)
    co[co < 2] = 0                                                          # no sign without a magnitude
    d = _capi.SqzEncodeDesc()
    d.width, d.height, d.color_mode, d.levels, d.scan_order, d.subsampling, d.budget = w, h, mode, levels, scan, seed & 1, 6 + co.size * 6
    dst = np.zeros(d.budget, np.uint8)
    n = C.c_int64(0)
    assert L.gamut_hip_sqz_encode_coeffs(co.ctypes.data, C.byref(d), dst.ctypes.data, C.byref(n)) == 0, L.gamut_hip_last_error()
    f = dst[:n.value].tobytes()
    assert np.array_equal(expected(f)[2], co)                               # lossless: the stream holds every bit
    return f


def test_band_sizes_around_the_thread_count_and_the_window(L):
    """one level: four bands of (w / 2) * (h / 2) entries.  C - 1, C, C + 1 for C = 1024 lanes and C = the window; 2C + 1 has no admissible
    factorisation for either (2049 = 3 * 683 needs a side below 8, 65537 is prime), so 2C + 2 stands in"""
    W = L.gamut_hip_sqz_read_window()
    assert W == 32768
    shapes = {1023: (66, 62), 1024: (64, 64), 1025: (82, 50), 2050: (82, 100), 32767: (434, 302), 32768: (512, 256), 32769: (198, 662), 65538: (396, 662)}
    files, names = [], []
    for k, (n, (w, h)) in enumerate(shapes.items()):
        assert (w // 2) * (h // 2) == n
        files.append(lossless_random(L, w, h, 0 if n > 4000 else k % 4, 1, k % 4, 400 + k)); names.append(f"bands of {n}")
    files.append(lossless_random(L, 300, 130, 2, 5, 1, 420)); names.append("300x130, 5 levels")
    assert not any(read_files(L, files, names)[0])


# ---- 5. large and many ----
def test_2048x2048_with_8_levels(L):
    assert not any(read_files(L, [sqz_cases.big_case()])[0])


def mixed_600():
    files = list(sqz_cases.tiny_files(600))
    refused = [f for _, f, e in sqz_cases.small_cases() if e != "ok"]
    for k, f in enumerate(refused):
        files.insert(7 + 23 * k, f)
    return files


def test_600_tiny_files_in_one_call_and_in_chunks(L):
    files = mixed_600()
    want, whole = read_files(L, files)
    assert sum(w != 0 for w in want) >= 15
    total = sum(co.size for _, _, co in map(expected, files) if co is not None)
    prev = L.gamut_hip_sqz_set_read_chunk(total // 4)                       # at least four chunks
    try:
        assert prev > total
        want2, chunked = read_files(L, files)
    finally:
        L.gamut_hip_sqz_set_read_chunk(prev)
    assert want2 == want and np.array_equal(whole, chunked)
    prev = L.gamut_hip_sqz_set_read_chunk(1)                                # a file per chunk
    try:
        read_files(L, files[:40])
    finally:
        L.gamut_hip_sqz_set_read_chunk(prev)


def test_a_large_call_before_a_small_one_and_a_callers_stream(L):
    big = [sqz_cases.make(256, 192, R.OKLAB, 3, R.SNAKE, 1, seed=500), sqz_cases.make(300, 130, R.GREY, 5, R.HILBERT, 0, seed=501)]
    small = [f for _, f, e in sqz_cases.small_cases() if e == "ok"][:6]
    read_files(L, big)
    read_files(L, small)                                                    # the scratch of the large call is reused
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        read_files(L, big + small, stream=C.c_void_p(s.cuda_stream))
    read_files(L, small[:1], stream=C.c_void_p(s.cuda_stream))


# ---- 6. mutations ----
@pytest.mark.parametrize("part", range(4))
def test_2000_mutations(L, part):
    files = M.mutations(2000, seed=21)[part * 500:(part + 1) * 500]
    want, _ = read_files(L, files)
    assert sum(w == 0 for w in want) >= 400


# ---- 7. the switch ----
def decode_pixels(L, files):
    exp = [expected(f) for f in files]
    n = len(files)
    sizes = [co.size if co is not None else 64 for _, _, co in exp]        # planes * w * h bytes of pixels
    offs, pos = [], 4096
    for k, s in enumerate(sizes):
        pos += 1 + 2 * (k % 8)
        offs.append(pos)
        pos += s + 4096
    bufs, ptrs, lens = host_buffers(files)
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    info = (_capi.SqzInfo * n)()
    st = (C.c_int * n)(*([77] * n))
    rc = L.gamut_hip_sqz_decode_batch_device(ptrs, lens, n, (C.c_int64 * n)(*offs), out.data_ptr(), info, st, None)
    torch.cuda.synchronize()
    return rc, L.gamut_hip_last_error(), list(st), [_info_words(i) for i in info], out.cpu().numpy()


def test_the_switch_puts_the_reader_behind_the_batch_decode(L):
    files = [f for _, f, _ in sqz_cases.small_cases()]
    prev = L.gamut_hip_sqz_set_reader(0)
    try:
        host = decode_pixels(L, files)
        assert L.gamut_hip_sqz_set_reader(1) == 0
        dev = decode_pixels(L, files)
        assert L.gamut_hip_sqz_set_reader(0) == 1
    finally:
        L.gamut_hip_sqz_set_reader(prev)
    assert host[0] == dev[0] == _capi.ERR_DECODE and host[1] == dev[1] and host[2] == dev[2] and host[3] == dev[3]
    assert np.array_equal(host[4], dev[4]) and np.count_nonzero(host[4] != 0xA5) > 100000


def test_the_switch_puts_the_reader_behind_image_load(L):
    from gamut_amd import image as gi
    cases = sqz_cases.small_cases()
    prev = L.gamut_hip_sqz_set_reader(0)
    try:
        got = []
        for which in (0, 1):
            L.gamut_hip_sqz_set_reader(which)
            res = []
            for name, f, e in cases:
                im = gi.Image(device=bool(len(res) & 1))
                ok = im.loadFromMemory(f)
                assert ok == (e == "ok"), name
                res.append((ok, im.errorMessage, (im.type, im.width, im.height) if ok else None, np.asarray(im.pixels()).copy() if ok else None))
            got.append(res)
    finally:
        L.gamut_hip_sqz_set_reader(prev)
    for (name, _, _), a, b in zip(cases, *got):
        assert a[:3] == b[:3] and (a[3] is None or np.array_equal(a[3], b[3])), name


def test_the_default_reader_is_the_host(L):
    import os
    if os.environ.get("GAMUT_HIP_SQZ_READER", "host") == "host":
        assert L.gamut_hip_sqz_set_reader(9) == 0
