"""GPU parity of the BATCHED PNG de-filter launches: every kernel combination png_defilter_launch (gamut_amd/csrc/png.hip) can start
(tests/png_batch_cases.py, checked for completeness in test_png_batch_cases_cpu.py), each with several distinct images, against the CPU oracle.
Bar: the WHOLE output allocation, bit for bit: pixels, the gaps between images, the spare image slots behind the batch and a guard on either
side; the status words and the sentinels behind them.  The one exception: the own bytes of an image whose stream was damaged on purpose."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gen
import oracle_lib as O
import png_batch_cases as B
from png_batch_cases import inflate_mode  # noqa: F401 -- the fixture, shared with test_png_gpu.py

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A                                 # the words behind the status array
SENTINELS = 8


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _DeviceBuffer:
    """one device allocation reused by the cases of a test: every case uploads its whole image of it"""

    def __init__(self, L, nbytes):
        from gamut_amd import _capi
        self.L, self.nbytes, self.capi = L, nbytes, _capi
        self.ptr = L.gamut_hip_device_malloc(nbytes)
        assert self.ptr, _capi.last_error()

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.capi.check(self.L.gamut_hip_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes, None))
        self.capi.check(self.L.gamut_hip_stream_synchronize(None))

    def download(self, nbytes):
        assert nbytes <= self.nbytes
        host = np.empty(nbytes, np.uint8)
        self.capi.check(self.L.gamut_hip_memcpy_d2h(host.ctypes.data, self.ptr, nbytes, None))
        self.capi.check(self.L.gamut_hip_stream_synchronize(None))
        return host

    def free(self):
        self.L.gamut_hip_device_free(self.ptr)


def _raw_bytes(c):
    return 2 * B.GUARD + c.count * B.raw_geometry(c)[1]


class _Buffers:
    """the three device allocations of a run of cases: streams, output, status"""

    def __init__(self, L, cases):
        self.raw = _DeviceBuffer(L, max(_raw_bytes(c) for c in cases))
        self.out = _DeviceBuffer(L, max(B.allocation_bytes(c) for c in cases))
        self.status = _DeviceBuffer(L, 4 * (max(c.count for c in cases) + SENTINELS))
        assert self.out.ptr % 128 == 0 and self.raw.ptr % 16 == 0, "the mirror assumes allocations that start on a 128-byte line"

    def free(self):
        for d in (self.raw, self.out, self.status):
            d.free()


def _run_case(L, bufs, c, rng):
    """one launch of a case -> the list of what is wrong with its output (empty: nothing).  The streams lie raw_stride apart (not tight, odd) in an allocation whose gaps
    and guards hold noise; the output allocation is 0xA5 all over; the status array is count zero words and SENTINELS words behind them."""
    from gamut_amd import _capi
    G = B.GUARD
    need, rs = B.raw_geometry(c)
    shift, stride = B.geometry(c)
    name = B.case_variant(c, bufs.out.ptr)
    assert name == B.case_variant(c)
    hraw = rng.integers(1, 256, _raw_bytes(c), dtype=np.uint8)
    for i, r in enumerate(B.raw_streams(c)):
        assert r.size == need
        hraw[G + i * rs:G + i * rs + need] = r
    bufs.raw.upload(hraw)
    total = B.allocation_bytes(c)
    bufs.out.upload(np.full(total, 0xA5, np.uint8))
    hst = np.full(c.count + SENTINELS, SENTINEL, np.uint32)
    hst[:c.count] = 0
    bufs.status.upload(hst)
    q, a, r = B.MODES[c.mode]
    with _env(GAMUT_HIP_PNG_QUEUE=q, GAMUT_HIP_PNG_ALIGNED=a, GAMUT_HIP_PNG_ROLL=r):
        _capi.check(L.gamut_hip_png_defilter_batch_device(bufs.raw.ptr + G, rs, rs, bufs.out.ptr + G + shift, stride, c.x, c.y, c.img_n, c.out_n, c.depth, c.color,
                                                           c.count, None if c.bad == "null" else bufs.status.ptr, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    got = bufs.out.download(total)
    status = bufs.status.download(hst.nbytes).view(np.uint32)
    exp, mask = B.expected_allocation(c)
    wrong = []
    d = B.describe_difference(c, got, exp, mask)
    if d:
        wrong.append(d)
    want = np.zeros(c.count, bool)
    if c.bad == "status":
        want[B.bad_position(c)[0]] = True
    if (status[:c.count] != 0).tolist() != want.tolist() or (status[c.count:] != SENTINEL).any():
        wrong.append(f"{B.case_id(c)} [{name}]: status words {[hex(int(s)) for s in status]}, want non-zero at {np.flatnonzero(want).tolist()} only and "
                     f"{SENTINELS} x {SENTINEL:#x} behind the {c.count}")
    return wrong


@pytest.mark.parametrize("fmt", range(len(B.FORMATS)), ids=[f"n{n}-d{d}-c{c}" for (n, d, c) in B.FORMATS])
def test_every_variant_with_several_images(hip, fmt):
    """gamut_hip_png_defilter_batch_device on every case of the table for one format: 3 to 7 distinct images with their own row filters, widths on and off the memory
    lines and under one piece, 70 / 300 / 518 rows, five layouts of the output, the launch switches.  A wrong image index, stride, tail guard or row count shows as
    a changed byte inside the allocation and is reported as case, variant, image, row and column.  A case with an invalid filter byte in its middle image must flag
    that image alone and leave every other byte as the oracle has it -- with status = NULL too."""
    import test_png_gpu
    assert B.FORMATS == test_png_gpu.FORMATS
    cases = [c for c in B.CASES if (c.img_n, c.depth, c.color) == B.FORMATS[fmt]]
    bufs = _Buffers(hip, cases)
    rng = np.random.default_rng(700 + fmt)
    failures, ran = [], set()
    try:
        for c in cases:
            failures += _run_case(hip, bufs, c, rng)
            ran.add(B.case_variant(c))
    finally:
        bufs.free()
    assert not failures, f"{len(failures)} differences in {len(cases)} cases:\n" + "\n".join(failures[:8])
    assert ran == {B.case_variant(c) for c in cases}


@pytest.fixture(params=["host", "device"])
def inflate(request):
    """GAMUT_HIP_PNG_INFLATE: where gamut_hip_png_decode_batch_device inflates the IDAT streams"""
    with _env(GAMUT_HIP_PNG_INFLATE=request.param):
        yield request.param


def test_offset_tables_on_and_off_the_lines(hip, inflate):
    """gamut_hip_png_decode_batch_device on five files of one geometry (one de-filter launch through raw_offs / out_offs tables) and an odd-sized one in their middle:
    RGB8 -> 4, RGBA8 -> 4, grey8 -> 2, RGBA16 at 16 bits, RGB8 -> 3 with rows that are no dword multiple; out_offset in irregular steps that are all multiples of 128
    (with `out` on a line: offs_line_aligned), of 16, of 4, odd.  Every file == the oracle's stbi_load, and the whole allocation == the expected one."""
    from gamut_amd import _capi
    G, h = B.GUARD, B.TABLE_HEIGHT
    failures = []
    for k, fmt in enumerate(B.TABLE_FORMATS):
        color, ch, depth, req, bits, w = fmt
        rng = np.random.default_rng(50 + k)
        fb = B.filter_unit(ch, depth)
        files = []
        for i in range(5):
            smp = rng.integers(0, 1 << depth, (h, w * ch))
            if i % 2:
                smp = (np.cumsum(rng.integers(-2, 3, (h, w * ch)), axis=1) + smp[:, :1]) % (1 << depth)
            files.append(gen.write_png(smp, w, h, color, depth, filters=B.mixed_filters(rng, i, gen.pack_samples(smp, depth), fb)))
        files.insert(3, gen.write_png(rng.integers(0, 1 << depth, (9, 40 * ch)), 40, 9, color, depth, filters=rng.integers(0, 5, 9).astype(np.uint8)))
        n = len(files)
        bufs = [np.frombuffer(f, np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
        want = [np.ascontiguousarray(O.stbi_load(f, req, bits == 16)[0]).view(np.uint8).reshape(-1) for f in files]
        assert len({e.tobytes() for e in want}) == n
        for form in B.TABLE_FORMS:
            offs, span = B.table_offsets([e.size for e in want], form)
            d_out = _DeviceBuffer(hip, 2 * G + span)
            try:
                assert d_out.ptr % 128 == 0
                d_out.upload(np.full(2 * G + span, 0xA5, np.uint8))
                info = (_capi.PngInfo * n)(); st = (C.c_int * n)()
                rc = hip.gamut_hip_png_decode_batch_device(ptrs, lens, n, req, bits, offs.ctypes.data_as(C.POINTER(C.c_int64)), d_out.ptr + G, info, st, 3, None)
                assert rc == 0 and not any(st), (rc, list(st), hip.gamut_hip_last_error())
                _capi.check(hip.gamut_hip_stream_synchronize(None))
                got = d_out.download(2 * G + span)
                assert B.table_variant(fmt, form, d_out.ptr + G) == B.table_variant(fmt, form)
            finally:
                d_out.free()
            exp = np.full(2 * G + span, 0xA5, np.uint8)
            where = f"inflate on the {inflate}, colour type {color} depth {depth} req_comp {req} bits {bits} {w}x{h}, offsets {form} [{B.table_variant(fmt, form)}]"
            for i, e in enumerate(want):
                at = G + int(offs[i])
                exp[at:at + e.size] = e
                mine = got[at:at + e.size]
                if not np.array_equal(mine, e):
                    j = int(np.flatnonzero(mine != e)[0])
                    wi = info[i].width * req * (bits // 8)
                    failures.append(f"{where}: file {i} row {j // wi} column {j % wi // (req * (bits // 8))}")
                assert (info[i].width, info[i].height, info[i].channels, info[i].bits) == ((40, 9) if i == 3 else (w, h)) + (req, bits)
            if not np.array_equal(got, exp):
                j = int(np.flatnonzero(got != exp)[0])
                failures.append(f"{where}: allocation byte {j - G} (files start at {offs.tolist()}): got {got[j:j + 8].tolist()} want {exp[j:j + 8].tolist()}")
    assert not failures, f"{len(failures)} differences:\n" + "\n".join(failures[:8])


def _decode_files(hip, files, req, offs, span):
    """gamut_hip_png_decode_batch_device on three host threads into an allocation of 0xA5 -> (return code, status per file, message, the allocation)"""
    from gamut_amd import _capi
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); lens = (C.c_size_t * n)(*[b.size for b in bufs])
    d_out = _DeviceBuffer(hip, span)
    try:
        d_out.upload(np.full(span, 0xA5, np.uint8))
        info = (_capi.PngInfo * n)(); st = (C.c_int * n)()
        rc = hip.gamut_hip_png_decode_batch_device(ptrs, lens, n, req, 8, offs.ctypes.data_as(C.POINTER(C.c_int64)), d_out.ptr + B.GUARD, info, st, 3, None)
        msg = hip.gamut_hip_last_error().decode()
        _capi.check(hip.gamut_hip_stream_synchronize(None))
        return rc, list(st), msg, d_out.download(span)
    finally:
        d_out.free()


@pytest.mark.parametrize("req", [4, 0])
def test_every_failure_kind_in_one_batch(hip, inflate_mode, req):
    """twelve files of 5x3 and 8x8 in one call, eight of them broken, each in its own way (png_batch_cases.failure_batch), good ones first, last and in between: the status
    is non-zero exactly where the oracle's stbi_load refuses the file, every other file == the oracle, the allocation is 0xA5 outside the good files (the one
    exception, as everywhere in this file: the own bytes of the two files with a bad filter byte, which the de-filter meets when the file's pixels are already on their
    way -- so it was before the call was split into stages), the return code and the message are the first broken file's.
    Then each broken file behind one good one: its own message."""
    from gamut_amd import _capi
    G = B.GUARD
    batch = B.failure_batch()
    files = [f for _, f in batch]
    want = [O.stbi_load(f, req, False) for f in files]
    assert [w is None for w in want] == [k is not None for k, _ in batch]
    px = [None if w is None else np.ascontiguousarray(w[0]).reshape(-1) for w in want]
    offs, span = B.table_offsets([8 * 8 * 4 if p is None else p.size for p in px], "odd")
    span += 2 * G
    rc, st, msg, got = _decode_files(hip, files, req, offs, span)
    exp, mask = np.full(span, 0xA5, np.uint8), np.ones(span, bool)
    for i, (kind, _) in enumerate(batch):
        at = G + int(offs[i])
        if px[i] is not None:
            exp[at:at + px[i].size] = px[i]
        elif kind.startswith("filter 5"):                    # (the rows in front of the bad byte are there -- the batched launch -- or what png_run made of them)
            mask[at:at + 8 * 8 * (req or 3)] = False
    where = f"inflate on the {inflate_mode}, req_comp {req}"
    assert [s != 0 for s in st] == [p is None for p in px], (where, st)
    assert np.array_equal(got[mask], exp[mask]), (where, (np.flatnonzero((got != exp) & mask)[:8] - G).tolist(), offs.tolist())
    first = next(i for i, p in enumerate(px) if p is None)
    assert rc == st[first] == _capi.ERR_DECODE and msg == f"image {first}: {B.FAILURE_TEXT[batch[first][0]]}", (where, rc, st, msg)
    for kind, f in batch:
        if kind is None:
            continue
        o2, s2 = B.table_offsets([px[0].size, 8 * 8 * 4], "odd")
        rc, st, msg, _ = _decode_files(hip, [files[0], f], req, o2, s2 + 2 * G)
        assert (rc, st, msg) == (_capi.ERR_DECODE, [0, _capi.ERR_DECODE], f"image 1: {B.FAILURE_TEXT[kind]}"), (where, kind, rc, st, msg)


@pytest.mark.parametrize("img_n,depth,x,y", [(1, 1, 8, 2), (2, 16, 2, 2)], ids=["grey1-8x2", "greyalpha16-2x2"])
def test_more_images_than_65535(hip, img_n, depth, x, y):
    """one launch of 65 537 images, more than a grid's y or z dimension holds: 251 distinct images (a prime: a wrapped or truncated image index shows), cycled.  1-bit grey
    takes the per-lane kernel with FB = 1 and the scalar expand; 16-bit grey + alpha the per-lane kernel with FB = 4 and -- count being over 65 535 -- the scalar
    expand instead of the vector one.  Every image == the oracle, the gaps, two spare slots and the guards stay 0xA5, no status word is set."""
    from gamut_amd import _capi
    G, count, P = B.GUARD, 65537, 251
    color = 0 if img_n == 1 else 4
    assert B.variant(x, y, img_n, img_n, depth, count, 0, 19) == f"lane<{B.filter_unit(img_n, depth)}> + expand"
    assert B.variant(x, y, img_n, img_n, depth, 65535, 0, 19).endswith(" + expand_vec<2,2,2>" if depth == 16 else " + expand")
    rng = np.random.default_rng(depth)
    fb = B.filter_unit(img_n, depth)
    raws, exps = [], []
    while len(raws) < P:
        rows = gen.pack_samples(rng.integers(0, 1 << depth, (y, x * img_n)), depth)
        raw = gen.png_forward_filter(rows, fb, rng.integers(0, 5, y))
        e = O.png_create_image_raw(raw, img_n, img_n, x, y, depth, color)
        if not any(np.array_equal(e, o) for o in exps):
            raws.append(raw); exps.append(e)
    raws, exps = np.stack(raws), np.stack(exps)
    need, n = raws.shape[1], exps.shape[1]
    rs, stride = (need + 8) | 1, n + 3
    which = np.arange(count) % P
    hraw = rng.integers(1, 256, (count, rs), dtype=np.uint8)
    hraw[:, :need] = raws[which]
    hraw = np.concatenate([rng.integers(1, 256, G, dtype=np.uint8), hraw.reshape(-1), rng.integers(1, 256, G, dtype=np.uint8)])
    total = 2 * G + (count + B.SPARE) * stride
    exp = np.full(total, 0xA5, np.uint8)
    exp[G:G + count * stride].reshape(count, stride)[:, :n] = exps[which]
    d_raw, d_out, d_st = _DeviceBuffer(hip, hraw.size), _DeviceBuffer(hip, total), _DeviceBuffer(hip, 4 * (count + SENTINELS))
    try:
        d_raw.upload(hraw)
        d_out.upload(np.full(total, 0xA5, np.uint8))
        hst = np.full(count + SENTINELS, SENTINEL, np.uint32)
        hst[:count] = 0
        d_st.upload(hst)
        with _env(GAMUT_HIP_PNG_QUEUE=None, GAMUT_HIP_PNG_ALIGNED=None, GAMUT_HIP_PNG_ROLL=None):
            rc = hip.gamut_hip_png_defilter_batch_device(d_raw.ptr + G, rs, rs, d_out.ptr + G, stride, x, y, img_n, img_n, depth, color, count, d_st.ptr, None)
        assert rc == 0, (rc, hip.gamut_hip_last_error())
        _capi.check(hip.gamut_hip_stream_synchronize(None))
        got = d_out.download(total)
        status = d_st.download(hst.nbytes).view(np.uint32)
    finally:
        for d in (d_raw, d_out, d_st):
            d.free()
    assert np.array_equal(status, hst), np.flatnonzero(status != hst)[:8]
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        k = int(bad[0])
        if k < G or k >= G + (count + B.SPARE) * stride:
            where = "the guard in front" if k < G else "the guard behind"
        else:
            img, r = divmod(k - G, stride)
            where = f"image {img}" + (" (a spare slot behind the batch)" if img >= count else ": the gap behind its rows" if r >= n else f" byte {r}")
        images = np.unique((bad[(bad >= G) & (bad < G + count * stride)] - G) // stride)
        pytest.fail(f"{bad.size} bytes differ in {images.size} images (the first: {images[:6].tolist()}, the last: {images[-3:].tolist()}), first at {where}: "
                    f"got {got[k:k + 8].tolist()} want {exp[k:k + 8].tolist()}")


GROUP_CASES = [B.Case(4, 8, 6, 4, 67, 150, 7, "stride+4", "queue", "mix", None), B.Case(3, 8, 2, 4, 67, 150, 7, "stride+4", "queue", "mix", None)]


def _group_child():
    """the child of test_queue_groups_in_a_child_process: prints a verdict per image"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    bufs = _Buffers(L, GROUP_CASES)
    rng = np.random.default_rng(5)
    clean = True
    for c in GROUP_CASES:
        wrong = _run_case(L, bufs, c, rng)
        clean = clean and not wrong
        print(f"variant {c.img_n}->{c.out_n}: {B.case_variant(c)}")
        for line in wrong:
            print("difference:", line)
        # per image: its own bytes of the allocation against the oracle (the gaps and guards are in `wrong`)
        exp, _ = B.expected_allocation(c)
        got = bufs.out.download(exp.size)
        shift, stride = B.geometry(c)
        for i in range(c.count):
            at = B.GUARD + shift + i * stride
            same = np.array_equal(got[at:at + B.image_bytes(c)], exp[at:at + B.image_bytes(c)])
            print(f"image {c.img_n}->{c.out_n} {i}: {'equal' if same else 'DIFFERENT'}")
    bufs.free()
    print("allocations:", "clean" if clean else "DIFFERENT")


def test_queue_groups_in_a_child_process():
    """the queue's group arithmetic: GAMUT_HIP_PNG_GROUP is read once per process, so a fresh child process runs with it set to 3 and the queue forced -- 7 images of
    3 bands, RGBA8 and RGB8 -> RGBA8: groups of 3, 3 and 1 images (a short last group), band-major inside each.  The child prints a verdict per image."""
    for c in GROUP_CASES:
        assert B.case_variant(c) in ("queue<4>", "queue<3,RGBA>") and (c.y + 63) // 64 == 3 and c.count == 7
    env = dict(os.environ, GAMUT_HIP_PNG_GROUP="3")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--group-child"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, cwd=os.path.dirname(os.path.abspath(__file__)))
    lines = r.stdout.splitlines()
    assert r.returncode == 0, r.stdout[-3000:]
    verdicts = [ln for ln in lines if ln.startswith("image ")]
    assert verdicts == [f"image {c.img_n}->{c.out_n} {i}: equal" for c in GROUP_CASES for i in range(c.count)], r.stdout[-3000:]
    assert "allocations: clean" in lines and not [ln for ln in lines if ln.startswith("difference:")], r.stdout[-3000:]


if __name__ == "__main__" and sys.argv[1:] == ["--group-child"]:
    _group_child()
