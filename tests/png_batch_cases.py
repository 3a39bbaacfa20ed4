"""Batched PNG de-filter: which kernels a launch takes (a mirror of png_defilter_launch, gamut_amd/csrc/png.hip), the table of batches that
reaches every one of them with several DISTINCT images, and the inputs / oracle outputs of those batches.

TEST INFRASTRUCTURE, shared by test_png_batch_cases_cpu.py (the table is complete, its inputs can show a wrong image index) and
test_png_batch_gpu.py (the kernels against the oracle).  Nothing here touches a GPU.

The launcher chooses by: the filter unit FB, the row bytes wb, `fused` / `rgba_fused` (8-bit rows written straight into a dword-aligned
output) or the scratch + expand route, `lines` / `rows16` (the de-filtered rows' base, pitch and image stride on 128 / 16 bytes), the row
segments of small batches, the work queue, its rolling form, and for the expand stage depth and count.  A variant's name is the de-filter
kernel, " seg=N" where images are cut into N row segments, and " + " the expand kernel where the rows go through the scratch."""
import collections
import functools
import os
import re
import zlib

import numpy as np
import pytest

import gen
import oracle_lib as O
from png_host_corpus import idat_stream, with_idat

# (img_n, depth, color): the same fifteen as tests/test_png_gpu.py (test_png_batch_gpu.py asserts it)
FORMATS = [(1, 1, 0), (1, 2, 0), (1, 4, 0), (1, 8, 0), (1, 16, 0), (2, 8, 4), (2, 16, 4), (3, 8, 2), (3, 16, 2), (4, 8, 6), (4, 16, 6),
           (1, 1, 3), (1, 2, 3), (1, 4, 3), (1, 8, 3)]
GUARD = 4096                                                          # bytes in front of and behind every device allocation of a case
SPARE = 2                                                             # image slots behind the batch that must stay untouched
PNG_WAVES = 8                                                         # png.hip: bands in flight per workgroup
# GAMUT_HIP_PNG_QUEUE, GAMUT_HIP_PNG_ALIGNED, GAMUT_HIP_PNG_ROLL (None: unset) -- the five of test_png_gpu.py's launch_mode, and the launcher's own rules
MODES = {"default": (None, None, None), "workgroups": ("0", "0", "0"), "queue": ("1", "0", "0"), "workgroups+aligned": ("0", "1", "0"),
         "queue+aligned": ("1", "1", "0"), "queue+roll": ("1", "0", "1")}
# out on a 128-byte line and the stride a multiple of 128 / the stride + 16 / + 4 / + 1 / out itself 4 bytes off a line
LAYOUTS = {"lines": (0, 0), "stride+16": (0, 16), "stride+4": (0, 4), "stride+1": (0, 1), "out+4": (4, 0)}


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def row_bytes(x, img_n, depth):
    return (img_n * x * depth + 7) >> 3


def filter_unit(img_n, depth):
    return 1 if depth < 8 else img_n * (2 if depth == 16 else 1)


def variant(x, y, img_n, out_n, depth, count, out_addr, out_stride, offs=False, offs_dword_aligned=False, offs_line_aligned=False,
            queue_env=None, aligned_env=None, roll_env=None, scratch_addr=0):
    """What png_defilter_launch starts for these arguments, as the code decides it.  out_addr: the `out` pointer; offs: raw_offs / out_offs tables are
    passed (then out_stride does not count and the two flags do); the three *_env: the values of GAMUT_HIP_PNG_QUEUE / _ALIGNED / _ROLL (None: unset);
    scratch_addr: where the launcher's own scratch lies (hipMalloc: on a 128-byte line)."""
    nbytes = 2 if depth == 16 else 1
    FB = filter_unit(img_n, depth)
    wb = row_bytes(x, img_n, depth)
    out_dwords = out_addr % 4 == 0 and (offs_dword_aligned if offs else (count == 1 or out_stride % 4 == 0))
    rgba_fused = depth == 8 and img_n == 3 and out_n == 4 and wb >= 16 and out_dwords
    fused = rgba_fused or (depth == 8 and out_n == img_n and wb % 4 == 0 and out_dwords)
    if fused:
        D, d_stride, d_offs, d_pitch = out_addr, out_stride, offs, (x * 4 if rgba_fused else wb)
    else:
        group = 4 * FB
        d_pitch = (wb + group - 1) // group * group
        d_pitch = (d_pitch + 127) // 128 * 128
        D, d_stride, d_offs = scratch_addr, d_pitch * y, False
    nseg = 1
    if count < 512 and y >= 256:
        nseg = min(8, 1024 // count)
        while nseg > 1 and y // nseg < 128:
            nseg -= 1
    nbands = (y + 63) // 64
    aligned_asked = not rgba_fused and wb >= 16 and (_atoi(aligned_env) != 0 if aligned_env else wb >= 256)
    lines = D % 128 == 0 and d_pitch % 128 == 0 and (offs_line_aligned if d_offs else (count == 1 or d_stride % 128 == 0))
    rows16 = D % 16 == 0 and d_pitch % 16 == 0 and (offs_line_aligned if d_offs else (count == 1 or d_stride % 16 == 0))
    aligned = aligned_asked and (lines or rows16)
    units = count * nbands
    queue = wb >= 16 and d_pitch * 64 < (1 << 31) and units < (1 << 31) and (_atoi(queue_env) != 0 if queue_env else units >= 1024)
    flags = (",RGBA" if rgba_fused else "") + (",AL" if aligned and not rgba_fused else "") + (",LN" if lines else "")
    if queue:
        roll = not rgba_fused and wb >= 16 and roll_env is not None and _atoi(roll_env) != 0
        name = f"rollq<{FB}>" if roll else f"queue<{FB}{flags}>"
    else:
        name = f"ring<{FB}{flags}>" if wb >= 16 else f"lane<{FB}>"
        if nseg > 1:
            name += f" seg={nseg}"
    if not fused:
        vec = depth >= 8 and count <= 65535 and (img_n, out_n) in ((1, 1), (1, 2), (2, 2), (3, 3), (3, 4), (4, 4))
        name += f" + expand_vec<{img_n},{out_n},{nbytes}>" if vec else " + expand"
    return name


def without_segments(name):
    return re.sub(r" seg=\d+", "", name)


def segments(name):
    m = re.search(r" seg=(\d+)", name)
    return int(m.group(1)) if m else 1


def defilter_kernel(name):
    return without_segments(name).split(" + ")[0]


def family(name):
    return name.split("<")[0]


# ------------------------------------------------------------------------------------------------ the cases
# filt: "mix" = every image its own kind of row filters (all-Paeth, all-None, random 0..4, random 2..4, the encoder's heuristic; a sixth and seventh image: random
# again), "cuts" = the patterns of the
# row-segment cases.  bad: None, or an invalid filter byte (9) in the middle image: "status" = with a status array, "null" = with status = NULL.
Case = collections.namedtuple("Case", "img_n depth color out_n x y count layout mode filt bad")


def _width(img_n, depth, ok):
    x = 1
    while not ok(x, row_bytes(x, img_n, depth)):
        x += 1
    return x


def widths(img_n, depth):
    """-> the widths of a format's cases by name.  lines: rows of whole 128-byte lines (>= 256 bytes: the launcher's own rule takes the line-aligned loads);
    ragged: an odd width of more than two 128-byte groups plus a tail (sub-byte depths: a partly filled last byte; 8-bit grey, grey + alpha, RGB: rows that are no
    dword multiple); dwords (those three only): ragged rows that are dword multiples, so they stay fused, but no multiple of 16; lane: rows under 16 bytes for the
    per-lane kernel, as wide as they get with an odd width; lane4 (those three): four pixels, rows under 16 bytes that stay fused."""
    w = {"lines": _width(img_n, depth, lambda x, wb: wb % 128 == 0 and wb >= 256),
         "ragged": _width(img_n, depth, lambda x, wb: wb >= 265 and x % 2 == 1),
         "lane": max(x for x in range(1, 14, 2) if row_bytes(x, img_n, depth) < 16)}
    if depth == 8 and img_n < 4:
        w["dwords"] = _width(img_n, depth, lambda x, wb: wb >= 265 and wb % 4 == 0 and wb % 16 != 0)
        w["lane4"] = 4
    return w


def out_ns(img_n):
    return [img_n] + ([img_n + 1] if img_n < 4 else [])               # the launcher: out_n == img_n or img_n + 1, at most 4


def _cases():
    cases = []
    wg = ("workgroups", "workgroups+aligned")
    five = [m for m in MODES if m != "default"]
    for k, (img_n, depth, color) in enumerate(FORMATS):
        w = widths(img_n, depth)
        for out_n in out_ns(img_n):
            def add(x, y, count, layouts, modes, filt="mix", bad=None):
                for layout in layouts:
                    for mode in modes:
                        cases.append(Case(img_n, depth, color, out_n, x, y, count, layout, mode, filt, bad))
            # 70 rows: two bands, the second partial
            add(w["lines"], 70, 5, LAYOUTS, MODES)
            add(w["ragged"], 70, 5, ("lines", "stride+4", "stride+1"), five)
            add(w["lane"], 70, 5, ("lines", "stride+1"), ("default", "workgroups", "queue+roll"))
            if "dwords" in w and out_n == img_n:
                add(w["dwords"], 70, 7, ("lines", "stride+16", "stride+1"), five)
                add(w["lane4"], 70, 5, ("lines", "stride+1"), ("workgroups", "queue+aligned"))
            # 518 rows: nine bands, a wave takes a second one; every kernel family
            add(w["ragged"], 518, 4, ("stride+4",), ("workgroups", "queue", "queue+roll"))
            add(w["lane"], 518, 4, ("stride+4",), ("workgroups",))
            # 300 rows, 3 and 7 images: two row segments an image
            add(w["lines"], 300, 3, ("lines", "stride+4"), wg, "cuts")
            add(w["lines"], 300, 7, ("stride+16", "stride+1"), wg, "cuts")
            add(w["ragged"], 300, 7 if k % 2 else 3, ("stride+4",), ("workgroups",), "cuts")
            add(w["lane"], 300, 3 if k % 2 else 7, ("lines",), ("workgroups",), "cuts")
    # an invalid filter byte in the middle image: every kernel family, a fused format and a scratch one
    for (img_n, depth, color, out_n) in ((4, 8, 6, 4), (3, 8, 2, 4), (1, 2, 0, 1)):
        w = widths(img_n, depth)
        for bad in ("status", "null"):
            for mode in ("workgroups", "queue+aligned", "queue+roll"):
                cases.append(Case(img_n, depth, color, out_n, w["ragged"], 70, 5, "stride+4", mode, "mix", bad))
            cases.append(Case(img_n, depth, color, out_n, w["lane"], 70, 5, "stride+4", "workgroups", "mix", bad))
            cases.append(Case(img_n, depth, color, out_n, w["ragged"], 300, 3, "stride+4", "workgroups", "cuts", bad))
    # neighbours share their inputs and their oracle output: see inputs() / expected()
    return sorted(cases, key=lambda c: (FORMATS.index((c.img_n, c.depth, c.color)), c.x, c.y, c.count, c.filt, c.out_n, c.layout, c.mode, str(c.bad)))


def sample_bytes(c):
    return 2 if c.depth == 16 else 1


def image_bytes(c):
    return c.x * c.y * c.out_n * sample_bytes(c)


def geometry(c):
    """-> (offset of `out` behind the front guard, image stride) in bytes: tight rows, the images in slots of a multiple of 128 bytes, then off it"""
    shift, extra = LAYOUTS[c.layout]
    return shift, (image_bytes(c) + 127) // 128 * 128 + 128 + extra


def raw_geometry(c):
    """-> (bytes of one stream, raw_stride): not tight, and odd"""
    need = (row_bytes(c.x, c.img_n, c.depth) + 1) * c.y
    return need, (need + 8) | 1


def case_variant(c, alloc_addr=0):
    """the variant of a case whose output allocation starts at alloc_addr (a multiple of 128, as the GPU test asserts of the real one)"""
    shift, stride = geometry(c)
    q, a, r = MODES[c.mode]
    return variant(c.x, c.y, c.img_n, c.out_n, c.depth, c.count, alloc_addr + GUARD + shift, stride, queue_env=q, aligned_env=a, roll_env=r)


def case_id(c):
    return (f"n{c.img_n} d{c.depth} c{c.color} -> {c.out_n}  {c.x}x{c.y} count={c.count} {c.layout} {c.mode} filters={c.filt}"
            + (f" bad filter byte, status {'array' if c.bad == 'status' else 'NULL'}" if c.bad else ""))


CASES = _cases()


# ------------------------------------------------------------------------------------------------ inputs and expected outputs
def mixed_filters(rng, kind, rows, fb):
    y = rows.shape[0]
    if kind == 0:
        return np.full(y, 4, np.uint8)
    if kind == 1:
        return np.full(y, 0, np.uint8)
    if kind == 2:
        return rng.integers(0, 5, y).astype(np.uint8)
    if kind == 3:
        return rng.integers(2, 5, y).astype(np.uint8)
    return gen.png_heuristic_filters(rows, fb)


def _cut_filters(rng, i, rows, fb):
    """row filters for the segment cases (two segments: one boundary, at y / 2, looked for within y / 4 - 1 rows of it -- png.hip, cut_row): a cut row (None / Sub) a
    few rows behind the boundary, one just in front of it, on it, cut rows only far from it (the boundary stays without one), none at all, then ordinary mixes"""
    y = rows.shape[0]
    f = rng.integers(2, 5, y).astype(np.uint8)
    if i == 0:
        f[y // 2 + 3] = 0
    elif i == 1:
        f[y // 2 - 1] = 1
        f[y // 2 + 40] = 0                     # further away on the other side: the nearer one wins
    elif i == 2:
        f[3] = 0
        f[y - 2] = 1
        f[y // 2 - y // 4] = 1                 # one row outside the window
    elif i == 3:
        pass                                   # no cut row at all
    elif i == 4:
        f[y // 2] = 1
    elif i == 5:
        f = rng.integers(0, 5, y).astype(np.uint8)
    else:
        f = gen.png_heuristic_filters(rows, fb)
    return f


@functools.lru_cache(maxsize=8)
def _inputs(img_n, depth, x, y, count, filt):
    rng = np.random.default_rng([img_n, depth, x, y, count, len(filt)])
    fb = filter_unit(img_n, depth)
    samples, filters, raws = [], [], []
    for i in range(count):
        s = rng.integers(0, 1 << depth, (y, x * img_n))
        if i % 2 and x > 8:                                           # smooth rows: the heuristic then picks more than one filter
            s = (np.cumsum(rng.integers(-2, 3, (y, x * img_n)), axis=1) + s[:, :1]) % (1 << depth)
        rows = gen.pack_samples(s, depth)
        f = _cut_filters(rng, i, rows, fb) if filt == "cuts" else mixed_filters(rng, (i + x + y) % 5 if i < 5 else 2 + i % 2, rows, fb)
        raw = gen.png_forward_filter(rows, fb, f)
        for a in (s, f, raw):
            a.setflags(write=False)
        samples.append(s); filters.append(f); raws.append(raw)
    return tuple(samples), tuple(filters), tuple(raws)


def inputs(c):
    """-> per image: the samples (y, x * img_n), the row filters (y,), the filtered stream ((wb + 1) * y bytes).  Read-only: shared between cases."""
    return _inputs(c.img_n, c.depth, c.x, c.y, c.count, c.filt)


def bad_position(c):
    """-> (image, byte of its stream) of the invalid filter byte of a `bad` case: the middle image, a row in its middle"""
    return c.count // 2, (row_bytes(c.x, c.img_n, c.depth) + 1) * (c.y // 2)


def raw_streams(c):
    """the streams as the launch gets them: clean, or with the one invalid filter byte"""
    raws = list(inputs(c)[2])
    if c.bad:
        img, at = bad_position(c)
        r = raws[img].copy()
        r[at] = 9
        raws[img] = r
    return raws


@functools.lru_cache(maxsize=8)
def _expected(img_n, depth, color, out_n, x, y, count, filt):
    out = []
    for raw in _inputs(img_n, depth, x, y, count, filt)[2]:
        e = O.png_create_image_raw(raw, img_n, out_n, x, y, depth, color)
        assert e is not None
        e.setflags(write=False)
        out.append(e)
    return tuple(out)


def expected(c):
    """-> the oracle's output bytes per image (of the CLEAN streams).  Read-only: shared between cases."""
    return _expected(c.img_n, c.depth, c.color, c.out_n, c.x, c.y, c.count, c.filt)


def allocation_bytes(c):
    return 2 * GUARD + (c.count + SPARE) * geometry(c)[1]


def expected_allocation(c):
    """the whole output allocation as it must read after the launch: GUARD, count + SPARE image slots `stride` apart (the first one `shift` behind the guard), GUARD
    -- 0xA5 wherever no pixel belongs.  -> (bytes, mask): mask is False over the damaged image's own bytes of a `bad` case, which nothing is asked of."""
    shift, stride = geometry(c)
    n = image_bytes(c)
    buf = np.full(allocation_bytes(c), 0xA5, np.uint8)
    mask = np.ones(buf.size, bool)
    for i, e in enumerate(expected(c)):
        at = GUARD + shift + i * stride
        buf[at:at + n] = e
        if c.bad and i == bad_position(c)[0]:
            mask[at:at + n] = False
    return buf, mask


def describe_difference(c, got, exp, mask=None):
    """where two allocations of a case first differ: case, variant, image, row and column"""
    diff = got != exp
    if mask is not None:
        diff &= mask
    bad = np.flatnonzero(diff)
    if bad.size == 0:
        return None
    shift, stride = geometry(c)
    k = int(bad[0])
    head = f"{case_id(c)} [{case_variant(c)}]: {bad.size} bytes differ, first at byte {k}: got {got[k:k + 8].tolist()} want {exp[k:k + 8].tolist()} -- "
    first, end = GUARD + shift, GUARD + shift + (c.count + SPARE) * stride
    if k < first or k >= end:
        return head + ("the guard in front" if k < first else "the guard behind")
    img, r = divmod(k - first, stride)
    where = f"image {img}" + (" (a spare slot behind the batch)" if img >= c.count else "")
    if img >= c.count:
        return head + where
    if r >= image_bytes(c):
        return head + f"{where}: the gap behind its rows"
    px = c.out_n * sample_bytes(c)
    row, col = divmod(r, c.x * px)
    return head + f"{where} row {row} column {col // px} (byte {col % px} of the pixel; row filter {int(inputs(c)[1][img][row])})"


# ------------------------------------------------------------------------------------------------ files through offset tables
# gamut_hip_png_decode_batch_device: (colour type, channels, depth, req_comp, bits, width) -- 64 pixels: rows of whole lines where the rows are fused; 67 pixels of RGB8:
# rows that are no dword multiple
TABLE_FORMATS = ((2, 3, 8, 4, 8, 64), (6, 4, 8, 4, 8, 64), (0, 1, 8, 2, 8, 64), (6, 4, 16, 4, 16, 64), (2, 3, 8, 3, 8, 67))
TABLE_HEIGHT = 70
TABLE_FORMS = ("lines", "16", "4", "odd")


def table_offsets(sizes, form):
    """out_offset of files of these sizes, in irregular steps: all multiples of 128 / of 16 but none of 128 / of 4 / odd ones.  -> (offsets, bytes they span)"""
    steps = [(s + 127) // 128 * 128 + 128 * (1 + i % 3) for i, s in enumerate(sizes)]
    offs = np.concatenate([[0], np.cumsum(steps)[:-1]]).astype(np.int64)
    if form == "16":
        offs += 16 * (1 + np.arange(len(sizes)) % 7)
    elif form == "4":
        offs += 4 * (1 + np.arange(len(sizes)) % 3)
    elif form == "odd":
        offs += 1 + 2 * (np.arange(len(sizes)) % 5)
    else:
        assert form == "lines"
    return offs, int(sum(steps)) + 128


def table_variant(fmt, form, out_addr=0, x=None, y=TABLE_HEIGHT, count=5):
    """what the one launch of the `count` same-geometry files of a table case starts (the flags are those of ALL the call's offsets, the odd-sized file's included)"""
    color, ch, depth, req, bits, w = fmt
    offs, _ = table_offsets([1] * (count + 1), form)
    return variant(w if x is None else x, y, ch, req, depth, count, out_addr, 0, offs=True,
                   offs_dword_aligned=out_addr % 4 == 0 and all(o % 4 == 0 for o in offs), offs_line_aligned=out_addr % 128 == 0 and all(o % 128 == 0 for o in offs))


# ------------------------------------------------------------------------------------------------ the file-level batch call
@pytest.fixture(params=["host", "device", "device, pitched staging", "device, tight staging"])
def inflate_mode(request):
    """where the IDAT streams of the PNG batch call are inflated: zlib on the host threads, or k_inflate on the GPU (inflate.hip: batches of more
    files than host threads choose it themselves, GAMUT_HIP_PNG_INFLATE forces either) -- and, on the GPU, how the streams' slices go up: every
    stream `pitch` bytes apart and one hipMemcpy2DAsync per slice round, or a tight image and a copy per (stream, slice) (the call picks by how
    unequal the streams are; GAMUT_HIP_PNG_PITCHED forces either)"""
    keys = ("GAMUT_HIP_PNG_INFLATE", "GAMUT_HIP_PNG_PITCHED", "GAMUT_HIP_PNG_SLICE_KB")
    old = [os.environ.get(k) for k in keys]
    os.environ["GAMUT_HIP_PNG_INFLATE"] = request.param.split(",")[0]
    if "staging" in request.param:                               # 64 KiB slices: the larger files of the tests take several rounds
        os.environ["GAMUT_HIP_PNG_PITCHED"] = "1" if "pitched" in request.param else "0"
        os.environ["GAMUT_HIP_PNG_SLICE_KB"] = "64"
    yield request.param.split(",")[0]
    for k, v in zip(keys, old):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# what the batch call says of each kind of broken file (gamut_hip_last_error() behind "image N: "), written down from a run of the commit before the call was
# split into stages
FAILURE_TEXT = {"bad signature": "png: bad signature", "no IDAT": "png: no IDAT", "bad zlib header": "png: bad zlib header", "flipped bit": "png: corrupt zlib stream",
                "cut short": "png: corrupt zlib stream", "filter 5, batched": "png: invalid filter", "filter 5, Adam7": "png: invalid filter", "no PLTE": "png: no PLTE"}


@functools.lru_cache(maxsize=None)
def failure_batch():
    """[(kind or None, file)]: twelve files of 5x3 and 8x8, every kind of failure the file-level batch call tells apart, good files first, last and in between.
    Three good 8x8 RGB8 files and the one with filter byte 5 share a geometry: one batched de-filter launch."""
    rng = np.random.default_rng(404)

    def rgb(w, h, **kw):
        return gen.write_png(rng.integers(0, 256, (h, w * 3)), w, h, 2, 8, **kw)

    def refiltered(data, row_bytes, row):                       # the file with filter byte 5 in front of a row of its (first) image
        raw = bytearray(zlib.decompress(idat_stream(data)))
        raw[row * (row_bytes + 1)] = 5
        return with_idat(data, [zlib.compress(bytes(raw), 6)])

    good = rgb(8, 8, filters=0)
    z = idat_stream(good)
    # one flipped bit that no decoder can take: a stored block's LEN no longer matches its NLEN, a coded block's BTYPE becomes 11
    btype = (z[2] >> 1) & 3
    flipped = z[:3] + bytes([z[3] ^ 1]) + z[4:] if btype == 0 else z[:2] + bytes([z[2] ^ (4 if btype == 1 else 2)]) + z[3:]
    bad_header = bytearray(z[:2]); bad_header[1] = 0x79
    files = [(None, rgb(5, 3)),
             ("bad signature", b"\x88" + good[1:]),
             (None, gen.write_png(rng.integers(0, 256, (8, 8 * 4)), 8, 8, 6, 8)),
             ("no IDAT", with_idat(good, [])),
             ("bad zlib header", with_idat(good, [bytes(bad_header[:1]), bytes(bad_header[1:])] + [z[i:i + 1] for i in range(2, len(z))])),
             (None, rgb(8, 8)),
             ("flipped bit", with_idat(good, [flipped])),
             ("cut short", with_idat(good, [z[:len(z) // 2]])),
             ("filter 5, batched", refiltered(good, 8 * 3, 4)),
             ("filter 5, Adam7", refiltered(rgb(8, 8, interlace=1, filters=0), 1 * 3, 0)),
             ("no PLTE", gen.write_png(rng.integers(0, 16, (3, 5)), 5, 3, 3, 4)),
             (None, rgb(8, 8))]
    assert len(files) == 12 and {k for k, _ in files if k} == set(FAILURE_TEXT)
    return files
