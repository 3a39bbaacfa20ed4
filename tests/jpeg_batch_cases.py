"""Batched JPEG reconstruction: which kernel a launch takes (a mirror of the two launchers of gamut_amd/csrc/jpeg.hip), the table of
batches that reaches every one of them with more than eight DISTINCT images, and the inputs / oracle outputs of those batches.

TEST INFRASTRUCTURE, shared by test_jpeg_batch_cases_cpu.py (the table is complete, its inputs can show a wrong image index) and
test_jpeg_batch_gpu.py (the kernels against the oracle).  Nothing here touches a GPU.

The launchers choose by: sampling mode, out_comps, `tuned` (rgba8 needs a dword-aligned base, pitch and image stride), `on_lines` (base,
|pitch| and -- for count > 1 -- |stride| multiples of 128: the NT template variants and JpegArgs.nt), strips of 24 or 32 MCUs,
GAMUT_HIP_JPEG_COLS=plain, dense blocks or tokens.  Every tuned kernel finds its image as blockIdx.z * 8 + (blockIdx.x & 7) and leaves
when that is >= count: 17 images are two full groups of eight, then one image and seven guarded slots."""
import collections
import functools
import io

import numpy as np

import oracle_lib as O

NB = {0: 1, 1: 3, 2: 4, 3: 4, 4: 6}                                   # blocks per MCU
MCU = {0: (8, 8), 1: (8, 8), 2: (16, 8), 3: (8, 16), 4: (16, 16)}     # MCU width, height
ST_NAME = {0: "GRAY", 1: "H1V1", 2: "H2V1", 3: "H1V2"}
ZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
       49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
GUARD = 4096                                                          # bytes in front of and behind every device allocation of a case
HEIGHT = 21                                                           # three MCU rows of 8 / two of 16, the last one partial
COUNT = 17
WIDTHS_ON = (128, 256, 384, 512)                                      # rows of every output format on 128-byte lines
WIDTHS_OFF = tuple(w + 5 for w in WIDTHS_ON)                          # a ragged last MCU; rgba8: a tight pitch = 4 (mod 128)


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def _m24(mcus_per_row):
    """k_jpeg_cols / k_jpeg_cols4: strips of 24 MCUs where they leave fewer idle threads at the end of a row than strips of 32"""
    waste32, waste24 = (32 - mcus_per_row % 32) % 32, (24 - mcus_per_row % 24) % 24
    return waste24 * 32 < waste32 * 24


def variant(scan_type, out_comps, out_addr, pitch, stride, count, w, cols_env, tokens):
    """The kernel instantiation (and, where a kernel reads it, JpegArgs.nt) that jpeg_reconstruct_launch -- tokens: jpeg_reconstruct_tokens_launch --
    starts for these arguments, as the code decides it.  out_addr: the `out` pointer handed over (row 0 of image 0); pitch < 0: bottom-up rows;
    cols_env: the value of GAMUT_HIP_JPEG_COLS (None: unset)."""
    apitch = abs(pitch)
    tuned = 0 < apitch < (1 << 27) and (out_comps != 4 or (out_addr % 4 == 0 and apitch % 4 == 0 and stride % 4 == 0))
    on_lines = ((out_addr | apitch | (abs(stride) if count > 1 else 0)) & 127) == 0
    if tokens:
        assert scan_type == 4
        if not tuned:
            return "error"                                            # the token launcher has no byte-wise kernel behind it: GAMUT_HIP_ERR_INVALID_ARG
        if out_comps == 4:
            return "h2v2<4,TOK,NT>" if on_lines else "h2v2<4,TOK>"
        return f"h2v2<{out_comps},TOK> nt={int(on_lines)}"            # (rgb8 / l8: one instantiation, the packed write-out branches on JpegArgs.nt)
    if not tuned:
        return "generic"
    mw = MCU[scan_type][0]
    mcus_per_row = (w + mw - 1) // mw
    nt = ",NT" if on_lines else ""

    def plain():                                                      # GAMUT_JPEG_PLAIN: rgba8 has the NT form only, whatever the lines
        return f"plain<{ST_NAME[scan_type]},{out_comps}{',NT' if out_comps == 4 else nt}>"
    cols_tuned = cols_env != "plain"
    if scan_type == 0:
        return plain()                                                # grey never reaches the k_jpeg_cols branch behind this one
    if scan_type == 1:
        return f"cols<H1V1,{out_comps},{24 if _m24(mcus_per_row) else 32}{nt}>" if cols_tuned else plain()
    if scan_type in (2, 3):
        return f"cols4<{ST_NAME[scan_type]},{out_comps},{24 if _m24(mcus_per_row) else 32}{nt}>" if cols_tuned else plain()
    if out_comps == 4:
        return "h2v2<4,NT>" if on_lines else "h2v2<4>"
    return f"h2v2<{out_comps}> nt={int(on_lines)}"


def family(name):
    return name.split("<")[0]


# ------------------------------------------------------------------------------------------------ the dense cases
# stride: "lines" = pitch * h rounded up to 128, plus 128; "off" = that + 4 (rgba8: stays on the tuned kernels) / + 1 (rgb8, l8); "odd" = that + 1 for rgba8,
# which must take k_jpeg_generic.  flip: rows bottom-up (a negative pitch).  zag: a max_zag array (its own stride nblk + 3) or NULL.
Case = collections.namedtuple("Case", "scan_type out_comps w count stride flip zag kind cols_env")


def _envs(st):
    return ("cols", "plain") if st in (1, 2, 3) else (None,)


def _cases():
    cases = []
    for st in range(5):
        for oc in (4, 3, 1):
            for zag in (False, True):
                for kind in ("natural", "wild"):
                    for env in _envs(st):
                        for w in WIDTHS_ON:
                            cases.append(Case(st, oc, w, COUNT, "lines", False, zag, kind, env))
                        for w in WIDTHS_OFF:
                            cases.append(Case(st, oc, w, COUNT, "off", False, zag, kind, env))
                        # rows on the lines, images not: on_lines fails by the stride alone
                        cases.append(Case(st, oc, 128, COUNT, "off", False, zag, kind, env))
                    if oc == 4:
                        cases.append(Case(st, 4, 128, COUNT, "odd", False, zag, kind, None))
                        cases.append(Case(st, 4, 133, COUNT, "odd", False, zag, kind, None))
            # bottom-up rows: one batch on the lines, one off them (both strip widths of k_jpeg_cols / k_jpeg_cols4 between them)
            for env in _envs(st):
                cases.append(Case(st, oc, 256, COUNT, "lines", True, True, "natural", env))
                cases.append(Case(st, oc, 389, COUNT, "off", True, True, "natural", env))
    # a full group of eight with nothing behind it, and eight plus one: one variant per kernel family
    for n in (8, 9):
        for zag in (False, True):
            for kind in ("natural", "wild"):
                cases.append(Case(4, 4, 128, n, "lines", False, zag, kind, None))        # h2v2
                cases.append(Case(1, 3, 128, n, "lines", False, zag, kind, "cols"))      # cols
                cases.append(Case(2, 1, 133, n, "off", False, zag, kind, "cols"))        # cols4
                cases.append(Case(0, 4, 133, n, "off", False, zag, kind, None))          # plain
                cases.append(Case(4, 4, 128, n, "odd", False, zag, kind, None))          # generic
    # neighbours share their inputs and their oracle output (input_key, out_comps): see inputs() / expected()
    return sorted(cases, key=lambda c: (c.scan_type, c.w, c.kind, c.zag, c.out_comps, c.count, c.stride, c.flip, str(c.cols_env)))


CASES = _cases()


def nblk(c):
    mw, mh = MCU[c.scan_type]
    return ((c.w + mw - 1) // mw) * ((HEIGHT + mh - 1) // mh) * NB[c.scan_type]


def geometry(c):
    """-> (|pitch|, image stride) in bytes"""
    row = c.w * c.out_comps
    pitch = row if c.w % 128 == 0 else row + (0 if c.out_comps == 4 else 3)
    base = (pitch * HEIGHT + 127) // 128 * 128 + 128
    stride = {"lines": base, "off": base + (4 if c.out_comps == 4 else 1), "odd": base + 1}[c.stride]
    assert c.stride != "odd" or c.out_comps == 4
    return pitch, stride


def case_variant(c, alloc_addr=0):
    """the variant of a case whose output allocation starts at alloc_addr (a multiple of 128, as the GPU test asserts of the real one)"""
    pitch, stride = geometry(c)
    out = alloc_addr + GUARD + ((HEIGHT - 1) * pitch if c.flip else 0)
    return variant(c.scan_type, c.out_comps, out, -pitch if c.flip else pitch, stride, c.count, c.w, c.cols_env, False)


def case_id(c):
    return (f"st{c.scan_type} comps{c.out_comps} {c.w}x{HEIGHT} n={c.count} stride={c.stride}{' flipped' if c.flip else ''} "
            f"max_zag={'yes' if c.zag else 'NULL'} {c.kind} COLS={c.cols_env}")


@functools.lru_cache(maxsize=4)
def _inputs(st, w, kind, zag):
    from test_jpeg_gpu import random_coeffs
    rng = np.random.default_rng([st, w, len(kind), int(zag)])
    mw, mh = MCU[st]
    mx, my = (w + mw - 1) // mw, (HEIGHT + mh - 1) // mh
    n = mx * my * NB[st]
    co = np.stack([random_coeffs(rng, n, kind) for _ in range(COUNT)])          # every image its own draw
    if not zag:
        return co, None
    # classes of the sparse IDCT variants (jpegload.d:295-376); <= 2 is the Col!(1) shortcut, which full-range coefficients tell from the dense form
    mz = rng.choice([1, 2, 2, 2, 3, 4, 6, 10, 20, 36, 64], (COUNT, n)).astype(np.uint8)
    if st == 4:                                                                 # waves (MCU pairs) all of whose Y blocks stay below position 10: the Row!4 / Col!4 passes
        m = mz.reshape(COUNT, my, mx, 6)
        sparse = np.repeat(rng.random((COUNT, my, (mx + 1) // 2)) < 0.4, 2, axis=2)[:, :, :mx]
        low = rng.choice([1, 2, 3, 5, 9, 10], (COUNT, my, mx, 4)).astype(np.uint8)
        m[..., :4] = np.where(sparse[..., None], low, m[..., :4])
    keep = np.arange(64)[None, None, :] < mz[:, :, None]                        # by zig-zag position
    co[:, :, ZAG] = np.where(keep, co[:, :, ZAG], 0)
    return co, mz


def inputs(c):
    """-> coefficients (count, nblk, 64) int16, max_zag (count, nblk) uint8 or None.  Read-only: shared between cases."""
    co, mz = _inputs(c.scan_type, c.w, c.kind, c.zag)
    return co[:c.count], None if mz is None else mz[:c.count]


@functools.lru_cache(maxsize=4)
def _expected(st, w, kind, zag, oc):
    co, mz = _inputs(st, w, kind, zag)
    return np.stack([O.jpeg_reconstruct(w, HEIGHT, 1 if st == 0 else 3, st, co[i], None if mz is None else mz[i], oc) for i in range(COUNT)])


def expected(c):
    """-> the oracle's pixels (count, HEIGHT, w * out_comps).  Read-only: shared between cases."""
    return _expected(c.scan_type, c.w, c.kind, c.zag, c.out_comps)[:c.count]


def slots(count):
    return 8 * ((count + 7) // 8)


def expected_allocation(c):
    """the whole output allocation as it must read after the launch: GUARD, slots(count) image slots `stride` apart, GUARD -- 0xA5 wherever no pixel belongs"""
    pitch, stride = geometry(c)
    exp = expected(c)
    buf = np.full(2 * GUARD + slots(c.count) * stride, 0xA5, np.uint8)
    for i in range(c.count):
        rows = buf[GUARD + i * stride:GUARD + i * stride + pitch * HEIGHT].reshape(HEIGHT, pitch)
        (rows[::-1] if c.flip else rows)[:, :c.w * c.out_comps] = exp[i]
    return buf


def describe_difference(c, got, exp):
    """where two allocations of a case first differ: image, row, column"""
    bad = np.flatnonzero(got != exp)
    if bad.size == 0:
        return None
    pitch, stride = geometry(c)
    k = int(bad[0])
    head = f"{case_id(c)} [{case_variant(c)}]: {bad.size} bytes differ, first at byte {k}: got {got[k:k + 8].tolist()} want {exp[k:k + 8].tolist()} -- "
    if k < GUARD or k >= GUARD + slots(c.count) * stride:
        return head + ("the guard in front" if k < GUARD else "the guard behind")
    img, r = divmod(k - GUARD, stride)
    where = f"image {img}" + (" (a spare slot behind the batch)" if img >= c.count else "")
    row, col = divmod(r, pitch)
    if row >= HEIGHT:
        return head + f"{where}: the gap behind its rows"
    y = HEIGHT - 1 - row if c.flip else row
    if col >= c.w * c.out_comps:
        return head + f"{where} row {y}: the row gap"
    return head + f"{where} row {y} column {col // c.out_comps} (byte {col % c.out_comps} of the pixel)"


# ------------------------------------------------------------------------------------------------ the token cases
TOKEN_SIZES = ((128, 40), (133, 40))
TOKEN_MIN_SCAN = 4096            # jpeg_entropy_kernels.hpp, kSyncMinBytes: a shorter scan takes one lane and keeps the dense blocks
TOKEN_OFFSETS = ("lines", "off4", "irregular")


@functools.lru_cache(maxsize=None)
def token_files(w, h):
    """COUNT distinct baseline 4:2:0 files (quality 90): smooth content under noise strong enough for a scan of >= TOKEN_MIN_SCAN bytes"""
    from PIL import Image
    import gen
    rng = np.random.default_rng([w, h])
    blobs = []
    for i in range(COUNT):
        px = gen.synth_rgb(w, h, 60 + i).astype(np.int32) + rng.integers(-96, 97, (h, w, 3))
        bio = io.BytesIO()
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)).save(bio, "JPEG", quality=90, subsampling=2)
        blobs.append(bio.getvalue())
    return tuple(blobs)


def token_offsets(w, h, comps, form):
    """out_offset of the COUNT files: equal steps on the lines / equal steps 4 bytes off them / steps that change from file to file"""
    base = (w * h * comps + 127) // 128 * 128 + 128
    if form == "lines":
        steps = [base] * COUNT
    elif form == "off4":
        steps = [base + 4] * COUNT
    else:
        steps = [base + 4 * (i % 3) for i in range(COUNT)]
    return np.concatenate([[0], np.cumsum(steps)[:-1]]).astype(np.int64), int(sum(steps))


def token_launches(offs):
    """the runs gamut_hip_jpeg_decode_batch_device cuts COUNT files of one geometry into (jpeg_host.hip, `reconstruct`): a run goes on while the step
    between neighbours equals the step behind its first file -- so steps that change every time still pair the files up.  -> [(first, count, stride)]"""
    runs, i, n = [], 0, len(offs)
    while i < n:
        j = i + 1
        ostride = int(offs[j] - offs[i]) if j < n else 0
        while j < n and int(offs[j] - offs[j - 1]) == ostride and ostride > 0:
            j += 1
        runs.append((i, j - i, ostride if j - i > 1 else 0))
        i = j
    return runs


def token_variants(w, h, comps, form, tokens, alloc_addr=0):
    offs, _ = token_offsets(w, h, comps, form)
    return [variant(4, comps, alloc_addr + GUARD + int(offs[i]), w * comps, stride, n, w, None, tokens) for (i, n, stride) in token_launches(offs)]
