"""The case table of tests/png_batch_cases.py, checked without a GPU: it reaches every kernel combination png_defilter_launch can start, each with several
distinct images, and its inputs are such that a wrong image index changes the expected bytes."""
import numpy as np
import pytest

import png_batch_cases as B

# Everything png_defilter_launch (gamut_amd/csrc/png.hip) can launch, as read from the launcher: the de-filter kernel with its template flags (FB first; RGBA =
# the alpha-inserting walk, AL = line-aligned loads, LN = every row on a 128-byte line of its own), and behind a "+" the expand kernel of the scratch route.
#   * fused rows (8-bit, out_n == img_n, FB 1..4, or RGB8 -> RGBA8) lie where the caller says: all four AL / LN combinations; RGBA excludes AL.
#   * scratch rows have a pitch the launcher rounds to 128 in a scratch of its own: LN always.  FB 6 and 8 (16-bit RGB / RGBA) are never fused, so
#     k_png_defilter_ring<6 | 8, ..., AL, false> and <6 | 8, ..., false, false>, and the same four of k_png_defilter_queue, are compiled but cannot be launched
#     (eight instantiations); every k_png_defilter_rollq, k_png_defilter and k_png_expand_vec instantiation can.
#   * the scalar k_png_expand takes the sub-byte depths and grey + alpha -> 3 channels (8 and 16 bit), which k_png_expand_vec has no instantiation for
#     (and every batch of more than 65 535 images: test_png_batch_gpu.py).
# Row segments (" seg=N") are a property of the launch, not another kernel: SEGMENTED lists the de-filter kernels the table must cut into segments.
VARIANTS = """
ring<1,AL,LN> ring<1,AL> ring<1,LN> ring<1> queue<1,AL,LN> queue<1,AL> queue<1,LN> queue<1> rollq<1> lane<1>
ring<2,AL,LN> ring<2,AL> ring<2,LN> ring<2> queue<2,AL,LN> queue<2,AL> queue<2,LN> queue<2> rollq<2> lane<2>
ring<3,AL,LN> ring<3,AL> ring<3,LN> ring<3> queue<3,AL,LN> queue<3,AL> queue<3,LN> queue<3> rollq<3> lane<3>
ring<4,AL,LN> ring<4,AL> ring<4,LN> ring<4> queue<4,AL,LN> queue<4,AL> queue<4,LN> queue<4> rollq<4> lane<4>
ring<3,RGBA,LN> ring<3,RGBA> queue<3,RGBA,LN> queue<3,RGBA>
ring<1,AL,LN>+expand ring<1,LN>+expand queue<1,AL,LN>+expand queue<1,LN>+expand rollq<1>+expand lane<1>+expand
ring<1,AL,LN>+expand_vec<1,1,1> ring<1,LN>+expand_vec<1,1,1> queue<1,AL,LN>+expand_vec<1,1,1> queue<1,LN>+expand_vec<1,1,1> rollq<1>+expand_vec<1,1,1> lane<1>+expand_vec<1,1,1>
ring<1,AL,LN>+expand_vec<1,2,1> ring<1,LN>+expand_vec<1,2,1> queue<1,AL,LN>+expand_vec<1,2,1> queue<1,LN>+expand_vec<1,2,1> rollq<1>+expand_vec<1,2,1> lane<1>+expand_vec<1,2,1>
ring<2,AL,LN>+expand_vec<1,1,2> ring<2,LN>+expand_vec<1,1,2> queue<2,AL,LN>+expand_vec<1,1,2> queue<2,LN>+expand_vec<1,1,2> rollq<2>+expand_vec<1,1,2> lane<2>+expand_vec<1,1,2>
ring<2,AL,LN>+expand_vec<1,2,2> ring<2,LN>+expand_vec<1,2,2> queue<2,AL,LN>+expand_vec<1,2,2> queue<2,LN>+expand_vec<1,2,2> rollq<2>+expand_vec<1,2,2> lane<2>+expand_vec<1,2,2>
ring<2,AL,LN>+expand_vec<2,2,1> ring<2,LN>+expand_vec<2,2,1> queue<2,AL,LN>+expand_vec<2,2,1> queue<2,LN>+expand_vec<2,2,1> rollq<2>+expand_vec<2,2,1> lane<2>+expand_vec<2,2,1>
ring<2,AL,LN>+expand ring<2,LN>+expand queue<2,AL,LN>+expand queue<2,LN>+expand rollq<2>+expand lane<2>+expand
ring<4,AL,LN>+expand_vec<2,2,2> ring<4,LN>+expand_vec<2,2,2> queue<4,AL,LN>+expand_vec<2,2,2> queue<4,LN>+expand_vec<2,2,2> rollq<4>+expand_vec<2,2,2> lane<4>+expand_vec<2,2,2>
ring<4,AL,LN>+expand ring<4,LN>+expand queue<4,AL,LN>+expand queue<4,LN>+expand rollq<4>+expand lane<4>+expand
ring<3,AL,LN>+expand_vec<3,3,1> ring<3,LN>+expand_vec<3,3,1> queue<3,AL,LN>+expand_vec<3,3,1> queue<3,LN>+expand_vec<3,3,1> rollq<3>+expand_vec<3,3,1> lane<3>+expand_vec<3,3,1>
ring<3,AL,LN>+expand_vec<3,4,1> ring<3,LN>+expand_vec<3,4,1> queue<3,AL,LN>+expand_vec<3,4,1> queue<3,LN>+expand_vec<3,4,1> rollq<3>+expand_vec<3,4,1> lane<3>+expand_vec<3,4,1>
ring<6,AL,LN>+expand_vec<3,3,2> ring<6,LN>+expand_vec<3,3,2> queue<6,AL,LN>+expand_vec<3,3,2> queue<6,LN>+expand_vec<3,3,2> rollq<6>+expand_vec<3,3,2> lane<6>+expand_vec<3,3,2>
ring<6,AL,LN>+expand_vec<3,4,2> ring<6,LN>+expand_vec<3,4,2> queue<6,AL,LN>+expand_vec<3,4,2> queue<6,LN>+expand_vec<3,4,2> rollq<6>+expand_vec<3,4,2> lane<6>+expand_vec<3,4,2>
ring<4,AL,LN>+expand_vec<4,4,1> ring<4,LN>+expand_vec<4,4,1> queue<4,AL,LN>+expand_vec<4,4,1> queue<4,LN>+expand_vec<4,4,1> rollq<4>+expand_vec<4,4,1> lane<4>+expand_vec<4,4,1>
ring<8,AL,LN>+expand_vec<4,4,2> ring<8,LN>+expand_vec<4,4,2> queue<8,AL,LN>+expand_vec<4,4,2> queue<8,LN>+expand_vec<4,4,2> rollq<8>+expand_vec<4,4,2> lane<8>+expand_vec<4,4,2>
"""
VARIANTS = {v.replace("+", " + ") for v in VARIANTS.split()}
SEGMENTED = """
ring<1,AL,LN> ring<1,AL> ring<1,LN> ring<1> ring<2,AL,LN> ring<2,AL> ring<2,LN> ring<2> ring<3,AL,LN> ring<3,AL> ring<3,LN> ring<3>
ring<4,AL,LN> ring<4,AL> ring<4,LN> ring<4> ring<6,AL,LN> ring<6,LN> ring<8,AL,LN> ring<8,LN> ring<3,RGBA,LN> ring<3,RGBA>
lane<1> lane<2> lane<3> lane<4> lane<6> lane<8>
"""
SEGMENTED = set(SEGMENTED.split())
EXPAND_VEC = {f"expand_vec<{i},{o},{b}>" for (i, o) in ((1, 1), (1, 2), (2, 2), (3, 3), (3, 4), (4, 4)) for b in (1, 2)}


def _reached(cases):
    return {B.without_segments(B.case_variant(c)) for c in cases}


def test_the_table_reaches_every_variant_the_launcher_can_start():
    assert len(VARIANTS) == 134 and len(SEGMENTED) == 28 and len(EXPAND_VEC) == 12
    reached = _reached(B.CASES)
    assert reached == VARIANTS, (sorted(VARIANTS - reached), sorted(reached - VARIANTS))
    # ... each with five images, all distinct (below), and without an invalid filter byte in the way; 3, 4 and 7 images besides
    five = _reached(c for c in B.CASES if c.count == 5 and not c.bad)
    assert five == VARIANTS, sorted(VARIANTS - five)
    assert {c.count for c in B.CASES} == {3, 4, 5, 7}
    # every format with more than one image, with out_n = img_n and with out_n = img_n + 1 where the launcher takes it
    pairs = {(c.img_n, c.depth, c.color, c.out_n) for c in B.CASES if c.count > 1}
    assert pairs == {(n, d, col, o) for (n, d, col) in B.FORMATS for o in ([n, n + 1] if n < 4 else [n])} and len(B.FORMATS) == 15
    # row segments: every ring and per-lane kernel, with 3 and with 7 images, two segments an image at 300 rows, with filter patterns made for them
    # (the batches of 518 rows are cut in four wherever their ordinary filters allow it: the launcher does that to every small batch outside the queue)
    seg = [c for c in B.CASES if B.segments(B.case_variant(c)) > 1]
    assert {(c.y, B.segments(B.case_variant(c))) for c in seg} == {(300, 2), (518, 4)}
    cuts = [c for c in B.CASES if c.filt == "cuts"]
    assert {c.y for c in cuts} == {300} and {c.count for c in cuts} == {3, 7} and all(c in seg for c in cuts)
    for n in (3, 7):
        assert {B.family(B.case_variant(c)) for c in cuts if c.count == n} == {"ring", "lane"}
        assert {(c.img_n, c.depth, c.color, c.out_n) for c in cuts if c.count == n} == pairs
    assert {B.defilter_kernel(B.case_variant(c)) for c in cuts} == SEGMENTED
    # the expand kernels, the per-lane kernel, the rolling queue and more bands than a workgroup has waves: all there, each family
    kernels = {v.split(" + ")[1] for v in reached if " + " in v}
    assert kernels == EXPAND_VEC | {"expand"}
    families = {"ring", "queue", "rollq", "lane"}
    assert {B.family(v) for v in reached} == families
    assert {B.family(B.case_variant(c)) for c in B.CASES if c.y == 518} == families and (518 + 63) // 64 > B.PNG_WAVES
    for bad in ("status", "null"):
        assert {B.family(B.case_variant(c)) for c in B.CASES if c.bad == bad} == families
        assert any(B.segments(B.case_variant(c)) > 1 for c in B.CASES if c.bad == bad)
        assert {" + " in B.case_variant(c) for c in B.CASES if c.bad == bad} == {True, False}
    # every switch setting and every layout is used, and the case ids are unique
    assert {c.mode for c in B.CASES} == set(B.MODES) and {c.layout for c in B.CASES} == set(B.LAYOUTS)
    assert len({B.case_id(c) for c in B.CASES}) == len(B.CASES)


def test_the_widths_are_the_ones_the_kernels_can_go_wrong_at():
    for (img_n, depth, color) in B.FORMATS:
        w = B.widths(img_n, depth)
        wb = {k: B.row_bytes(x, img_n, depth) for k, x in w.items()}
        assert wb["lines"] % 128 == 0 and wb["lines"] >= 256
        assert wb["ragged"] > 2 * 128 and wb["ragged"] % 128 and wb["ragged"] % 16                    # two whole groups and a tail
        assert 0 < wb["lane"] < 16
        if depth < 8:
            assert (w["ragged"] * depth) % 8 and (w["lane"] * depth) % 8                              # a partly filled last byte
            assert wb["lane"] <= w["lane"]                                                            # (the launcher's "invalid width" test)
        if "dwords" in w:
            assert wb["ragged"] % 4 and wb["dwords"] % 4 == 0 and wb["dwords"] % 16 and wb["dwords"] > 256 and wb["lane4"] % 4 == 0 and wb["lane4"] < 16


def test_the_layouts_flip_the_variant_as_the_mirror_says():
    def names(img_n, depth, out_n, x, mode):
        cs = [c for c in B.CASES if (c.img_n, c.depth, c.out_n, c.x, c.y, c.mode, c.color) == (img_n, depth, out_n, x, 70, mode, {1: 0, 2: 4, 3: 2, 4: 6}[img_n])]
        return {c.layout: B.case_variant(c) for c in cs}
    assert names(4, 8, 4, 64, "workgroups+aligned") == {"lines": "ring<4,AL,LN>", "stride+16": "ring<4,AL>", "stride+4": "ring<4>",
                                                         "stride+1": "ring<4,AL,LN> + expand_vec<4,4,1>", "out+4": "ring<4>"}
    assert names(4, 8, 4, 64, "default") == names(4, 8, 4, 64, "workgroups+aligned")                  # 256-byte rows: the launcher's own rule
    assert names(4, 8, 4, 64, "queue") == {"lines": "queue<4,LN>", "stride+16": "queue<4>", "stride+4": "queue<4>",
                                            "stride+1": "queue<4,LN> + expand_vec<4,4,1>", "out+4": "queue<4>"}
    assert names(3, 8, 4, 128, "queue+aligned") == {"lines": "queue<3,RGBA,LN>", "stride+16": "queue<3,RGBA>", "stride+4": "queue<3,RGBA>",
                                                     "stride+1": "queue<3,AL,LN> + expand_vec<3,4,1>", "out+4": "queue<3,RGBA>"}
    assert names(3, 8, 4, 128, "queue+roll")["lines"] == "queue<3,RGBA,LN>"                           # the rolling form has no alpha-inserting walk
    assert set(names(4, 8, 4, 64, "queue+roll").values()) == {"rollq<4>", "rollq<4> + expand_vec<4,4,1>"}
    assert set(names(4, 16, 4, 32, "workgroups").values()) == {"ring<8,LN> + expand_vec<4,4,2>"}       # the scratch route: the layout of `out` does not count
    assert names(1, 8, 1, 256, "queue+aligned")["stride+16"] == "queue<1,AL>" and names(2, 8, 2, 128, "workgroups")["out+4"] == "ring<2>"


def test_the_mirror_on_known_launches():
    """launches whose kernels the launcher's text (or a test that relies on it) states outright"""
    v = B.variant
    # bench config 3: 512 tight 4K RGBA8 images: k_png_defilter_queue<4, 8, 2, false, true, true>
    assert v(3840, 2160, 4, 4, 8, 512, 0, 3840 * 2160 * 4) == "queue<4,AL,LN>"
    assert v(3840, 2160, 4, 4, 8, 511, 0, 3840 * 2160 * 4) == "queue<4,AL,LN>" and v(1920, 1080, 4, 4, 8, 61, 0, 1920 * 1080 * 4) == "queue<4,AL,LN>"
    assert v(1920, 1080, 4, 4, 8, 60, 0, 1920 * 1080 * 4) == "ring<4,AL,LN> seg=8"                   # 60 x 17 bands: four units short of the queue
    # a single 4K image: 34 bands, below the queue's threshold ("a 4K image alone keeps one workgroup busy for 34 bands"): row segments, as many as
    # leave 128 rows each and at most eight -- 2160 / 8 = 270
    assert v(3840, 2160, 4, 4, 8, 1, 0, 0) == "ring<4,AL,LN> seg=8" and v(3840, 1000, 4, 4, 8, 1, 0, 0) == "ring<4,AL,LN> seg=7"
    assert v(3840, 2160, 4, 4, 8, 1, 0, 0, queue_env="1") == "queue<4,AL,LN>" and v(3840, 2160, 4, 4, 8, 1, 0, 0, queue_env="1", roll_env="1") == "rollq<4>"
    assert v(3840, 2160, 4, 4, 8, 8, 0, 3840 * 2160 * 4, queue_env="0") == "ring<4,AL,LN> seg=8" and v(64, 255, 4, 4, 8, 1, 0, 0) == "ring<4,AL,LN>"
    assert v(64, 1000, 4, 4, 8, 3, 0, 64 * 1000 * 4 + 64) == "ring<4,AL> seg=7" and v(97, 256, 4, 4, 8, 1, 0, 0) == "ring<4> seg=2"    # (388-byte rows: no multiple of 16)
    # test_rows_off_the_memory_lines: x = 962 RGB8 -> RGB8 has rows of 2886 bytes, no dword multiple: the scratch and expand_vec<3,3,1>
    assert v(962, 200, 3, 3, 8, 3, 0, 962 * 200 * 3 + 64) == "ring<3,AL,LN> + expand_vec<3,3,1>"
    assert v(1004, 131, 3, 3, 8, 3, 0, 1004 * 131 * 3 + 64) == "ring<3>"                              # 3012-byte rows: fused, off the lines, no multiple of 16
    # RGB8 -> RGBA8 is fused only into a dword-aligned output
    assert v(962, 200, 3, 4, 8, 3, 0, 962 * 200 * 4 + 64) == "ring<3,RGBA>" and v(960, 200, 3, 4, 8, 1, 0, 0) == "ring<3,RGBA,LN>"
    assert v(962, 200, 3, 4, 8, 3, 1, 962 * 200 * 4 + 64) == "ring<3,AL,LN> + expand_vec<3,4,1>"
    assert v(962, 200, 3, 4, 8, 3, 0, 962 * 200 * 4 + 65) == "ring<3,AL,LN> + expand_vec<3,4,1>"
    assert v(5, 200, 3, 4, 8, 3, 0, 4000) == "lane<3> + expand_vec<3,4,1>"                            # rows under 16 bytes
    # offset tables: the two flags stand in for the stride
    assert v(203, 131, 3, 4, 8, 5, 0, 0, offs=True, offs_dword_aligned=True) == "ring<3,RGBA>" and v(203, 131, 3, 4, 8, 5, 0, 0, offs=True) == "ring<3,AL,LN> + expand_vec<3,4,1>"
    assert v(64, 70, 4, 4, 8, 5, 0, 0, offs=True, offs_dword_aligned=True, offs_line_aligned=True) == "ring<4,AL,LN>"
    assert v(64, 70, 4, 4, 8, 5, 0, 0, offs=True, offs_dword_aligned=True) == "ring<4>"
    # more images than a grid dimension holds: the vector expand is not asked
    assert v(2, 2, 2, 2, 16, 65537, 0, 16) == "lane<4> + expand" and v(2, 2, 2, 2, 16, 65535, 0, 16) == "lane<4> + expand_vec<2,2,2>"
    assert v(8, 2, 1, 1, 1, 65537, 0, 19) == "lane<1> + expand"
    # the queue's own threshold: 1024 (image, band) units, rows of at least one piece
    assert v(67, 70, 4, 4, 8, 512, 0, 67 * 70 * 4) == "queue<4>" and v(67, 70, 4, 4, 8, 511, 0, 67 * 70 * 4) == "ring<4>" and v(3, 70, 4, 4, 8, 512, 0, 3 * 70 * 4) == "lane<4>"


@pytest.mark.parametrize("fmt", range(len(B.FORMATS)))
def test_the_images_of_a_batch_differ_and_the_oracle_returns_the_source(fmt):
    """conditions on the INPUTS: the oracle's output of any two images of a batch differs in at least half of the rows (else a kernel that took image j for image i
    could pass); where nothing is inserted and samples are whole bytes the oracle's output is the samples the streams were made from (PNG is lossless: the oracle
    against data it did not produce); the row filters differ between the images of a batch; a damaged stream is refused by the oracle"""
    seen = set()
    for c in B.CASES:
        key = (c.img_n, c.depth, c.color, c.out_n, c.x, c.y, c.count, c.filt)
        if (c.img_n, c.depth, c.color) != B.FORMATS[fmt] or key in seen:
            continue
        seen.add(key)
        samples, filters, raws = B.inputs(c)
        exp = B.expected(c)
        assert len(exp) == c.count and all(e.size == B.image_bytes(c) for e in exp)
        rows = [e.reshape(c.y, -1) for e in exp]
        for i in range(c.count):
            for j in range(i + 1, c.count):
                assert np.count_nonzero((rows[i] != rows[j]).any(axis=1)) * 2 >= c.y, (B.case_id(c), i, j)
        assert len({f.tobytes() for f in filters}) == c.count, B.case_id(c)
        assert all(f.max() <= 4 for f in filters)
        if c.out_n == c.img_n and c.depth >= 8:
            for i in range(c.count):
                src = samples[i].astype(np.uint8 if c.depth == 8 else "<u2").view(np.uint8).reshape(-1)
                assert np.array_equal(exp[i], src), (B.case_id(c), i)
        if c.filt == "cuts":                                                                          # the patterns the segment cases are there for
            lo, hi = c.y // 2 - (c.y // 4 - 1), c.y // 2 + (c.y // 4 - 1)
            cut = [np.flatnonzero(f[lo:hi + 1] <= 1) + lo for f in filters]
            assert cut[0].tolist() == [c.y // 2 + 3] and cut[1].tolist() == [c.y // 2 - 1, c.y // 2 + 40]
            assert cut[2].size == 0 and (filters[2] <= 1).sum() == 3                                  # cut rows, none of them within reach of the boundary
            if c.count > 3:
                assert (filters[3] <= 1).sum() == 0 and cut[4].tolist() == [c.y // 2] and cut[5].size > 3
        else:
            kinds = [np.unique(f).tolist() for f in filters]
            assert [4] in kinds and [0] in kinds or c.count < 5, B.case_id(c)
    for c in B.CASES:
        if c.bad and (c.img_n, c.depth, c.color) == B.FORMATS[fmt]:
            img, at = B.bad_position(c)
            raws = B.raw_streams(c)
            assert raws[img][at] == 9 and at % (B.row_bytes(c.x, c.img_n, c.depth) + 1) == 0 and 0 < img < c.count - 1
            assert B.O.png_create_image_raw(raws[img], c.img_n, c.out_n, c.x, c.y, c.depth, c.color) is None
            assert all(np.array_equal(raws[i], B.inputs(c)[2][i]) for i in range(c.count) if i != img)


def test_expected_allocation_and_describe_difference():
    c = next(c for c in B.CASES if (c.img_n, c.depth, c.out_n, c.layout, c.mode, c.y, c.bad) == (4, 8, 4, "out+4", "workgroups", 70, None) and c.x == 64)
    exp, mask = B.expected_allocation(c)
    shift, stride = B.geometry(c)
    assert (shift, stride % 128, exp.size) == (4, 0, 2 * B.GUARD + 7 * stride) and mask.all()
    n = B.image_bytes(c)
    assert (exp[:B.GUARD + 4] == 0xA5).all() and (exp[B.GUARD + 4 + 4 * stride + n:] == 0xA5).all() and np.array_equal(exp[B.GUARD + 4 + stride:][:n], B.expected(c)[1])
    assert B.describe_difference(c, exp, exp) is None
    got = exp.copy(); got[B.GUARD + 4 + 3 * stride + 256 * 9 + 4 * 5 + 2] ^= 1
    assert "image 3 row 9 column 5 (byte 2" in B.describe_difference(c, got, exp) and "ring<4>" in B.describe_difference(c, got, exp)
    got = exp.copy(); got[B.GUARD + 4 + 2 * stride + n] = 0
    assert "image 2: the gap behind its rows" in B.describe_difference(c, got, exp)
    got = exp.copy(); got[B.GUARD + 4 + 5 * stride + 1] = 0
    assert "image 5 (a spare slot" in B.describe_difference(c, got, exp)
    got = exp.copy(); got[7] = 0
    assert "guard in front" in B.describe_difference(c, got, exp)
    got = exp.copy(); got[-1] = 0
    assert "guard behind" in B.describe_difference(c, got, exp)
    b = next(c for c in B.CASES if c.bad == "status")
    exp, mask = B.expected_allocation(b)
    assert np.count_nonzero(~mask) == B.image_bytes(b)
    got = exp.copy(); got[~mask] ^= 0xFF
    assert B.describe_difference(b, got, exp, mask) is None and B.describe_difference(b, got, exp) is not None


def test_the_offset_tables_flip_the_variant_as_the_mirror_says():
    """the four forms of out_offset of test_offset_tables_on_and_off_the_lines: today both `lines` and `rows16` of a table launch follow offs_line_aligned"""
    rgb4, rgba, grey2, rgba16, rgb3 = B.TABLE_FORMATS
    for form in B.TABLE_FORMS:
        sizes = [17920, 17920, 17920, 1440, 17920, 17920]
        offs, span = B.table_offsets(sizes, form)
        assert all(b - a >= n for a, b, n in zip(offs[:-1], offs[1:], sizes)) and offs[-1] + sizes[-1] <= span and len(set(np.diff(offs).tolist())) > 2
        assert {"lines": all(o % 128 == 0 for o in offs), "16": all(o % 16 == 0 and o % 128 for o in offs),
                "4": all(o % 4 == 0 for o in offs) and any(o % 16 for o in offs), "odd": all(o % 2 for o in offs)}[form]
    t = B.table_variant
    assert [t(rgba, f) for f in B.TABLE_FORMS] == ["ring<4,AL,LN>", "ring<4>", "ring<4>", "ring<4,AL,LN> + expand_vec<4,4,1>"]
    assert [t(rgb4, f) for f in B.TABLE_FORMS] == ["ring<3,RGBA,LN>", "ring<3,RGBA>", "ring<3,RGBA>", "ring<3,LN> + expand_vec<3,4,1>"]
    assert {t(grey2, f) for f in B.TABLE_FORMS} == {"ring<1,LN> + expand_vec<1,2,1>"} and {t(rgba16, f) for f in B.TABLE_FORMS} == {"ring<8,AL,LN> + expand_vec<4,4,2>"}
    assert {t(rgb3, f) for f in B.TABLE_FORMS} == {"ring<3,LN> + expand_vec<3,3,1>"}
    assert t(rgba, "lines", out_addr=4) == "ring<4>" and t(rgba, "lines", x=40, y=9, count=1) == "ring<4>"             # the odd-sized file: 160-byte rows
