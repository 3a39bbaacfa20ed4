"""The case table of tests/jpeg_batch_cases.py, checked without a GPU: it reaches every kernel instantiation the two JPEG reconstruction
launchers can start, and its inputs are such that a wrong image index or an ignored max_zag changes the expected bytes."""
import hashlib

import numpy as np
import pytest

import jpeg_batch_cases as B
import oracle_lib as O

# Every instantiation jpeg_reconstruct_launch and jpeg_reconstruct_tokens_launch (gamut_amd/csrc/jpeg.hip) can launch, as read from the launchers:
# NT = the template argument (nontemporal stores, rows and images on 128-byte lines); "nt=" = JpegArgs.nt where one instantiation branches on it
# (the packed write-out of the 4:2:0 kernel).  k_jpeg_plain -> rgba8 exists in its NT form only and serves both layouts.  Grey is taken by
# k_jpeg_plain before the k_jpeg_cols branch is tested, so k_jpeg_cols<GRAYSCALE, ...> (12 instantiations) cannot be launched and is not listed.
VARIANTS = """
generic
plain<GRAY,4,NT> plain<GRAY,3,NT> plain<GRAY,3> plain<GRAY,1,NT> plain<GRAY,1>
plain<H1V1,4,NT> plain<H1V1,3,NT> plain<H1V1,3> plain<H1V1,1,NT> plain<H1V1,1>
plain<H2V1,4,NT> plain<H2V1,3,NT> plain<H2V1,3> plain<H2V1,1,NT> plain<H2V1,1>
plain<H1V2,4,NT> plain<H1V2,3,NT> plain<H1V2,3> plain<H1V2,1,NT> plain<H1V2,1>
cols<H1V1,4,24,NT> cols<H1V1,4,24> cols<H1V1,4,32,NT> cols<H1V1,4,32>
cols<H1V1,3,24,NT> cols<H1V1,3,24> cols<H1V1,3,32,NT> cols<H1V1,3,32>
cols<H1V1,1,24,NT> cols<H1V1,1,24> cols<H1V1,1,32,NT> cols<H1V1,1,32>
cols4<H2V1,4,24,NT> cols4<H2V1,4,24> cols4<H2V1,4,32,NT> cols4<H2V1,4,32>
cols4<H2V1,3,24,NT> cols4<H2V1,3,24> cols4<H2V1,3,32,NT> cols4<H2V1,3,32>
cols4<H2V1,1,24,NT> cols4<H2V1,1,24> cols4<H2V1,1,32,NT> cols4<H2V1,1,32>
cols4<H1V2,4,24,NT> cols4<H1V2,4,24> cols4<H1V2,4,32,NT> cols4<H1V2,4,32>
cols4<H1V2,3,24,NT> cols4<H1V2,3,24> cols4<H1V2,3,32,NT> cols4<H1V2,3,32>
cols4<H1V2,1,24,NT> cols4<H1V2,1,24> cols4<H1V2,1,32,NT> cols4<H1V2,1,32>
h2v2<4,NT> h2v2<4>
h2v2<3>|nt=1 h2v2<3>|nt=0
h2v2<1>|nt=1 h2v2<1>|nt=0
h2v2<4,TOK,NT> h2v2<4,TOK>
h2v2<3,TOK>|nt=1 h2v2<3,TOK>|nt=0
h2v2<1,TOK>|nt=1 h2v2<1,TOK>|nt=0
"""
VARIANTS = {v.replace("|", " ") for v in VARIANTS.split()}


def _token_variants(tokens):
    return {v for (w, h) in B.TOKEN_SIZES for comps in (4, 3, 1) for form in B.TOKEN_OFFSETS for v in B.token_variants(w, h, comps, form, tokens)}


def test_the_table_reaches_every_variant_the_launchers_can_start():
    assert len(VARIANTS) == 69
    dense = {B.case_variant(c) for c in B.CASES}
    tok = _token_variants(True)
    assert "error" not in tok
    assert dense | tok == VARIANTS, (sorted(VARIANTS - dense - tok), sorted((dense | tok) - VARIANTS))
    assert dense == {v for v in VARIANTS if "TOK" not in v} and tok == {v for v in VARIANTS if "TOK" in v}
    # ... each with 17 images: two full groups of eight, then one image and seven guarded slots
    assert {B.case_variant(c) for c in B.CASES if c.count == B.COUNT} == dense
    # the files of the token cases under GAMUT_HIP_JPEG_HANDOFF=dense: 4:2:0 only
    assert _token_variants(False) == {v for v in dense if v.startswith("h2v2")}
    # 8 and 9 images: one variant of every kernel family
    for n in (8, 9):
        assert {B.family(B.case_variant(c)) for c in B.CASES if c.count == n} == {"h2v2", "cols", "cols4", "plain", "generic"}
    # bottom-up rows: on and off the lines, every sampling mode
    for st in range(5):
        flipped = [c for c in B.CASES if c.flip and c.scan_type == st]
        assert {c.count for c in flipped} == {B.COUNT} and {c.w % 128 == 0 for c in flipped} == {True, False}


def test_the_mirror_on_known_launches():
    """launches whose kernel the launcher's text states outright"""
    v = B.variant
    assert v(4, 4, 0, 1920 * 4, 1920 * 1080 * 4, 1024, 1920, None, False) == "h2v2<4,NT>"          # bench.py's headline
    assert v(4, 4, 0, 1366 * 4, 1366 * 768 * 4, 2, 1366, None, False) == "h2v2<4>"
    assert v(4, 4, 1, 1920 * 4, 0, 1, 1920, None, False) == "generic" and v(4, 4, 0, 1920 * 4, 1920 * 1080 * 4 + 1, 2, 1920, None, False) == "generic"
    assert v(4, 3, 1, 1920 * 3, 5, 3, 1920, None, False) == "h2v2<3> nt=0"                         # rgb8 rows may start anywhere
    assert v(1, 4, 0, 1920 * 4, 0, 1, 1920, None, False) == "cols<H1V1,4,24,NT>"                   # 1080p: 240 MCUs = 10 x 24
    assert v(1, 4, 0, 1024 * 4, 64, 1, 1024, None, False) == "cols<H1V1,4,32,NT>"                  # one image: its stride does not count
    assert v(1, 4, 0, 1024 * 4, 64, 2, 1024, None, False) == "cols<H1V1,4,32>"
    assert v(1, 3, 0, -1024 * 3, 1024 * 3 * 8, 2, 1024, "plain", False) == "plain<H1V1,3,NT>"
    assert v(0, 4, 4, 400, 0, 1, 100, "cols", False) == "plain<GRAY,4,NT>" and v(0, 1, 4, 100, 0, 1, 100, None, False) == "plain<GRAY,1>"
    assert v(2, 1, 0, 512, 512 * 21, 17, 512, None, False) == "cols4<H2V1,1,32,NT>" and v(3, 1, 0, 512, 512 * 21, 17, 512, None, False) == "cols4<H1V2,1,32,NT>"
    assert v(4, 4, 0, 512, 0, 1, 128, None, True) == "h2v2<4,TOK,NT>" and v(4, 4, 2, 512, 0, 1, 128, None, True) == "error"
    # steps that change from file to file still pair the files up: the run test compares a step with the one behind the run's first file
    assert B.token_launches(np.array([0, 100, 204, 312, 412])) == [(0, 2, 100), (2, 2, 108), (4, 1, 0)]
    assert B.token_launches(np.arange(17) * 128) == [(0, 17, 128)]


def _key(c):
    return (c.scan_type, c.w, c.kind, c.zag, c.out_comps)


@pytest.mark.parametrize("scan_type", [0, 1, 2, 3, 4])
def test_the_images_of_a_batch_differ_and_max_zag_shows(scan_type):
    """a condition on the INPUTS: the oracle's pixels of any two images of a batch differ (else a kernel that took image j for image i would pass), and where
    a case passes max_zag the oracle's pixels with it differ from those without, for at least one image (else a kernel that read another image's
    max_zag, or none, would pass)"""
    seen = set()
    for c in B.CASES:
        if c.scan_type != scan_type or _key(c) in seen:
            continue
        seen.add(_key(c))
        co, mz = B.inputs(c._replace(count=B.COUNT))
        exp = B.expected(c._replace(count=B.COUNT))
        assert len({hashlib.sha256(e.tobytes()).digest() for e in exp}) == B.COUNT, B.case_id(c)
        assert len({hashlib.sha256(e.tobytes()).digest() for e in co}) == B.COUNT
        if mz is not None:
            assert len({hashlib.sha256(e.tobytes()).digest() for e in mz}) == B.COUNT
        # (the sparse IDCT variants differ from the dense one by 32-bit wrap-around only -- jpegload.d:295-376 -- which "natural" magnitudes never reach: their
        #  max_zag cases run the sparse passes on ordinary data, the "wild" ones -- every mode, width and output format has one, see below -- carry this condition)
        if mz is not None and c.kind == "wild":
            comps = 1 if scan_type == 0 else 3
            differ = [i for i in range(B.COUNT) if not np.array_equal(O.jpeg_reconstruct(c.w, B.HEIGHT, comps, scan_type, co[i], None, c.out_comps), exp[i])]
            assert differ, B.case_id(c)
            # ... the first group of eight alone shows it too (the batches of 8 and 9 images)
            assert [i for i in differ if i < 8], B.case_id(c)
    for (st, w, kind, zag, oc) in list(seen):
        assert (st, w, "wild", True, oc) in seen and (st, w, "wild", False, oc) in seen and (st, w, "natural", zag, oc) in seen
    # ... and every variant has a case whose max_zag shows
    assert {B.case_variant(c) for c in B.CASES if c.scan_type == scan_type} == {B.case_variant(c) for c in B.CASES if c.scan_type == scan_type and c.zag and c.kind == "wild"}


def test_the_token_files_are_distinct_and_long_enough_for_tokens():
    """17 distinct files per size whose pixels differ pairwise, each with a scan of at least kSyncMinBytes (jpeg_entropy_kernels.hpp): shorter scans keep the dense blocks
    whatever GAMUT_HIP_JPEG_HANDOFF says"""
    for (w, h) in B.TOKEN_SIZES:
        blobs = B.token_files(w, h)
        px = [O.decompress_jpeg(b, 4) for b in blobs]
        assert all(p is not None and p[0].shape == (h, w * 4) for p in px)
        assert len({hashlib.sha256(p[0].tobytes()).digest() for p in px}) == B.COUNT
        for b in blobs:
            d = O.DecodedJpeg(b)
            assert d.scan_type == O.JPGD_YH2V2 and b"\xff\xdd" not in b[:b.index(b"\xff\xda")]          # 4:2:0, no restart interval: one segment
            assert len(b) - (b.index(b"\xff\xda") + 14) - 2 >= B.TOKEN_MIN_SCAN, (w, h, len(b))           # behind the SOS header, in front of EOI
