"""The hand-built baseline scans of tests/jpeg_scan_cases.py on the CPU: three readings of every file -- the plain T.81 decoder of
tests/jpeg_scan_ref.py, the oracle (O.DecodedJpeg: coefficients and max_zag) and the product's host feeder (gamut_hip_jpeg_decode_coeffs) -- and
the census that proves each case stands on what its name says.  -m gpu: tests/test_jpeg_scan_cases_gpu.py runs the same files through the
device decoders.

Cases whose verdict the oracle alone decided (nobody had run such streams against it before; the names say what it does):
  * three_non_interleaved_scans_no_defined_result_in_the_reference: T.81 defines a sequential frame of one scan per component; the reference's
    sequential path is made for ONE interleaved scan and runs a single-component scan over MCU buffers of another size -- `undefined`, not the
    `image` one would expect; the library refuses the file.
  * eight_prefixes_...: the table has 255 code words, not 256 -- the reference refuses a DHT that lists more than 255."""
import collections
import ctypes as C

import numpy as np
import pytest

import jpeg_scan_cases as S
import jpeg_scan_ref as R
import oracle_lib as O
from gamut_amd import _capi

CASES = S.corpus()
IDS = [c.name for c in CASES]
G = S.geometry()


@pytest.fixture(scope="module")
def decoded():
    """the plain decoder's reading of every well-formed case, made once (the phase-locked ones with the trace the lock census needs)"""
    return {c.name: R.decode(c.data, trace=c.family == "phase") for c in CASES if c.wellformed}


def oracle(data):
    buf = np.frombuffer(data, np.uint8)
    f = O.JpegFrame()
    rc = O.lib().orc_jpeg_decode_coeffs(O._ptr(buf), buf.size, C.byref(f))
    if rc != 0:
        return rc, None, None
    n = f.mcus_per_row * f.mcus_per_col * f.blocks_per_mcu
    co = np.ctypeslib.as_array(f.coeffs, (n, 64)).copy(); mz = np.ctypeslib.as_array(f.max_zag, (n,)).copy()
    O.lib().orc_jpeg_frame_free(C.byref(f))
    return rc, co, mz


def feeder(data):
    buf = np.frombuffer(data, np.uint8)
    L = _capi.lib()
    f = _capi.JpegFrame()
    rc = L.gamut_hip_jpeg_decode_coeffs(buf.ctypes.data, buf.size, C.byref(f))
    if rc != _capi.OK:
        assert not f.coeffs and not f.max_zag
        return rc, None, None
    n = f.mcus_per_row * f.mcus_per_col * f.blocks_per_mcu
    co = np.ctypeslib.as_array(f.coeffs, (n, 64)).copy(); mz = np.ctypeslib.as_array(f.max_zag, (n,)).copy()
    L.gamut_hip_jpeg_frame_free(C.byref(f))
    return rc, co, mz


def test_geometry_is_read_from_the_kernels():
    """geometry() asserts that it found every number in jpeg_entropy_kernels.hpp; here: that the numbers hang together the way the cases assume"""
    assert set(G) == {"fast_bits", "sub_entries", "sync_min_bytes", "sync_threads", "lane_min_bytes", "lds_huff", "unstuff_tile"}
    assert 8 <= G["fast_bits"] < 16 and G["sub_entries"] >= 1 << (16 - G["fast_bits"])          # one deepest second level fits, a comb's
    assert G["lane_min_bytes"] * G["sync_threads"] >= G["sync_min_bytes"] >= 2 * G["lane_min_bytes"] and G["lane_min_bytes"] % 64 == 0
    assert G["unstuff_tile"] % 16 == 0 and G["lds_huff"] >= 4


def test_the_corpus_keeps_its_proportions():
    kinds = collections.Counter(c.verdict for c in CASES)
    assert set(kinds) <= {"image", "null", "undefined"}
    assert kinds["undefined"] * 10 <= len(CASES) and kinds["image"] * 4 >= 3 * len(CASES), kinds
    fam = collections.Counter(c.family for c in CASES)
    assert set(fam) == {"tables", "grammar", "bytes", "phase", "restart", "sampling"} and len(CASES) >= 60, fam
    assert [(n, d, v) for n, d, v in S.cases()] == [(c.name, c.data, c.verdict) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_readings_agree(case, decoded):
    rc, co, mz = oracle(case.data)
    frc, fco, fmz = feeder(case.data)
    assert rc == {"image": 0, "null": -1, "undefined": -2}[case.verdict], (case.name, rc)
    assert (frc == _capi.OK) == (case.verdict == "image"), (case.name, frc, _capi.last_error())
    if case.verdict == "image":
        assert np.array_equal(fco, co) and np.array_equal(fmz, mz), case.name
    if not case.wellformed:
        return
    ref = decoded[case.name]
    assert np.array_equal(ref.coeffs, case.expect), (case.name, "the plain decoder does not read back what the writer put in")
    if case.verdict == "image":
        assert np.array_equal(co, case.expect), (case.name, np.argwhere(co != case.expect)[:4])
        # max_zag of a well-formed block: one behind the position of the last symbol that is not the EOB (the coefficient's own, or a ZRL's
        # sixteenth zero), 64 for a block that ends without EOB; 1 for a block of nothing but DC
        assert mz.min() >= 1 and mz.max() <= 64
        last = np.zeros(len(co), int)
        nat = np.array(R.ZIGZAG)
        for z in range(63, 0, -1):
            hit = (case.expect[:, nat[z]] != 0) & (last == 0)
            last[hit] = z + 1
        assert (mz >= np.maximum(last, 1)).all(), case.name


@pytest.mark.parametrize("case", [c for c in CASES if c.wellformed], ids=[c.name for c in CASES if c.wellformed])
def test_the_census_proves_the_name(case, decoded):
    cen = decoded[case.name].census
    cl = dict(case.claims)
    huff = decoded[case.name].huff
    for key, want in cl.pop("lengths", {}).items():
        assert set(want) <= set(cen.lengths[key]), (key, sorted(cen.lengths[key]))
    if "deepest_level" in cl:
        key = cl.pop("deepest_level")
        assert R.sub_need(huff[key].bits[1:]) == 1 << (16 - G["fast_bits"]) and 16 in cen.lengths[key] and 10 in cen.lengths[key]
    for key, n in cl.pop("sub_need_is", {}).items():
        assert R.sub_need(huff[key].bits[1:]) == n
    for key, n in cl.pop("sub_need_over", {}).items():
        assert R.sub_need(huff[key].bits[1:]) > n == G["sub_entries"]
    if cl.get("prefixes_fit_and_left") is not None:
        key = cl["prefixes_fit_and_left"]
        fit, left = R.sub_fit(huff[key].bits[1:], G["sub_entries"])
        used = set(cen.prefixes[key])
        assert left and used & set(left) and len(used & set(fit)) >= 6, (sorted(used), fit, left)
    cl.pop("prefixes_fit_and_left", None)
    for key in cl.pop("complete", []):
        assert sum(n << (16 - ln) for ln, n in enumerate(huff[key].bits[1:], 1)) == 65536
    if cl.pop("all_ones_used", False):
        h = huff[(1, 0)]
        assert cen.lengths[(1, 0)][16] and cen.prefixes[(1, 0)][(1 << G["fast_bits"]) - 1] and h.codes()[-1][:2] == (0xFFFF, 16)
        assert cen.symbols[("ac", h.codes()[-1][2] & 15)] > 0
    if "tables_used" in cl:
        assert cen.tables_used == set(cl.pop("tables_used"))
    if "dht_segment_of" in cl:
        assert cl.pop("dht_segment_of") in cen.dht_segments
    for key in cl.pop("defined_twice", []):
        assert cen.tables_defined[key] == 2
    for tq, p in cl.pop("dqt_precision", {}).items():
        assert cen.dqt_precision[tq] == p
    if cl.pop("zero_products", False):
        assert cen.zero_products > 0
    if cl.pop("dc_wraps", False):
        assert cen.dc_wraps >= 3, cen.dc_wraps
    for sym, n in cl.pop("symbols", {}).items():
        assert cen.symbols[sym] >= n, (sym, cen.symbols[sym])
    if "segment_is" in cl:
        assert cen.segments == cl.pop("segment_is"), cen.segments
    if "segment_is_first" in cl:
        want = cl.pop("segment_is_first")
        assert cen.segments[:len(want)] == want and min(cen.segments) < 200 and sorted(cen.segments)[-2] >= G["sync_min_bytes"], cen.segments
    if "segment_at_least" in cl:
        assert max(cen.segments) >= cl.pop("segment_at_least"), cen.segments
    if "stuffed_is" in cl:
        assert cen.stuffed == cl.pop("stuffed_is") == sum(cen.segments)
    if "stuffed_at" in cl:
        tile = G["unstuff_tile"]
        want = cl.pop("stuffed_at")
        assert set(want) <= set(cen.stuffed_at) and all(w % tile == tile - 1 for w in want)          # FF the last byte of a tile, 00 the first of the next
        assert len(case.data) - case.data.index(b"\xff\xda") - 10 > cl.pop("raw_at_least")
    if "marker_at" in cl:
        assert cen.marker_at[:1] == cl.pop("marker_at") and cen.marker_at[0] % G["unstuff_tile"] == G["unstuff_tile"] - 1
    if "intervals" in cl:
        n = cl.pop("intervals")
        assert len(cen.segments) == n and cen.rst == [k & 7 for k in range(n - 1)]
    if "fill" in cl:
        assert cen.fill == cl.pop("fill")
    if "lanes" in cl or "lanes_grow" in cl or "phase_lock" in cl:
        assert len(cen.segments) == 1 and cen.segments[0] >= G["sync_min_bytes"], ("not a segment the many-lane kernel is given", cen.segments)
    if "lanes" in cl:
        assert S.lane_bytes(cen.segments[0], G) == tuple(cl.pop("lanes"))
    if cl.pop("lanes_grow", False):                             # what the name promises: more than the minimum per lane, not every lane at work
        sub, lanes = S.lane_bytes(cen.segments[0], G)
        assert sub > G["lane_min_bytes"] and lanes < G["sync_threads"], (sub, lanes)
    if "scan_type" in cl:
        assert oracle(case.data)[0] == 0 and O.DecodedJpeg(case.data).scan_type == cl.pop("scan_type")
    if "scans" in cl:
        assert len(cen.scans) == cl.pop("scans")
    if "max_zag" in cl:
        blk, want = cl.pop("max_zag")
        assert oracle(case.data)[2][blk] == want
    if "phase_lock" in cl:
        kind = cl.pop("phase_lock")
        sub, lanes = S.lane_bytes(cen.segments[0], G)
        lock = R.phase_lock(cen.trace[0], sub)
        assert len(lock) == lanes - 1
        if kind == "all":                                       # no lane but the first ever stands in the true state
            assert not any(lock.values())
        else:                                                   # the block of the MCU: a lane in three starts right, the others never get there
            assert all(lock[t] == (t % 3 == 0) for t in lock if t < lanes - 3), [t for t in lock if lock[t] != (t % 3 == 0)][:8]
    assert not cl, ("claims nobody checked", cl)


@pytest.mark.parametrize("case", [c for c in CASES if not c.wellformed], ids=[c.name for c in CASES if not c.wellformed])
def test_the_claims_of_the_cases_the_plain_decoder_does_not_read(case):
    """what such a case claims is checked on the file itself: the Kraft sum of the tables its DHT segments hold, the raw length of its scan"""
    cl = dict(case.claims)
    huff, raw = R.header(case.data)
    for key in cl.pop("complete", []):
        assert sum(n << (16 - ln) for ln, n in enumerate(huff[key].bits[1:], 1)) == 65536 and huff[key].codes()[-1][0] == (1 << huff[key].codes()[-1][1]) - 1
    if "scan_below" in cl:
        assert raw < cl.pop("scan_below")
    if "scan_at_least" in cl:
        assert raw - case.data.count(b"\xff\x00") - 2 >= cl.pop("scan_at_least")
    assert not cl, ("claims nobody checked", cl)


def test_the_census_of_the_cases_that_rest_on_a_habit():
    """what can be said of the streams the plain decoder refuses: it does refuse them, and for the reason the name gives"""
    why = {}
    for c in CASES:
        if c.wellformed:
            continue
        try:
            R.decode(c.data)
            why[c.name] = None
        except R.Undefined as e:
            why[c.name] = str(e)
        except (IndexError, AssertionError):
            why[c.name] = "truncated"
    for name, w in why.items():
        if name.startswith("unassigned_window"):
            assert w == "no code word", (name, w)
        elif name.startswith("symbol_"):
            assert w == "r/0", (name, w)
        elif name.startswith("run_past"):
            assert w == "run past 63", (name, w)
        elif name.startswith("zrl_past"):
            assert w == "ZRL past the block", (name, w)
        elif name.startswith("dc_symbol"):
            assert w == "DC category above 15", (name, w)
        elif "truncated" in name:
            assert w is not None, (name, w)
        else:
            assert False, ("a case without a reason", name, w)
