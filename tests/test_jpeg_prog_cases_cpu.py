"""The hand-built progressive scans of tests/jpeg_prog_cases.py on the CPU: four readings of every well-formed file -- what the writer's symbol
model says the symbols mean, the plain Annex G decoder of tests/jpeg_prog_ref.py, the oracle (O.DecodedJpeg) and the product's host feeder
(gamut_hip_jpeg_decode_coeffs) agree on coefficients and max_zag -- and the census that proves each case stands on what its name says.  For the
other files the verdict is the oracle's, the host feeder agrees with it, and where the oracle returns an image the plain decoder, told to follow
the reference's habits, reads the same coefficients.  -m gpu: tests/test_jpeg_prog_cases_gpu.py runs the same files through k_prog_scan.

Cases whose verdict the oracle alone decided (the names say what it does): the surplus octets in front of an RSTn (restart_leftover_bad states
the rule), the cut last scan, the EOB runs that reach past their interval."""
import collections

import numpy as np
import pytest

import jpeg_prog_cases as S
import jpeg_prog_ref as R
import oracle_lib as O
from gamut_amd import _capi
from test_jpeg_scan_cases_cpu import feeder, oracle

CASES = S.corpus()
IDS = [c.name for c in CASES]
G = S.geometry()
RC = {"image": 0, "null": -1, "undefined": -2}


@pytest.fixture(scope="module")
def decoded():
    """the plain decoder's reading, made once: T.81 alone for the well-formed cases, with the reference's habits for the others (None: refused)"""
    out = {}
    for c in CASES:
        try:
            out[c.name] = R.decode(c.data, habits=not c.wellformed)
        except (R.Undefined, IndexError):
            out[c.name] = None
    return out


def test_geometry_is_read_from_the_kernel():
    assert set(G) == {"batch", "dc_chunk", "slots", "t6_bits", "wavehuff_bits", "window_dwords", "padding", "deps"}
    assert G["batch"] & (G["batch"] - 1) == 0 and G["batch"] > 2 * G["slots"] and G["dc_chunk"] % 64 == 0          # `u & (kProgBatch - 1)`; a lane per bit
    assert G["t6_bits"] < G["wavehuff_bits"] < 9 and G["window_dwords"] == 63 and G["padding"] * 8 >= 33


def test_the_corpus_keeps_its_proportions():
    kinds = collections.Counter(c.verdict for c in CASES)
    assert set(kinds) <= set(RC)
    assert kinds["image"] * 4 >= 3 * len(CASES), kinds
    fam = collections.Counter(c.family for c in CASES)
    assert set(fam) == set(S.FAMILIES) and len(CASES) >= 100, fam
    for f in S.FAMILIES:
        assert any(c.family == f and c.wellformed and c.verdict == "image" for c in CASES), f
    assert max(len(c.data) for c in CASES) <= 64 << 10 and sum(len(c.data) for c in CASES) <= 1 << 20
    blocks = {c.name: R.header_blocks(c.data) for c in CASES}
    assert sorted(blocks.values())[-3:-2][0] <= 6 * G["batch"] and len([n for n in blocks.values() if n > G["dc_chunk"]]) == 2, "two large cases"
    assert [(n, d, v) for n, d, v in S.cases()] == [(c.name, c.data, c.verdict) for c in CASES]
    assert len(set(c.data for c in CASES)) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_readings_agree(case, decoded):
    rc, co, mz = oracle(case.data)
    frc, fco, fmz = feeder(case.data)
    assert rc == RC[case.verdict], (case.name, rc)
    assert (frc == _capi.OK) == (case.verdict == "image"), (case.name, frc, _capi.last_error())
    ref = decoded[case.name]
    if case.verdict == "image":
        assert np.array_equal(fco, co) and np.array_equal(fmz, mz), (case.name, np.argwhere(fco != co)[:4].tolist())
        assert ref is not None, (case.name, "the plain decoder does not read the file")
        assert np.array_equal(ref.coeffs, co), (case.name, np.argwhere(ref.coeffs != co)[:4].tolist())
        assert np.array_equal(ref.max_zag, mz), (case.name, np.flatnonzero(ref.max_zag != mz)[:8].tolist())
    if case.wellformed:
        assert ref is not None and np.array_equal(ref.coeffs, case.expect), (case.name, "the plain decoder does not read back what the writer put in")
        assert np.array_equal(ref.max_zag, case.max_zag), case.name
    elif case.verdict == "image":
        # a habit of the reference: T.81 alone defines no result
        with pytest.raises((R.Undefined, IndexError)):
            R.decode(case.data)
    else:
        assert ref is None, (case.name, "refused by the reference, read by the plain decoder")


def _kind(cen, k):
    return [s for s in cen if s.kind == k]


@pytest.mark.parametrize("case", [c for c in CASES if c.claims], ids=[c.name for c in CASES if c.claims])
def test_the_census_proves_the_name(case, decoded):
    d = decoded[case.name]
    assert d is not None
    sc = d.scans
    cl = dict(case.claims)
    first, refine = _kind(sc, R.AC_FIRST), _kind(sc, R.AC_REFINE)
    acs = first + refine
    B = G["batch"]
    if "max_eobrun" in cl:
        assert max(s.max_eobrun for s in acs) == cl.pop("max_eobrun") == 0x7FFF
    if "eob_sizes" in cl:
        assert {n for s in acs for (_, n, _, _) in s.eob_starts} >= set(cl.pop("eob_sizes"))
    for n in cl.pop("extra_all_ones", []):
        assert any(e == n and x == (1 << n) - 1 for s in acs for (_, e, x, _) in s.eob_starts), n
    for n in cl.pop("extra_all_zero", []):
        assert any(e == n and x == 0 for s in acs for (_, e, x, _) in s.eob_starts), n
    if "file_below" in cl:
        assert len(case.data) < cl.pop("file_below")
    if "run_starts" in cl:
        want = cl.pop("run_starts")
        res = cl.pop("run_start_residues")
        for s in acs:                                           # the first scan and its refinement: the same runs
            got = {u: run for (u, _, _, run) in s.eob_starts if run > 1 or not s.history.get(u)}
            assert set(want) <= set(got), sorted(set(want) - set(got))
            for length in range(1, 6):
                assert {u % res for u, run in got.items() if run == length} == set(range(res)), length
            assert {B - 2, B - 1, 0} <= {u % B for u, run in got.items() if run > 1}           # units 62, 63 and 64 of a batch
        assert first and refine and len(refine[0].free_skips) >= 40
    if cl.pop("ends_on_last_block", False):
        assert all(max(u + run for (u, _, _, run) in s.eob_starts) == s.units for s in acs)
    if cl.pop("band_of_one", False):
        assert all(s.ss == s.se for s in acs)
    if "hand_offs" in cl:
        assert all((s.units - 1) // B == cl["hand_offs"] for s in acs); cl.pop("hand_offs")
    if "code_lengths" in cl:
        assert set(cl.pop("code_lengths")) <= set().union(*[set(s.lengths) for s in acs])
    if "run_ends_at_interval_end" in cl:
        ri = cl.pop("run_ends_at_interval_end")
        assert any(s.ri == ri and any(u + run == ri for (u, _, _, run) in s.eob_starts) for s in acs)
    if "habit" in cl:
        want = cl.pop("habit")
        assert any(h[0] == want for s in sc for h in s.habits), [h for s in sc for h in s.habits][:4]
    if "lands_on_se" in cl:
        n = cl.pop("lands_on_se")
        assert max(int((d.quantised[:, s.se] != 0).sum()) for s in acs if s.se < 63 or len(acs) == 1) >= n      # blocks with a coefficient ON Se
    for sym, n in cl.pop("symbols", {}).items():
        assert sum(s.symbols[sym] for s in sc) >= n, (sym, [s.symbols[sym] for s in sc])
    if "left_int16" in cl:
        n = cl.pop("left_int16")
        got = sum(s.left_int16 for s in sc)
        assert got >= n and (n > 0 or got == 0), got
    if "al" in cl:
        al = cl.pop("al")
        assert any(s.al == al for s in sc)
    if "bands" in cl:
        assert [(s.ss, s.se) for s in first] == cl.pop("bands")
    for kind, n in cl.pop("scans_of_kind", {}).items():
        assert len(_kind(sc, kind)) == n
    if "new_per_block" in cl:
        n = cl.pop("new_per_block")
        assert all(sum(s.symbols[("new", r)] for r in range(16)) == n * s.units for s in refine)
    if cl.pop("no_first_scan", False):
        assert not first and all(not h for s in refine for h in s.history.values())
    if "history_is" in cl:
        n = cl.pop("history_is")
        assert all(len(h) == n for s in refine for h in s.history.values())
    if "corr_after_eob" in cl:
        n = cl.pop("corr_after_eob")
        assert all(c == n for s in refine for (_, sym, c) in s.corr_bits) and any(sym is None for s in refine for (_, sym, _) in s.corr_bits)
    if cl.pop("both_signs", False):
        assert (d.quantised[:, 1:] > 0).any() and (d.quantised[:, 1:] < 0).any()
    if "corr_behind_symbol" in cl:
        sym, n = cl.pop("corr_behind_symbol")
        assert any(s_ == sym and c >= n for s in refine for (_, s_, c) in s.corr_bits)
    if "starved" in cl:
        assert sum(len(s.starved) for s in refine) == cl.pop("starved")
    if "past_band" in cl:
        z = cl.pop("past_band")
        assert any(k == z == s.se + 1 for s in refine for (_, k) in s.past_band)
        assert any(o.kind == R.AC_FIRST and o.ss <= z <= o.se for o in sc)                  # ... which another scan owns
    if cl.pop("habit_plane_set", False):
        assert sum(s.plane_set for s in refine) >= 8
    if "free_skips_and_corr_only" in cl:
        units = cl.pop("free_skips_and_corr_only")
        s = refine[0]
        assert set(units) <= s.eob_units and set(units) & s.free_skips and set(units) & s.corr_only
        assert len(s.free_skips) >= 40 and len(s.corr_only) >= 40
        flip = [u for u in range(1, s.units) if u in s.eob_units and (u in s.free_skips) != (u - 1 in s.free_skips)]
        assert len(flip) >= 100                                                           # alternating
    if "intervals" in cl:
        n = cl.pop("intervals")
        assert len(refine[0].segments) == n
    if "code_in_front_of_extra" in cl:
        ln, n = cl.pop("code_in_front_of_extra")
        assert any(l_ == ln and sym == n << 4 for s in acs for (_, _, l_, sym) in s.code_at)
    if cl.pop("stuffed_with_bits", False):
        s = refine[0]
        ff = set(s.stuffed[0])
        assert len(ff) >= 20 and sum(1 for (_, p) in s.sign_at if p >> 3 in ff) >= 20 and sum(1 for (_, p) in s.corr_at if p >> 3 in ff) >= 20
    if cl.pop("straddles_reload", False):
        s = refine[0]
        edge = G["window_dwords"] * 32                                                     # the first position whose dword is not in the window
        inside = [u for u, (_, a, b) in s.block_span.items() if a < edge < b]
        assert inside and s.seg_bits[0] > 2 * edge - 32
        u = inside[0]
        assert any(a <= p < edge for (_, p) in s.sign_at for a in [s.block_span[u][1]]) and any(edge <= p < s.block_span[u][2] for (_, p) in s.corr_at)
    if cl.pop("sign_is_last_bit", False):
        s = refine[0]
        assert s.seg_bits[-1] == 8 * s.segments[-1] and s.sign_at[-1] == (len(s.segments) - 1, s.seg_bits[-1] - 1)
    if "past_end" in cl:
        n = cl.pop("past_end")
        got = sum(s.past_end for s in sc)
        assert got == n if n is not True else got > 0, got
    if cl.pop("negative_history", False):
        assert any(v < 0 for v in d.quantised[:, 1:].ravel())
    if "scan_type" in cl:
        assert O.DecodedJpeg(case.data).scan_type == cl.pop("scan_type")
    if "blocks_per_unit" in cl:
        n = cl.pop("blocks_per_unit")
        s = _kind(sc, R.DC_REFINE)[0]
        assert len(s.comps) == 3 and len(s.corr_at) == n * s.units and d.frame["nb"] == n
    if cl.pop("outside_stay_zero", False):
        fr = d.frame
        coded = sum(s.units for s in _kind(sc, R.DC_FIRST))
        assert coded < fr["mpr"] * fr["mpc"] * fr["nb"] and all(len(s.comps) == 1 for s in sc)
        assert (d.quantised[:, 0] == 0).sum() >= fr["mpr"] * fr["mpc"] * fr["nb"] - coded
    if "units_over" in cl:
        assert _kind(sc, R.DC_REFINE)[0].units > cl.pop("units_over")
    if cl.pop("negative_values", False):
        assert (d.quantised[:, 0] < 0).sum() > 100
    if "lined_up" in cl:
        assert cl.pop("lined_up") is False
        a, b = first[0], refine[0]
        assert a.comps == b.comps and a.ri != b.ri
    if "dri_values" in cl:
        assert d.dri_values == cl.pop("dri_values")
    if "kinds_with_intervals" in cl:
        assert len({s.kind for s in sc if len(s.segments) > 1}) == cl.pop("kinds_with_intervals")
    if "fill" in cl:
        i, want = cl.pop("fill")
        assert sc[i].fill[:len(want)] == want
    if "surplus" in cl:
        i = cl.pop("surplus")
        assert sc[i].surplus[0] >= 1 and sc[i].surplus[1] >= 1
    if "scans" in cl:
        assert len(sc) == cl.pop("scans")
    if "unmentioned" in cl:
        c = cl.pop("unmentioned")
        assert all(c not in s.comps for s in sc) and len(d.frame["comp"]) > c
    if "deps_over" in cl:
        n = cl.pop("deps_over")
        r = refine[0]
        assert len([s for s in first if s.comps == r.comps and s.ss <= r.se and r.ss <= s.se]) > n
    if cl.pop("dht_between", False):
        assert d.dht_between >= 2 and d.dqt_between >= 1
    assert not cl, ("claims nobody checked", cl)
