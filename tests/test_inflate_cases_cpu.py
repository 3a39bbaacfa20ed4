"""The constructed DEFLATE streams of tests/inflate_cases.py are what they claim to be, without a GPU: zlib and the plain inflate of
tests/inflate_ref.py agree with the builder on every case (accept / reject, bytes, and for a reject the kernel status the case names), the census
of the reference shows that each mechanism of gamut_amd/csrc/inflate.hip the list is aimed at is reached by a named case, and the census of the
encoder-made streams of tests/test_inflate_gpu.py shows what those never reached (the table in DESIGN.md 4.7)."""
import functools

import pytest

import inflate_cases as IC
import inflate_corpus
import inflate_ref as R


_zlib = inflate_corpus.zlib_inflate


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = IC.by_name(name)
    try:
        return R.inflate(c.data) + (None,)
    except R.InflateError as e:
        return None, None, e.reason


def _census(name):
    out, cs, _ = _ref(name)
    assert out is not None, name
    return cs


def test_builder_is_quick_and_deterministic():
    import time
    t0 = time.perf_counter()
    s = IC.Stream().fixed(IC.cat(IC.lits(b"abc"), IC.matches([3] * 80000, 3)), final=1)            # 120 KB of stream
    data = s.case("x", "").data
    # (token runs are numpy bit arrays: a tenth of a second on an idle machine; a bit at a time in Python it is most of a minute.  The bound leaves a loaded
    # machine room and still tells the two apart.)
    assert len(data) > 100 * 1024 and time.perf_counter() - t0 < 10.0
    assert _zlib(data) == b"abc" * 80001
    again = IC.code_length_cases()
    assert [c.data for c in again] == [IC.by_name(c.name).data for c in again]


@pytest.mark.parametrize("name", [c.name for c in IC.cases()])
def test_zlib_and_the_reference_agree_with_the_builder(name):
    c = IC.by_name(name)
    z = _zlib(c.data)
    out, _, reason = _ref(name)
    if c.status is None:
        assert z is not None and z == c.expect, "zlib does not give the builder's bytes"
        assert out == c.expect, f"the reference: {reason or 'other bytes'}"
    else:
        assert z is None, "zlib accepts a stream the case calls corrupt"
        assert out is None, "the reference accepts a stream the case calls corrupt"
        assert c.status == IC.ANY or IC.STATUS_OF_REASON[reason] == c.status, f"the reference turns it away for: {reason}"
    assert c.note


def test_sizes_stay_small():
    big = [c for c in IC.cases() if len(c.data) > 1024]
    for c in IC.cases():
        assert len(c.data) <= 200 * 1024 and (c.expect is None or len(c.expect) <= 1 << 20), c.name
    assert len(big) < len(IC.cases()) // 2, "most cases are under 1 KiB"


def test_memo_walk_equals_the_naive_walk():
    for name in ("long codes", "random header 7", "2 000 matches of length 32", "block-size whiplash"):
        c = IC.by_name(name)
        out, cs = R.inflate(c.data, memo=True)
        naive = _census(name)
        assert out == c.expect
        assert inflate_corpus.census_row(cs) == inflate_corpus.census_row(naive)


# ---- the census: every mechanism is reached by a named case ----------------------------------------------------------------------------------
def test_long_codes_reach_the_canonical_search():
    """LongLit serves literal / length codes of 12-15 bits, LongDist distance codes of 11-15 bits (kLitBits = 11, kDistBits = 10)"""
    for name in ("long codes", "long codes, three rounds, then a full stored block"):
        cs = _census(name)
        assert cs.max_lit_len == 15 and cs.max_dist_len == 15, name
    cs = _census("long codes")
    assert cs.dist_syms == set(range(30))
    assert {257, 258, 284, 285} <= cs.len_syms and cs.spelled_258_as_284 >= 30
    assert {286} <= cs.hlit and {30, 28} <= cs.hdist
    lit = IC.ALL_LIT
    assert sorted(l for l in lit if l) == list(range(1, 16)) + [15] and lit[256] == 15
    assert {s < 256 for s, l in enumerate(lit) if l >= 12} == {True, False}, "codes of 12 bits and more on literals and on length symbols"
    for dist in (IC.ALL_DIST_A, IC.ALL_DIST_B):
        assert set(range(1, 14)) <= set(dist)
    assert sorted(l for l in IC.ALL_DIST_A if l) == list(range(1, 16)) + [15]
    assert len(IC.by_name("long codes, three rounds, then a full stored block").data) > 2 * IC.ROUND_BYTES + 65535


def test_code_length_streams_cross_a_round():
    long_ones = [c for c in IC.cases() if c.name.startswith("code lengths:")]
    assert len(long_ones) == 7
    for c in long_ones:
        cs = _census(c.name)
        assert cs.max_cl_bits > IC.CL_ROUND_BITS and cs.max_cl_bits == c.meta["cl_bits"], c.name
        assert 19 in cs.hclen
    assert IC.by_name("code lengths: round 2 begins with a repeat-16").meta["round2_first_symbol"] == 16
    c = IC.by_name("code lengths: a 17 ends round 1, a repeat-16 begins round 2")
    assert c.meta["round2_first_symbol"] == 16 and c.meta["round2_begin"] - IC.CL_ROUND_BITS < 10          # the 17 (10 bits) straddles the boundary
    for label, want in (("on", 0), ("one bit before", 31), ("one bit after", 1)):
        m = IC.by_name(f"code lengths: the last length ends {label} a lane boundary of round 2").meta
        assert (m["cl_bits"] - m["round2_begin"]) % 32 == want
    assert 4 in _block_field("hclen 4", "hclen")
    assert len([c for c in IC.cases() if c.name.startswith("random header")]) == 64


def _block_field(name, field):
    """a header field of a stream the reference turns away: from the blocks it saw up to there"""
    c = IC.by_name(name)
    r = R._Reader(c.data, False)
    r.take(3)
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    return {dict(hlit=hlit, hdist=hdist, hclen=hclen)[field]}


def test_header_limits_are_in_the_bytes():
    for v in (287, 288):
        assert _block_field(f"hlit {v}", "hlit") == {v}
    for v in (31, 32):
        assert _block_field(f"hdist {v}", "hdist") == {v}
    assert _census("hdist 1 with length 0, literals only").dist_code_sizes == {0}
    assert _census("one 1-bit distance code, bit 0").dist_code_sizes == {1}
    assert 257 in _census("hlit 257").hlit


def test_speculation_cases_cover_every_phase_and_two_rounds():
    families, out_of_step = {}, {}
    token_bits = {"2-bit codes": 2, "4-bit codes": 4, "8-bit codes": 8, "even tokens with matches": 2}
    for c in IC.cases():
        if c.name.startswith("never resynchronises"):
            cs = _census(c.name)
            main = cs.blocks[-1]
            family = c.meta["family"]
            families.setdefault(family, set()).add(main["begin_bit"] % 8)
            assert main["bits"] > 2 * 8 * IC.ROUND_BYTES, c.name
            # no Huffman block in front: the kernel's `awake` estimate wakes all kT lanes in every round, so a chain that is out of step is walked lane by lane
            # through a full round (a short block in front would narrow the rounds to one wave: IC.lanes_awake)
            assert [b["type"] for b in cs.blocks[:-1]] in ([], [0]), c.name
            awake = IC.lanes_awake(cs.blocks)[-1]
            assert len(awake) == 3 and set(awake) == {IC.LANES}, (c.name, awake)
            # lanes begin on multiples of 256 bits counted from a dword boundary: the true chain never lands on one where its phase is no multiple of the token length
            out_of_step.setdefault(family, 0)
            out_of_step[family] += main["begin_bit"] % 32 % token_bits[family] != 0
    assert len(families) == 4 and all(v == set(range(8)) for v in families.values()), families
    assert out_of_step == {"2-bit codes": 4, "4-bit codes": 6, "8-bit codes": 7, "even tokens with matches": 4}
    cs = _census("long codes, three rounds, then a full stored block")
    assert [b["type"] for b in cs.blocks] == [0, 2, 0, 1] and IC.lanes_awake(cs.blocks)[1] == [IC.LANES] * 3
    cs = _census("block-size whiplash")
    bits = [b["bits"] for b in cs.blocks]
    assert bits[0] < 64 and bits[1] > 3 * 8 * IC.ROUND_BYTES and bits[2] < 8 and bits[3] > 2 * 8 * IC.ROUND_BYTES
    awake = IC.lanes_awake(cs.blocks)
    assert awake[0] == [IC.LANES] and set(awake[1]) == {IC.WAVE} and awake[2] == [IC.LANES] and set(awake[3]) == {IC.WAVE}, "narrow, wide, narrow"
    for name, lane, first in (("end-of-block in lane 1022", 1022, False), ("end-of-block in lane 1022, the lane's first token", 1022, True),
                              ("end-of-block in lane 1023, the lane's first token", 1023, True), ("end-of-block in lane 5, the lane's first token", 5, True)):
        c = IC.by_name(name)
        cs = _census(name)
        block = cs.blocks[-2]
        assert len(cs.blocks) == 2 and block["at_bit"] == 0, "the stream's first block: all lanes awake, the lanes count from bit 0"
        assert IC.lanes_awake(cs.blocks)[0][0] == IC.LANES
        eob = block["begin_bit"] + block["bits"] - 8                       # (the codes of that block are all 8 bits)
        assert eob // IC.LANE_BITS == lane == c.meta["eob_lane"] and (eob % IC.LANE_BITS == 0) == first, name
    cs = _census("40 000 tokens in one round")
    assert cs.max_round_tokens > IC.TOKEN_CAP and cs.rounds == 1


def test_byte_cases_overflow_the_lists_they_are_aimed_at():
    assert _census("2 000 matches of length 32").max_long_per_tile > IC.LONG_CAP
    assert _census("2 000 matches of length 33").max_long_per_tile > IC.LONG_CAP
    assert _census("2 000 matches of length 31").max_long_per_tile <= 130         # (the 258-byte matches of the history in front)
    for c in IC.cases():
        if "run" in c.meta:
            assert _census(c.name).max_same_dist_run == c.meta["run"], c.name
    assert max(c.meta.get("run", 0) for c in IC.cases()) > 16 * IC.WAVE and min(c.meta["run"] for c in IC.cases() if "run" in c.meta) > IC.WAVE
    assert len(IC.by_name("a same-distance run across rounds").data) > IC.ROUND_BYTES
    assert len(IC.by_name("a same-distance run across tiles").expect) > 9 * IC.TILE_BYTES
    assert len(IC.by_name("9 000 matches of length 3 at distance 3").expect) <= IC.TILE_BYTES
    assert _census("9 000 matches, each copying the one before").max_same_dist_run < 40


def test_stored_blocks_follow_every_phase():
    cs = _census("stored blocks behind Huffman blocks that end on every bit of a byte")
    ends = {(b["begin_bit"] + b["bits"]) % 8 for b in cs.blocks if b["type"] == 2}
    assert ends == set(range(8))


# ---- the census of the streams the suite had before ---------------------------------------------------------------------------------------
def test_census_of_the_encoder_made_corpus():
    """every _corpus() entry under all eleven settings of test_inflate_matches_zlib_on_every_encoder_setting, in full: what zlib's encoder never
    wrote (the figures of DESIGN.md 4.7, "before") -- against the constructed cases, which reach each of them"""
    cs, holder = inflate_corpus.census_of(inflate_corpus.corpus_streams())
    row = inflate_corpus.census_row(cs)
    print(row, holder)
    assert cs.max_dist_len <= 10, "LongDist (distance codes of 11 bits and more) was never run"
    assert cs.max_lit_len <= 14
    assert cs.spelled_258_as_284 == 0
    assert cs.max_cl_bits <= IC.CL_ROUND_BITS
    assert max(cs.hclen) < 19 and min(cs.hdist) > 1 and min(cs.dist_code_sizes) > 1, "hclen 19, hdist 1 and a block with fewer than two distance codes were never seen"
    assert cs.max_round_tokens <= IC.TOKEN_CAP and cs.max_long_per_tile <= IC.LONG_CAP, "neither list overflowed"
    mine = R.Census()
    for c in IC.cases():
        if c.status is None:
            mine.merge(_census(c.name))
    assert mine.max_dist_len == 15 and mine.max_lit_len == 15 and mine.spelled_258_as_284 and mine.max_cl_bits > IC.CL_ROUND_BITS
    assert mine.dist_syms == set(range(30)) and 0 in mine.dist_code_sizes and 1 in mine.dist_code_sizes and 19 in mine.hclen
    print(inflate_corpus.census_row(mine))
