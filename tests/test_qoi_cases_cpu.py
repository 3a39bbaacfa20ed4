"""The case list of tests/qoi_cases.py, checked without a GPU: an op walker that lays every stream out as the decode kernels see it (windows of
param(0) chunk bytes, groups of 64 ops per window, lanes of param(1) bytes) finds each property a case is named for in its bytes, and a second
decoder, written from the reference's text, agrees with the oracle on streams no encoder writes.  The second half checks the launch layouts
of tests/qoi_batch.py that tests/test_qoi_batch_gpu.py runs the cases in: where the streams and their pixels lie, and which kernel a launch gets."""
import collections
import ctypes as C
import functools
import gc
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import qoi_batch as B
import qoi_cases as Q
from gamut_amd import _capi

Op = collections.namedtuple("Op", "n off len kind win idx group lane first_px npx run px slot src executed")
Group = collections.namedtuple("Group", "win group ops before waiting total straight")


def op_length(b1):
    return 4 if b1 == 0xFE else 5 if b1 == 0xFF else 2 if b1 >> 6 == 2 else 1


def op_kind(b1):
    return "rgb" if b1 == 0xFE else "rgba" if b1 == 0xFF else ("index", "diff", "luma", "run")[b1 >> 6]


def walk(data):
    """every op that starts below the end of the chunk bytes, with where it lies (window, op number in the window, group, lane), the pixels it makes
    (clamped to the image), the table slot it writes and, for an INDEX op, the op that last wrote the slot it reads (None: nobody)"""
    w, h, _ = Q.header(data)
    total, chunk = w * h, max(len(data) - 8 - Q.HEADER, 0)
    body = data[Q.HEADER:] + bytes(8)
    ops, p, px, table, writer, produced = [], 0, (0, 0, 0, 255), [(0, 0, 0, 0)] * 64, [None] * 64, 0
    in_window = collections.Counter()
    while p < chunk:
        b1, src, run = body[p], None, 1
        kind, length = op_kind(b1), op_length(b1)
        if kind == "rgb":
            px = (body[p + 1], body[p + 2], body[p + 3], px[3])
        elif kind == "rgba":
            px = tuple(body[p + 1:p + 5])
        elif kind == "index":
            src, px = writer[b1], table[b1]
        elif kind == "diff":
            px = ((px[0] + (b1 >> 4 & 3) - 2) & 255, (px[1] + (b1 >> 2 & 3) - 2) & 255, (px[2] + (b1 & 3) - 2) & 255, px[3])
        elif kind == "luma":
            vg = (b1 & 63) - 32
            px = ((px[0] + vg - 8 + (body[p + 1] >> 4)) & 255, (px[1] + vg) & 255, (px[2] + vg - 8 + (body[p + 1] & 15)) & 255, px[3])
        else:
            run = 1 + (b1 & 63)
        win = p // Q.WIN
        idx = in_window[win]; in_window[win] += 1
        slot = Q.hash_of(px)
        table[slot], writer[slot] = px, len(ops)
        npx = max(0, min(run, total - produced))
        ops.append(Op(len(ops), p, length, kind, win, idx, idx // Q.GROUP, idx % Q.GROUP, produced, npx, run, px, slot, src, produced < total))
        produced += npx
        p += length
    return ops, total, chunk


def groups(ops):
    """the groups the one-wave kernel works through, with the pixels that wait in its buffer in front of each (three-channel output): a group of more
    than BUF_GROUP pixels is stored straight to the image behind what waited, the others join the buffer, which lets whole rows of 256 go"""
    out, waiting, before = [], 0, 0
    keys = sorted({(o.win, o.group) for o in ops if o.executed})
    for key in keys:
        mine = [o for o in ops if (o.win, o.group) == key]
        total = sum(o.npx for o in mine)
        straight = total > Q.BUF_GROUP
        out.append(Group(key[0], key[1], mine, before, waiting, total, straight))
        waiting = 0 if straight else (waiting + total) % 256
        before += total
    return out


WALKS = {c.name: walk(c.data) for c in Q.CONSTRUCTED}


def test_the_geometry_is_the_kernels():
    assert (Q.WIN, Q.LANE, Q.BUF_GROUP, Q.WIDE_BELOW, Q.HOST_GROUP) == tuple(Q.param(k) for k in range(5)) and Q.param(5) == -1 and Q.param(-1) == -1
    assert Q.WIN % Q.LANE == 0 and Q.WIN // Q.LANE == 64 and Q.LANE >= 5 and Q.BUF_GROUP >= 256
    # The host-memory entry cuts a batch into launches of param(4) streams, and a launch runs one wave per stream from param(3) streams on: as long
    # as this holds, nothing that comes from host memory reaches the one-wave kernel -- only gamut_hip_qoi_decode_resident_device with at least
    # param(3) streams does.  If it stops holding, the docstrings of test_qoi_gpu.py and tools/fuzz_qoi_gpu.py need another look.
    assert Q.param(4) < Q.param(3)


def test_the_cases_stay_small():
    for c in Q.CONSTRUCTED:
        ops, total, chunk = WALKS[c.name]
        assert total <= 30000 and chunk <= 5 * Q.WIN, c.name
    # repeated to the smallest batch the one-wave kernel takes, all of them (the arbitrary ones included) stay under 10 MB in and 25 MB out
    assert sum(len(c.data) for c in Q.CASES) * (Q.WIDE_BELOW / len(Q.CASES)) < 10e6
    assert sum(Q.expected(c.name, 4).size for c in Q.CASES) * (Q.WIDE_BELOW / len(Q.CASES)) < 25e6


@pytest.mark.parametrize("ch", (3, 4))
@pytest.mark.parametrize("boundary", Q.BOUNDARIES)
def test_every_op_length_straddles_every_boundary_by_every_byte_count(boundary, ch):
    assert len(Q.STRADDLES) == 8 and {l for l, _ in Q.STRADDLES} == {2, 4, 5} and all(0 < s < l for l, s in Q.STRADDLES)
    assert len({(l, s) for l in (2, 4, 5) for s in range(1, l)}) == 8
    for (length, s) in Q.STRADDLES:
        c = Q.BY_NAME[f"straddle-{boundary}-L{length}-s{s}-ch{ch}"]
        ops, total, chunk = WALKS[c.name]
        assert Q.header(c.data)[2] == ch
        at = {"window": lambda o: o.off + s > 0 and (o.off + s) % Q.WIN == 0,
              "lane": lambda o: (o.off + s) % Q.LANE == 0 and (o.off + s) % Q.WIN != 0,
              "end": lambda o: o.off + s == chunk}[boundary]
        hit = [o for o in ops if o.len == length and at(o)]
        also_first = (boundary, ch, length, s) == ("window", 4, 2, 1)                      # (the LUMA op across the first boundary is one of these as well)
        assert len(hit) == (2 if also_first else 1) and hit[-1].executed and hit[-1].npx == 1, c.name
        o = hit[-1]
        assert ops[o.n - 1].kind == "diff" and ops[o.n - 1].px != o.px                 # reached through one-byte ops; its pixel shows
        if boundary == "end":
            assert o.n == len(ops) - 1 and total > o.first_px + 1                          # the tail of the image repeats it
            assert o.px[:3] != (0, 0, 0) or length != 2
        else:
            assert ops[o.n + 1].off % (Q.WIN if boundary == "window" else Q.LANE) == length - s and ops[-1].executed
    if boundary == "window":                                                               # ... the first boundary, and the second behind a first that is straddled too
        first = {WALKS[f"straddle-window-L{l}-s{s}-ch{ch}"][0][-1].win for l, s in Q.STRADDLES}
        assert first == ({1} if ch == 3 else {2})
        if ch == 4:
            assert all(any(o.off == Q.WIN - 1 and o.len == 2 for o in WALKS[f"straddle-window-L{l}-s{s}-ch4"][0]) for l, s in Q.STRADDLES)
    if boundary == "end":                                                                  # the bytes the op reads behind the chunk are the file's padding
        assert all(Q.BY_NAME[f"straddle-end-L{l}-s{s}-ch{ch}"].data[-8:] == (Q.PADDING if ch == 3 else Q.ODD_PADDING) for l, s in Q.STRADDLES)


def test_the_chunk_lengths():
    names = [c.name for c in Q.CONSTRUCTED if c.name.startswith("chunk-")]
    assert [WALKS[n][2] for n in names] == [0, 1, 31, 32, 33, Q.WIN - 1, Q.WIN, Q.WIN + 1, 2 * Q.WIN] == list(Q.CHUNK_LENGTHS)
    assert len(Q.BY_NAME["chunk-0-bytes"].data) == 22 and (Q.expected("chunk-0-bytes", 4).reshape(-1, 4) == (0, 0, 0, 255)).all()
    for n in names:
        ops, total, chunk = WALKS[n]
        assert not ops or (ops[-1].off + ops[-1].len == chunk and ops[-1].executed), n
        assert {Q.header(Q.BY_NAME[n].data)[2] for n in names} == {3, 4}
    kinds = {o.kind for n in names for o in WALKS[n][0]}
    assert kinds == {"rgb", "rgba", "index", "diff", "luma", "run"}


def _buffer_groups():
    return {c.name: groups(WALKS[c.name][0]) for c in Q.CONSTRUCTED if Q.header(c.data)[2] == 3}


def test_the_pixel_buffer_of_three_channel_outputs():
    G = _buffer_groups()
    every = [(n, i, g) for n, gs in G.items() for i, g in enumerate(gs)]
    # a group of 64 ops with RUN-62 ops that goes round the buffer, with 1 and with 255 pixels waiting in it, and right after exactly 256 have
    # left it (more than 255 never wait: whole rows of 256 leave at once); ordinary ops follow
    for before, waiting in ((257, 1), (255, 255), (256, 0)):
        hit = [(n, i) for n, i, g in every if g.straight and len(g.ops) == 64 and (g.before, g.waiting) == (before, waiting) and any(o.run == 62 for o in g.ops)]
        assert hit, (before, waiting)
        n, i = hit[0]
        assert n.startswith("buffer-long-group-behind-") and len(G[n]) > i + 1 and not G[n][i + 1].straight and {o.kind for o in G[n][i + 1].ops} >= {"diff", "luma", "rgb"}
    assert any(g.total == Q.BUF_GROUP and not g.straight and g.waiting == 255 and len(g.ops) == 64 for _, _, g in every)      # the fullest the buffer gets
    assert any(g.total == Q.BUF_GROUP + 1 and g.straight and g.waiting == 255 for _, _, g in every)
    assert any(g.total == 64 * 62 and all(o.kind == "run" and o.npx == 62 for o in g.ops) and len(g.ops) == 64 for _, _, g in every)
    assert {256, 512} <= {g.waiting + g.total for _, _, g in every if not g.straight}
    for n in G:
        if n.startswith("buffer-"):
            assert all(o.executed for o in WALKS[n][0]) and WALKS[n][0][-1].win == 0, n


def test_the_image_fills_in_the_middle_of_a_run():
    def crossing(name):
        ops, total, _ = WALKS[name]
        hit = [o for o in ops if o.kind == "run" and o.first_px < total < o.first_px + o.run and o.npx > 0]
        assert len(hit) == 1 and hit[0].n + 64 < len(ops), name                           # ops follow it that must change nothing
        return hit[0], ops
    o, ops = crossing("full-run-first-lane")
    assert o.lane == 0 and o.group == 1
    o, ops = crossing("full-run-last-lane")
    assert o.lane == 63 and o.group == 1
    # in a group of more than BUF_GROUP pixels: the part of it inside the image is what the one-wave kernel decides by -- more (round the buffer), and fewer
    o, ops = crossing("full-run-long-group")
    assert 0 < o.lane < 63 and sum(x.npx for x in ops if (x.win, x.group) == (o.win, o.group)) > Q.BUF_GROUP
    o, ops = crossing("full-run-long-group-cut-below-the-threshold")
    assert 0 < o.lane < 63 and sum(x.run for x in ops if (x.win, x.group) == (o.win, o.group)) > Q.BUF_GROUP > sum(x.npx for x in ops if (x.win, x.group) == (o.win, o.group))
    assert {Q.header(Q.BY_NAME[n].data)[2] for n in ("full-run-first-lane", "full-run-last-lane", "full-run-long-group")} == {3, 4}
    ops, total, chunk = WALKS["full-then-a-window-of-noise"]
    last = max(o.n for o in ops if o.executed)
    assert ops[last].first_px + ops[last].npx == total and chunk - ops[last].off > Q.WIN and ops[last].win == 0 and ops[-1].win >= 1
    ops, total, chunk = WALKS["ends-one-pixel-short"]
    assert sum(o.npx for o in ops) == total - 1 and ops[-1].executed
    ops, total, chunk = WALKS["ends-after-its-first-op"]
    assert len(ops) == 1 and total > 30 and (Q.expected("ends-after-its-first-op", 3).reshape(-1, 3) == ops[0].px[:3]).all()


def test_where_the_index_ops_find_their_slots():
    idx = [(n, o, WALKS[n][0]) for n in WALKS for o in WALKS[n][0] if o.kind == "index" and o.executed]
    def some(pred, name):
        hit = [(n, o) for n, o, ops in idx if n == name and pred(o, ops)]
        assert hit, name
        return hit
    # nobody wrote the slot: (0, 0, 0, 0), in a four-channel file, so that the alpha shows at outputs 0 and 4 -- as the stream's first op, and later
    hit = some(lambda o, ops: o.src is None, "index-slot-never-written")
    assert all(o.px == (0, 0, 0, 0) for _, o in hit) and {o.n == 0 for _, o in hit} == {True, False} and Q.header(Q.BY_NAME["index-slot-never-written"].data)[2] == 4
    for _, o in hit:
        assert Q.expected("index-slot-never-written", 0).reshape(-1, 4)[o.first_px].tolist() == [0, 0, 0, 0]
        assert Q.expected("index-slot-never-written", 3).reshape(-1, 3)[o.first_px].tolist() == [0, 0, 0]
    same = lambda o, ops: o.src is not None and (ops[o.src].win, ops[o.src].group) == (o.win, o.group)
    some(lambda o, ops: same(o, ops) and ops[o.src].kind == "rgb" and o.px != ops[o.n - 1].px, "index-slot-written-in-the-same-group")
    some(lambda o, ops: o.src is not None and ops[o.src].win == o.win and ops[o.src].group == o.group - 1 and o.px != ops[o.n - 1].px, "index-slot-written-in-the-previous-group")
    some(lambda o, ops: o.src is not None and ops[o.src].win == o.win - 1 and ops[o.src].group == 0 and o.px != ops[o.n - 1].px, "index-slot-written-in-the-previous-window")
    some(lambda o, ops: o.src is not None and ops[o.src].win == o.win - 1 and ops[o.src].kind == "run", "index-slot-written-in-the-previous-window")
    # written twice inside the group, by different pixels: the newest counts; and an older group's pixel counts until the first of them
    def writers(o, ops):                                                                   # (an INDEX op that finds a pixel writes the slot it read)
        return [x for x in ops[:o.n] if (x.win, x.group) == (o.win, o.group) and x.slot == o.slot]
    twice = some(lambda o, ops: same(o, ops) and len({x.px for x in writers(o, ops) if x.kind != "index"}) >= 2 and o.px == ops[o.src].px, "index-slot-written-twice-in-one-group")
    assert len(twice) >= 2
    some(lambda o, ops: not same(o, ops) and any(x.slot == o.slot and x.n > o.n and (x.win, x.group) == (o.win, o.group) and x.px != o.px for x in ops), "index-slot-written-twice-in-one-group")
    # the slot's last writer is a RUN op: of the start pixel, which no other op ever stored, and of an ordinary one
    hit = some(lambda o, ops: o.src is not None and ops[o.src].kind == "run", "index-slot-written-by-a-run")
    assert any(o.px == (0, 0, 0, 255) and ops[o.src].n == 0 for (_, o), ops in ((h, WALKS[h[0]][0]) for h in hit))
    # 64 INDEX ops in one group: on 64 slots, and all on one
    def full_groups(name):
        ops = WALKS[name][0]
        return [[o for o in ops if (o.win, o.group) == key] for key in {(o.win, o.group) for o in ops}]
    assert any(len(g) == 64 and all(o.kind == "index" for o in g) and len({o.slot for o in g}) == 64 and len({o.px for o in g}) == 64 for g in full_groups("index-64-ops-in-one-group"))
    assert any(len(g) == 64 and all(o.kind == "index" for o in g) and len({o.slot for o in g}) == 1 and g[0].px != (0, 0, 0, 0) for g in full_groups("index-64-ops-on-one-slot"))
    # the first op of a window
    some(lambda o, ops: o.win == 1 and o.idx == 0 and o.off == Q.WIN and o.src is not None and o.px != ops[o.n - 1].px, "index-first-op-of-a-window")
    for n in WALKS:
        if n.startswith("index-"):
            assert all(o.executed for o in WALKS[n][0]), n


def test_alpha_set_in_a_three_channel_file():
    name = "alpha-rgba-ops-in-a-three-channel-file"
    ops, total, _ = WALKS[name]
    assert Q.header(Q.BY_NAME[name].data)[2] == 3 and all(o.executed for o in ops) and ops[-1].group >= 1
    alphas = [o.px[3] for o in ops]
    assert len({o.px[3] for o in ops if o.kind == "rgba"}) >= 2 and 255 not in {o.px[3] for o in ops if o.kind == "rgba"}
    for kind in ("diff", "luma", "run", "rgb"):                                            # the alpha an RGBA op set is carried by the ops that leave it alone
        assert any(o.kind == kind and o.px[3] != 255 for o in ops), kind
    idx = [o for o in ops if o.kind == "index"]
    assert any(o.px[3] == 255 and ops[o.n - 1].px[3] != 255 for o in idx) and any(o.px[3] not in (0, 255) and ops[o.n - 1].px[3] == 255 for o in idx)     # INDEX: the named pixel's alpha, both ways
    assert any(o.px[3] != ops[o.n - 1].px[3] and o.group >= 1 for o in idx)
    assert any(a.px[3] != 255 and b.kind in ("diff", "luma") and b.group == a.group + 1 and b.lane == 0 for a, b in zip(ops, ops[1:]))                       # ... across a group boundary
    e0, e3, e4 = (Q.expected(name, ch) for ch in (0, 3, 4))
    assert np.array_equal(e0, e3) and np.array_equal(e4.reshape(-1, 4)[:, :3].reshape(-1), e3)
    assert e4.reshape(-1, 4)[[o.first_px for o in ops], 3].tolist() == alphas


def py_qoi_decode(data, channels):
    """qoi_decode (codecs/qoi.d:448-550) again, in plain Python: independent of the oracle's C and of the walker above"""
    size = len(data)
    w, h, file_ch = int.from_bytes(data[4:8], "big"), int.from_bytes(data[8:12], "big"), data[12]
    if channels not in (0, 3, 4) or size < 14 + 8 or data[:4] != b"qoif" or w == 0 or h == 0 or file_ch not in (3, 4) or data[13] > 1 or h >= 400000000 // w:
        return None
    channels = channels or file_ch
    px_len = w * h * channels
    pixels = bytearray(px_len)
    index = [[0, 0, 0, 0] for _ in range(64)]
    r, g, b, a = 0, 0, 0, 255
    p, run, chunks_len = 14, 0, size - 8
    for px_pos in range(0, px_len, channels):
        if run > 0:
            run -= 1
        elif p < chunks_len:
            b1 = data[p]; p += 1
            if b1 == 0xFE:
                r, g, b = data[p], data[p + 1], data[p + 2]; p += 3
            elif b1 == 0xFF:
                r, g, b, a = data[p], data[p + 1], data[p + 2], data[p + 3]; p += 4
            elif b1 & 0xC0 == 0x00:
                r, g, b, a = index[b1]
            elif b1 & 0xC0 == 0x40:
                r = (r + ((b1 >> 4) & 3) - 2) & 255; g = (g + ((b1 >> 2) & 3) - 2) & 255; b = (b + (b1 & 3) - 2) & 255
            elif b1 & 0xC0 == 0x80:
                b2 = data[p]; p += 1
                vg = (b1 & 0x3F) - 32
                r = (r + vg - 8 + ((b2 >> 4) & 15)) & 255; g = (g + vg) & 255; b = (b + vg - 8 + (b2 & 15)) & 255
            else:
                run = b1 & 0x3F
            index[(r * 3 + g * 5 + b * 7 + a * 11) % 64] = [r, g, b, a]
        pixels[px_pos:px_pos + channels] = (r, g, b, a)[:channels]
    return bytes(pixels)


@pytest.mark.parametrize("ch", (0, 3, 4))
def test_a_second_decoder_agrees_with_the_oracle(ch):
    """the constructed streams push the oracle where no encoder's output does: ops read out of the padding, slots nobody wrote, alpha in three-channel files"""
    for c in Q.CONSTRUCTED:
        assert py_qoi_decode(c.data, ch) == Q.expected(c.name, ch).tobytes(), c.name
    for c in Q.ARBITRARY[:4] + Q.ARBITRARY[24:26]:
        assert py_qoi_decode(c.data, ch) == Q.expected(c.name, ch).tobytes(), c.name
    assert py_qoi_decode(b"qoif" + bytes(30), ch) is None and O.qoi_decode(b"qoif" + bytes(30), ch) is None


def test_the_walker_agrees_with_the_oracle():
    """the pixels the walker gives the ops, laid out by their run lengths, with the last one repeated to the end of the image"""
    for c in Q.CONSTRUCTED:
        ops, total, _ = WALKS[c.name]
        px, last = [], (0, 0, 0, 255)
        for o in ops:
            px += [o.px] * o.npx
            last = o.px if o.executed else last
        px += [last] * (total - len(px))
        assert np.array_equal(np.array(px, np.uint8).reshape(-1), Q.expected(c.name, 4)), c.name


def test_the_case_list():
    assert len(Q.CONSTRUCTED) == 3 * 8 * 2 + 9 + 8 + 7 + 9 + 1 and len(Q.ARBITRARY) == 40 and len({c.data for c in Q.CASES}) == len(Q.CASES)
    assert not Q.expected(Q.CASES[0].name, 4).flags.writeable


# ---- the launch layouts of tests/qoi_batch.py, as tests/test_qoi_batch_gpu.py uses them ------------------------------------------------------------

def _resident_layouts():
    """(label, layout, runs one wave per stream) of every resident launch of test_qoi_batch_gpu.py"""
    out = [(f"{kernel}-{ch}", B.resident(kernel, ch), kernel == "one_wave") for kernel in ("one_wave", "phases") for ch in (0, 3, 4)]
    out += [(f"threshold-{n}-{ch}", B.threshold(n, ch), n >= Q.WIDE_BELOW) for n in (Q.WIDE_BELOW - 1, Q.WIDE_BELOW) for ch in (4, 3)]
    return out


@functools.lru_cache(maxsize=None)
def _layouts():
    return _resident_layouts()


def test_the_layouts_run_the_kernel_they_are_named_for():
    for label, L, one_wave in _layouts():
        assert (L.n >= Q.WIDE_BELOW) == one_wave, label
    assert B.resident("one_wave", 4).n == B.ONE_WAVE_COPIES * len(Q.CASES) == 854 and B.resident("pipeline", 4).n == len(Q.CASES) == 122
    assert [L.n for label, L, _ in _layouts() if label.startswith("threshold")] == [Q.WIDE_BELOW - 1] * 2 + [Q.WIDE_BELOW] * 2
    assert [s for s in B.threshold(Q.WIDE_BELOW - 1, 4).streams] == B.resident("one_wave", 4).streams[:Q.WIDE_BELOW - 1]     # the first streams of the same list
    # from host memory: all cases are one launch, three times all cases are two, and neither reaches the one-wave kernel
    assert B.host(1, 0).n == len(Q.CASES) <= Q.HOST_GROUP < B.host(3, 0).n == 3 * len(Q.CASES) <= 2 * Q.HOST_GROUP and Q.HOST_GROUP < Q.WIDE_BELOW
    assert [c.name.rsplit("-", 3)[0] for c in B.drop_in_cases()[:3]] == ["straddle-window", "straddle-lane", "straddle-end"] and len(B.drop_in_cases()) == 8
    assert all(c in Q.CONSTRUCTED for c in B.drop_in_cases()) and len({c.name for c in B.drop_in_cases()}) == 8


def test_every_stream_lies_in_the_blob_with_its_slack():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gamut_hip.h")).read()
    assert [int(x) for x in re.findall(r"#define GAMUT_HIP_QOI_SLACK (\d+)", header)] == [B.SLACK]
    assert B.DESC.itemsize == C.sizeof(_capi.QoiDesc) == 12 and [B.DESC.fields[f][1] for f in ("width", "height", "channels", "colorspace")] == [
        getattr(_capi.QoiDesc, f).offset for f in ("width", "height", "channels", "colorspace")]
    for label, L, _ in _layouts():
        assert (L.begin.dtype, L.out_offset.dtype, L.size.dtype, L.blob.dtype) == (np.int64, np.int64, np.int32, np.uint8), label
        assert L.begin[0] % 2 == 1 and L.blob.size == L.blob_len == int(L.begin[-1]) + int(L.size[-1]) + B.SLACK, label
        for i, s in enumerate(L.streams):
            assert L.blob[L.begin[i]:L.begin[i] + L.size[i]].tobytes() == s.case.data, (label, s.case.name)
            assert (L.descs[i]["width"], L.descs[i]["height"], L.descs[i]["channels"]) == Q.header(s.case.data), (label, s.case.name)
        ends = L.begin + L.size
        assert (L.begin[1:] - ends[:-1] >= B.SLACK).all() and (ends + B.SLACK <= L.blob_len).all(), label
        res = L.begin % 64
        assert (res[1:] != res[:-1]).all() and set(res.tolist()) == set(range(64)), label
        # what lies between the streams: every kind of fill, really there -- a stream's fill lies in front of it (the slack of the stream before),
        # and the last stream's behind it as well
        assert {s.fill for s in L.streams} == set(B.FILLS), label
        for kind, byte in (("zeros", 0), ("0xFF", 0xFF), ("0xFE", 0xFE), ("0xFD", 0xFD)):
            hit = [i for i in range(1, L.n) if L.streams[i].fill == kind]
            assert hit, (label, kind)
            assert all((L.blob[ends[i - 1]:L.begin[i]] == byte).all() and L.begin[i] - ends[i - 1] >= B.SLACK for i in hit), (label, kind)
            if L.streams[-1].fill == kind:
                assert (L.blob[ends[-1]:] == byte).all() and L.blob_len - ends[-1] == B.SLACK
        i = [k for k in range(1, L.n) if L.streams[k].fill == "stream"][0]
        gap = L.blob[ends[i - 1]:L.begin[i]].tobytes()
        assert gap[:4] == b"qoif" and gap == (L.streams[i].case.data * (len(gap) // L.size[i] + 1))[:len(gap)]
        i = [k for k in range(1, L.n) if L.streams[k].fill == "noise"][0]
        assert len(set(L.blob[ends[i - 1]:L.begin[i]].tolist())) > 64
    # a copy differs from the next one in what lies around it: with seven copies, every case meets every fill
    L = B.resident("one_wave", 0)
    assert all({s.fill for s in L.streams if s.case.name == c.name} == set(B.FILLS) for c in Q.CASES)


def test_no_two_output_ranges_touch():
    hosts = [(f"host-{k}-{ch}", B.host(k, ch), False) for k in (1, 3) for ch in (0, 3)]
    for label, L, _ in _layouts() + hosts:
        ends = L.out_offset + L.out_bytes
        gaps = np.concatenate([L.out_offset[:1], L.out_offset[1:] - ends[:-1], [L.out_len - ends[-1]]])
        assert gaps.min() >= 1 and gaps.max() <= 67 and L.poison.size == L.out_len and (L.poison == B.POISON).all(), label
        assert [int(x) for x in L.out_bytes] == [Q.expected(s.case.name, L.channels).size for s in L.streams]
        # three- and four-channel outputs each begin at every residue mod 16 (an output of `channels` 0 has its file's count)
        assert set(L.out_channels.tolist()) == ({3, 4} if L.channels == 0 else {L.channels}), label
        for ch in set(L.out_channels.tolist()):
            assert set((L.out_offset[L.out_channels == ch] % 16).tolist()) == set(range(16)), (label, ch)
        exp = L.expected_allocation()
        assert not exp.flags.writeable and exp is L.expected_allocation()
        inside = np.zeros(L.out_len, bool)
        for i, s in enumerate(L.streams):
            assert np.array_equal(exp[L.out_offset[i]:ends[i]], Q.expected(s.case.name, L.channels)), (label, s.case.name)
            inside[L.out_offset[i]:ends[i]] = True
        assert (exp[~inside] == B.POISON).all() and inside.sum() == L.out_bytes.sum()


def test_a_wrong_byte_is_reported_by_the_name_of_its_case():
    L = B.resident("one_wave", 0)
    got = L.expected_allocation().copy()
    assert L.first_difference(got) is None
    i = 500
    s, ch = L.streams[i], int(L.out_channels[i])
    got[L.out_offset[i] + 5 * ch + 1] ^= 0x40; got[L.out_offset[i + 3]] ^= 1
    d = L.first_difference(got)
    assert (d.case, d.copy, d.byte, d.pixel) == (s.case.name, s.copy, 5 * ch + 1, 5) and s.case.name in d.text and f"copy {s.copy}" in d.text and "2 bytes differ" in d.text
    got = L.expected_allocation().copy(); got[L.out_offset[i] + L.out_bytes[i]] = 0        # the first byte behind the image
    d = L.first_difference(got)
    assert (d.case, d.copy, d.byte) == (s.case.name, s.copy, int(L.out_bytes[i])) and "gap behind" in d.text
    got = L.expected_allocation().copy(); got[0] = 0
    d = L.first_difference(got)
    assert d.case == L.streams[0].case.name and d.byte == -int(L.out_offset[0]) and "gap in front" in d.text
    assert L.first_difference(got[:-1]).case is None


def test_the_tables_outlive_everything_but_the_layout():
    """The record of the first attempt at tests/test_qoi_batch_gpu.py, which ended in a host segmentation fault: a pointer taken from a temporary
    array (`np.array(...).ctypes.data`) names memory numpy has freed by the time the C call reads it.  Here every pointer comes from an attribute of
    the layout: with nothing alive but the layout, each still reads back as its table."""
    def make(kind):
        L = B.resident("one_wave", 3) if kind == "resident" else B.host(3, 0)
        tables = L.tables()
        addresses = {name: (C.cast(p, C.c_void_p).value, nbytes) for name, (p, nbytes) in tables.items()}
        del tables
        return L, addresses
    for kind in ("resident", "host"):
        L, addresses = make(kind)
        gc.collect()
        churn = [np.full(1 << 20, 0xEE, np.uint8) for _ in range(8)]; del churn          # (freed memory gets reused)
        gc.collect()
        assert set(addresses) >= {"size", "out_offset", "poison", "descs_read"}
        for name, (address, nbytes) in addresses.items():
            assert nbytes > 0 and C.string_at(address, nbytes) == getattr(L, name).tobytes(), (kind, name)
        if kind == "host":
            for i, s in enumerate(L.streams):
                assert C.string_at(int(L.ptrs[i]), int(L.size[i])) == s.case.data, s.case.name
