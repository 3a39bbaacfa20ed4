"""TGAEncoder (source/gamut/codecs/tga.d:57-281) read on POSITIONS rather than with a cursor: which pixels start a packet is worked
out from the runs of equal pixels, the way the GPU kernel does it (gamut_amd/csrc/tga_encode.hip), with numpy.  The second of the two
independent restatements; the first, tests/c/tga_write_ref.c, walks the row as the reference does.

A run is a maximal stretch of two or more equal pixels, P its first pixel, O its last.  It is entered at P + e (e = 1: the raw packet in
front took P) and cut into packets of 128 from there; if (O - P + 1 - e) % 128 == 1 its last pixel is left over and the raw packets
behind the run start there, else at O + 1; raw packets sit 128 apart from that entry, and the next run has e = 0 exactly when its
first pixel is such a start."""
import numpy as np


def file_channels(comp):
    return 3 if comp in (1, 3) else 4


def convert(img):
    """(h, w, comp) source -> (h, w, file channels) in file byte order B, G, R (, A), rows still top-down"""
    img = np.asarray(img, np.uint8)
    comp = img.shape[2]
    if comp == 1:
        return np.repeat(img, 3, axis=2)
    if comp == 2:
        return np.concatenate([np.repeat(img[:, :, :1], 3, axis=2), img[:, :, 1:]], axis=2)
    return np.concatenate([img[:, :, 2::-1], img[:, :, 3:]], axis=2)


def converted_source(img):
    """what a decoder must give back for the file: (h, w, file channels) in R, G, B (, A) order, top-down"""
    f = convert(img)
    return np.concatenate([f[:, :, 2::-1], f[:, :, 3:]], axis=2)


def _behind(mask):
    """per x: how many consecutive True of mask follow x, capped at 127 (the row's end stops the count)"""
    w = mask.size
    x = np.arange(w)
    stop = np.minimum.accumulate(np.where(~mask, x, w)[::-1])[::-1]        # the first False at or behind x
    return np.minimum(np.append(stop[1:], w) - x - 1, 127)


def row_plan(px):
    """px: (w, fc) -> (start, emit, op) per pixel: starts a packet, has its bytes in the file, the packet byte where it starts one"""
    w = px.shape[0]
    x = np.arange(w)
    sim = np.zeros(w, bool)
    sim[1:] = (px[1:] == px[:-1]).all(axis=1)
    nxt = np.append(sim[1:], False)
    op = np.where(nxt, 0x80 | _behind(sim), _behind(~sim))
    first = ~sim & nxt
    P = np.maximum.accumulate(np.where(first, x, -1))
    O = np.maximum.accumulate(np.where(sim, x, -1))

    def entry(p, o, e):
        return 0 if p < 0 else (o if (o - p + 1 - e) % 128 == 1 else o + 1)
    e_at = np.zeros(w, np.int64)
    firsts = np.flatnonzero(first)
    e, pp, po = 0, -1, -1
    for i, s in enumerate(firsts):                                          # the one serial chain: a two-state map per run
        e = int((s - entry(pp, po, e)) % 128 != 0)
        e_at[s] = e
        pp, po = int(s), int(O[(firsts[i + 1] if i + 1 < firsts.size else w) - 1])
    e_of = np.where(P >= 0, e_at[np.maximum(P, 0)], 0)
    in_run = sim | first
    k = x - P
    run_start = in_run & (k >= e_of) & ((k - e_of) % 128 == 0)
    ent = np.where(P < 0, 0, np.where((O - P + 1 - e_of) % 128 == 1, O, O + 1))
    raw_start = ~in_run & ((x - ent) % 128 == 0)
    start = run_start | raw_start
    emit = np.where(in_run, (k < e_of) | run_start, True)
    return start, emit, op


def encode_row(px, rle=True):
    w, fc = px.shape
    if not rle:
        return px.tobytes()
    start, emit, op = row_plan(px)
    cells = np.zeros((w, 1 + fc), np.uint8)
    cells[:, 0] = op
    cells[:, 1:] = px
    keep = np.zeros((w, 1 + fc), bool)
    keep[:, 0] = start
    keep[:, 1:] = emit[:, None]
    return cells[keep].tobytes()


def packets(values):
    """one row of l8 values -> its packets as strings: 'R5' a run-length packet of 5 pixels, 'raw3' a raw one of 3"""
    px = convert(np.asarray(values, np.uint8).reshape(1, -1, 1))[0]
    start, _, op = row_plan(px)
    return [("R" if o & 0x80 else "raw") + str((o & 127) + 1) for o in op[start]]


def header(w, h, fc, rle=True):
    hd = bytearray(18)
    hd[2] = 10 if rle else 2
    hd[12:16] = bytes([w & 255, w >> 8, h & 255, h >> 8])
    hd[16] = fc * 8
    return bytes(hd)


def encode(img, rle=True):
    """(h, w, comp) uint8 -> the file's bytes"""
    f = convert(img)
    h, w, fc = f.shape
    return header(w, h, fc, rle) + b"".join(encode_row(f[y], rle) for y in range(h - 1, -1, -1))


def bound(w, h, comp):
    if not (1 <= w <= 65535 and 1 <= h <= 65535 and 1 <= comp <= 4):
        return 0
    b = 18 + w * h * (file_channels(comp) + 1)
    return 0 if b > 2 ** 31 - 1 else b
