"""The generated GIF files of the tests, by name: cases() -> list of (name, file bytes, pillow) where pillow says that Pillow and the
reference agree on the file by construction (disposal 0 / 1, no transparency, frames inside the screen, a well-formed stream)."""
import functools

import numpy as np

import gif_gen as g

PAL = g.palette(256, 0)


def _one(name, sw, sh, frames, pillow=False, **kw):
    kw.setdefault("gct", PAL)
    return name, g.make(sw, sh, frames, **kw), pillow


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2024)
    out = []
    # ---- LZW
    for cs in (0, 1, 2, 7, 8, 9, 12):
        levels = min(1 << cs, 256)
        sym = g.noise(rng, 23 * 9, 1 << cs) if cs else np.zeros(23 * 9, np.int64)
        out.append(_one(f"lzw_cs{cs}_noise", 23, 9, [g.frame(0, 0, 23, 9, sym, cs=cs)], pillow=2 <= cs <= 8))
        out.append(_one(f"lzw_cs{cs}_flat", 40, 17, [g.frame(0, 0, 40, 17, g.flat(40, 17, min(levels, 4), 3) if cs else np.zeros(680, np.int64), cs=cs)],
                        pillow=2 <= cs <= 8))
    out.append(_one("kwkwk_runs", 64, 8, [g.frame(0, 0, 64, 8, np.array(([5] * 37 + [1, 2] * 20 + [9] * 3 + [7] * 60) * 4)[:512], cs=4)], pillow=True))
    out.append(_one("flat_96x48", 96, 48, [g.frame(0, 0, 96, 48, np.full(96 * 48, 3), cs=2)], pillow=True))
    out.append(_one("flat_300x40", 300, 40, [g.frame(0, 0, 300, 40, np.full(300 * 40, 1), cs=2)], pillow=True))
    out.append(_one("noise_fills_table", 100, 70, [g.frame(0, 0, 100, 70, g.noise(rng, 7000), cs=8)], pillow=True))
    out.append(_one("deferred_clear_under_8192", 100, 70, [g.frame(0, 0, 100, 70, g.noise(rng, 16000), cs=8, clear_when=8000)]))
    out.append(_one("deferred_clear_crossing_8192", 100, 70, [g.frame(0, 0, 100, 70, g.noise(rng, 16000), cs=8, clear_when=None)]))
    out.append(_one("deferred_clear_cs12", 100, 70, [g.frame(0, 0, 100, 70, g.noise(rng, 9000, 4096), cs=12)]))
    out.append(_one("several_clears", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 16), cs=4, start_clears=3, clears_at={50: 2, 51: 1, 400: 4})]))
    out.append(_one("no_clear_at_start", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 16), cs=4, start_clears=0)]))
    out.append(_one("avail_after_clear", 30, 20, [g.frame(0, 0, 30, 20, cs=4, codes=[g.CLEAR, 18, g.END])]))
    out.append(_one("avail_after_second_clear", 30, 20, [g.frame(0, 0, 30, 20, cs=4, codes=[g.CLEAR, 3, 4, 18, g.CLEAR, 18, g.END])]))
    out.append(_one("code_above_avail", 30, 20, [g.frame(0, 0, 30, 20, cs=4, codes=[g.CLEAR, 3, 4, 21, g.END])]))
    out.append(_one("no_end_code", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 16), cs=4, end=False)], pillow=True))
    out.append(_one("data_after_end_code", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 16), cs=4, block=50, after_end=bytes(range(1, 180)))]))
    out.append(_one("one_byte_subblocks", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 16), cs=4, block=1)], pillow=True))
    out.append(_one("payload_shorter", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 333, 16), cs=4)]))
    out.append(_one("payload_longer", 30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 1500, 16), cs=4)]))
    ok = g.make(30, 20, [g.frame(0, 0, 30, 20, g.noise(rng, 600, 256), cs=8, block=100)], gct=PAL)
    out.append(("truncated_in_subblock", ok[:len(ok) - 150], False))
    out.append(("truncated_before_terminator", ok[:len(ok) - 2], False))
    out.append(("no_trailer", ok[:len(ok) - 1], False))
    # ---- geometry
    for fy in (0, 3):
        for h in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17):
            bgf = g.frame(0, 0, 12, 22, g.noise(rng, 12 * 22, 64), cs=6)
            out.append(_one(f"interlaced_h{h}_y{fy}", 12, 22, [bgf, g.frame(2, fy, 9, h, g.noise(rng, 9 * (h + 9), 64), cs=6, interlace=True)]))
    out.append(_one("interlaced_exact", 31, 29, [g.frame(0, 0, 31, 29, g.photo_like(rng, 31, 29), cs=8, interlace=True)], pillow=True))
    out.append(_one("frame_w0", 20, 10, [g.frame(0, 0, 20, 10, g.noise(rng, 200, 8), cs=3), g.frame(4, 2, 0, 5, g.noise(rng, 30, 8), cs=3)]))
    out.append(_one("frame_h0", 20, 10, [g.frame(0, 0, 20, 10, g.noise(rng, 200, 8), cs=3), g.frame(4, 2, 7, 0, g.noise(rng, 30, 8), cs=3),
                                         g.frame(1, 1, 5, 0, g.noise(rng, 60, 8), cs=3, interlace=True)]))
    out.append(_one("overhang_bottom", 20, 10, [g.frame(3, 6, 10, 9, g.noise(rng, 90, 8), cs=3), g.frame(1, 4, 6, 30, g.noise(rng, 180, 8), cs=3, interlace=True)]))
    out.append(_one("frame_below_screen", 20, 10, [g.frame(3, 12, 10, 4, g.noise(rng, 40, 8), cs=3)]))
    out.append(_one("overhang_right", 20, 10, [g.frame(12, 2, 9, 4, g.noise(rng, 36, 8), cs=3)]))
    out.append(_one("no_colour_table", 20, 10, [g.frame(0, 0, 20, 10, g.noise(rng, 200, 8), cs=3)], gct=None))
    out.append(_one("lct_only", 20, 10, [g.frame(0, 0, 20, 10, g.noise(rng, 200, 8), cs=3, lct=g.palette(8, 5))], gct=None, pillow=True))
    # ---- compositing
    rects = [(0, 0, 40, 30), (5, 4, 20, 15), (15, 10, 22, 18), (2, 12, 30, 9), (10, 2, 12, 26)]
    for d in (0, 1, 2, 3):
        fr = [g.frame(x, y, w, h, g.noise(rng, w * h, 32), cs=5, gce_bytes=g.gce(d, None, 4 + k)) for k, (x, y, w, h) in enumerate(rects)]
        out.append(_one(f"disposal_{d}", 40, 30, fr, pillow=d < 2))
    fr = [g.frame(x, y, w, h, g.noise(rng, w * h, 32), cs=5, gce_bytes=g.gce((k * 7) % 4, None if k == 2 else 3 + k, 3)) for k, (x, y, w, h) in enumerate(rects)]
    out.append(_one("mixed_disposal_transparency_gct", 40, 30, fr))
    fr = [g.frame(x, y, w, h, g.noise(rng, w * h, 32), cs=5, lct=g.palette(32, k) if k % 2 else None, gce_bytes=g.gce(2 if k == 1 else 1, 7, 3))
          for k, (x, y, w, h) in enumerate(rects)]
    out.append(_one("transparency_lct", 40, 30, fr))
    fr = [g.frame(x, y, w, h, g.noise(rng, w * h, 32), cs=5, gce_bytes=g.gce(2, 9, 3) if k in (0, 1, 3) else b"") for k, (x, y, w, h) in enumerate(rects)]
    out.append(_one("later_frame_without_gce", 40, 30, fr))
    fr = [g.frame(x, y, w, h, g.noise(rng, w * h, 32), cs=5, gce_bytes=g.gce(2, 11, 30) if k == 4 else b"") for k, (x, y, w, h) in enumerate(rects)]
    out.append(_one("first_frame_sees_last_gce", 40, 30, fr))
    out.append(_one("gce_after_last_frame", 40, 30, [g.frame(0, 0, 40, 30, g.noise(rng, 1200, 32), cs=5), g.frame(3, 3, 9, 9, g.noise(rng, 81, 32), cs=5)],
                    tail=g.gce(2, 5, 7)))
    fr = [g.frame(0, 0, 40, 30, g.noise(rng, 1200, 256), cs=8, lct=g.palette(256, 1)), g.frame(4, 4, 30, 20, g.noise(rng, 600, 256), cs=8, lct=g.palette(4, 2)),
          g.frame(0, 0, 40, 30, g.noise(rng, 1200, 256), cs=8)]
    out.append(_one("stale_lct_entries", 40, 30, fr, gct=g.palette(16, 3)))
    out.append(_one("index_past_every_table", 40, 30, [g.frame(0, 0, 40, 30, g.noise(rng, 1200, 256), cs=8)], gct=g.palette(4, 4)))
    out.append(_one("transparent_index_past_gct", 40, 30, [g.frame(0, 0, 40, 30, g.noise(rng, 1200, 256), cs=8, gce_bytes=g.gce(1, 200, 2)),
                                                           g.frame(0, 0, 40, 30, g.noise(rng, 1200, 256), cs=8, gce_bytes=g.gce(1, None, 2))], gct=g.palette(4, 4)))
    out.append(_one("zero_frames", 40, 30, []))
    out.append(_one("zero_frames_gif87", 7, 5, [], version=b"GIF87a", aspect=49, tail=g.comment() + g.app_ext(3) + g.plain_text()))
    out.append(_one("extensions_and_aspect", 16, 16, [g.frame(0, 0, 16, 16, g.noise(rng, 256, 4), cs=2, pre=g.app_ext() + g.comment(b"x" * 300), gce_bytes=g.gce(0, None, 1)),
                                                       g.frame(1, 1, 8, 8, g.noise(rng, 64, 4), cs=2, pre=g.plain_text(), gce_bytes=g.gce(1, None, 0))], aspect=113, pillow=True))
    out.append(_one("unknown_extension", 16, 16, [g.frame(0, 0, 16, 16, g.noise(rng, 256, 4), cs=2, pre=b"\x21\x77\x02ab\x00")]))
    out.append(_one("bad_gce_size", 16, 16, [g.frame(0, 0, 16, 16, g.noise(rng, 256, 4), cs=2, gce_bytes=g.gce(size=5))]))
    out.append(_one("bad_gce_terminator", 16, 16, [g.frame(0, 0, 16, 16, g.noise(rng, 256, 4), cs=2, gce_bytes=g.gce(terminator=1))]))
    out.append(_one("lzw_cs_13", 16, 16, [g.frame(0, 0, 16, 16, cs=13, payload=b"\x00\x01")]))
    out.append(_one("zero_by_zero_screen", 0, 0, []))
    out.append(_one("zero_height_screen", 9, 0, [g.frame(0, 0, 9, 4, g.noise(rng, 36, 4), cs=2)]))
    return out


def three_frames():
    """a 3-frame file for the Image tests: noise, a flat sub-rectangle, an interlaced photo-like one; disposal 1 and 2, one transparent index"""
    rng = np.random.default_rng(77)
    fr = [g.frame(0, 0, 37, 21, g.noise(rng, 37 * 21), cs=8, gce_bytes=g.gce(1, None, 5)),
          g.frame(4, 3, 20, 11, g.flat(20, 11, 4, 3), cs=8, gce_bytes=g.gce(2, 2, 7)),
          g.frame(9, 1, 25, 19, g.photo_like(rng, 25, 19), cs=8, interlace=True, gce_bytes=g.gce(1, None, 9))]
    return g.make(37, 21, fr, gct=PAL, aspect=49)


def large():
    """640 x 480, 8 frames: full-screen photo-like and flat frames and sub-rectangles with disposal and transparency"""
    rng = np.random.default_rng(640)
    fr = []
    for k in range(8):
        if k % 4 == 0:
            x, y, w, h = 0, 0, 640, 480
        else:
            w, h = int(rng.integers(200, 640)), int(rng.integers(150, 480))
            x, y = int(rng.integers(0, 640 - w + 1)), int(rng.integers(0, 480 - h + 1))
        sym = g.photo_like(rng, w, h) if k % 2 == 0 else g.flat(w, h, 8, 16)
        fr.append(g.frame(x, y, w, h, sym, cs=8, interlace=k == 3, gce_bytes=g.gce(k % 3, 4 if k in (2, 5) else None, 4)))
    return g.make(640, 480, fr, gct=PAL)


def mutated(n, seed):
    """n mutated small files -> list of bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        b, spans = g.small_valid(rng)
        out.append(g.mutate(b, spans, rng))
    return out
