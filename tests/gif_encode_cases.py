"""Named inputs for the GIF encoder.  Every case carries `expect`: a predicate on the C reference's per-frame report
(tests/gif_encode_ref_c.py) -- and, where the name is about a field of the file, on the reference's file bytes -- which says that the
case hits what its name says; all_cases() evaluates it, so a case that drifts off its
target fails where it is built and not silently in a comparison of two equally wrong files.

Case = (name, frames (n, h, w, 4) uint8, kwargs for encode(), expect(report list, file bytes) -> bool)."""
import functools

import numpy as np

import gif_encode_ref_c as R

OPAQUE = 255


def _rgba(rgb, alpha=OPAQUE):
    rgb = np.asarray(rgb, np.uint8)
    return np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), alpha, np.uint8)], axis=-1)


def noise(w, h, seed, frames=1):
    return _rgba(np.random.default_rng(seed).integers(0, 256, (frames, h, w, 3), dtype=np.uint8))


def few(w, h, ncol, seed, frames=1):
    """random pixels out of `ncol` stable colours (see stable_colours)"""
    pal = stable_colours(ncol)
    idx = np.random.default_rng(seed).integers(0, ncol, (frames, h, w))
    return _rgba(pal[idx])


@functools.lru_cache(maxsize=None)
def _stable_levels():
    """Channel values that cook to ONE value at depth 16 whatever the dither adds: for 5 bits the product v * 249 must lie at least
    61440 >> 5 below the next multiple of 2048, for 6 bits v * 253 at least 61440 >> 6 below the next multiple of 1024."""
    s5 = [v for v in range(256) if (v * 249) % 2048 + (61440 >> 5) < 2048]
    s6 = [v for v in range(256) if (v * 253) % 1024 + (61440 >> 6) < 1024]
    # one level per cooked value
    s5 = list({(v * 249) >> 11: v for v in s5}.values()); s6 = list({(v * 253) >> 10: v for v in s6}.values())
    return s5, s6


def stable_colours(n):
    """n colours with n distinct cooked values at depth 16"""
    s5, s6 = _stable_levels()
    cols = [(r, g, b) for b in s5 for g in s6 for r in s5]
    assert len(cols) >= n
    step = max(1, len(cols) // n)
    return np.array(cols[::step][:n], np.uint8)


def exact_colours(w, h, n):
    """an image that uses each of n stable colours at least once"""
    pal = stable_colours(n)
    assert w * h >= n
    return _rgba(pal[(np.arange(w * h) % n).reshape(1, h, w)])


def gradient(w, h):
    x = np.arange(w)[None, :] * 255 // max(1, w - 1)
    img = np.zeros((1, h, w, 3), np.uint8)
    img[0, ..., 0] = x
    img[0, ..., 1] = (np.arange(h)[:, None] * 255 // max(1, h - 1)) // 64 * 64
    return _rgba(img)


def photo_like(w, h, frames, seed):
    """smooth fields plus a little noise, drifting from frame to frame"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((frames, h, w, 3), np.float64)
    for f in range(frames):
        for c in range(3):
            out[f, ..., c] = 128 + 90 * np.sin(x / (11.0 + 3 * c) + 0.3 * f) * np.cos(y / (17.0 - 2 * c) - 0.2 * f) + rng.normal(0, 6, (h, w))
    return _rgba(np.clip(out, 0, 255).astype(np.uint8))


def scan_framing(kind, w0=40, w1=4000, h=4, ncol=3, seed=1):
    """how the framing cases below were found: the first width at which the C reference reports `kind` for a one-frame image of random
    stable colours (and, for LAST_PARTIAL, a single sub-block)"""
    for w in range(w0, w1):
        rep = R.encode(few(w, h, ncol, seed))[1][0]
        if rep["last_kind"] == kind:
            return w
    return None


FRAMING_EXACTLY_FULL_W = 519           # scan_framing(R.LAST_EXACTLY_FULL)
FRAMING_NOTHING_LEFT_W = 250           # scan_framing(R.LAST_NONE_AFTER_ROLLOVER)


def _cases():
    c = []

    def add(name, frames, expect, **kw):
        """expect: predicate on the report, or on (report, file bytes) when it is marked with `expect.wants_file = True`"""
        c.append((name, np.ascontiguousarray(frames), kw, expect))

    def on_file(fn):
        fn.wants_file = True
        return fn

    def size_hits(w, h, body, tail, waves):
        """body / tail: the rows have a 4-pixel vector part / a scalar rest; waves: 64-pixel stretches of the parse.  The file carries
        the size in the header and in every image descriptor; noise this small has a colour per pixel and stays at depth 16 below 256
        pixels, and must leave depth 16 from 256 pixels on"""
        def check(r, data):
            le = w.to_bytes(2, "little") + h.to_bytes(2, "little")
            px = w * h
            return ((body, tail, waves) == (w >= 4, w % 4 != 0, (px + 63) // 64) and data[6:10] == le and data[32 + 13:32 + 17] == le and len(r) == 2
                    and all((x["count"] == px and x["depth"] == 16) if px < 256 else x["depth"] < 16 for x in r))
        return on_file(check)

    # ---- widths and heights: vector body, tail, wave edges
    for w, h, body, tail, waves in ((1, 1, False, True, 1), (3, 1, False, True, 1), (1, 5, False, True, 1), (5, 3, True, True, 1), (7, 4, True, True, 1),
                                    (64, 1, True, False, 1), (65, 2, True, True, 3), (257, 3, True, True, 13)):
        add(f"size_{w}x{h}", noise(w, h, 100 + w + h, frames=2), size_hits(w, h, body, tail, waves))
    # ---- colour counts at depth 16 -> table bits 2 .. 8, and the 255 / 256 boundary
    for n, tb in ((1, 2), (2, 2), (3, 2), (4, 3), (5, 3), (16, 5), (40, 6), (100, 7), (255, 8)):
        add(f"colours_{n}", exact_colours(32, 16, n), lambda r, n=n, tb=tb: r[0]["depth"] == 16 and r[0]["count"] == n and r[0]["table_bits"] == tb)
    add("colours_256_drops_a_depth", exact_colours(32, 16, 256), lambda r: r[0]["depth"] < 16 and r[0]["count"] < 256)
    add("noise_128x96", noise(128, 96, 7), lambda r: r[0]["depth"] <= 13 and r[0]["resets"] >= 1)
    add("gradient_stays_16", gradient(96, 40), lambda r: r[0]["depth"] == 16)
    # ---- the depth heuristic
    add("few_then_noise", np.concatenate([few(48, 32, 4, 1), noise(48, 32, 2)]), lambda r: r[0]["depth"] == 16 and r[1]["depth"] < 16)
    add("noise_then_few", np.concatenate([noise(48, 32, 3), few(48, 32, 4, 4)]), lambda r: r[0]["depth"] < 16 and r[1]["depth"] == r[0]["depth"] + 160 // r[0]["count"] < 16)      # alone, frame 1 would stay at 16
    # ---- frame differencing
    f0 = few(40, 24, 6, 5)
    add("identical_frames", np.concatenate([f0, f0]), lambda r: r[1]["compatible"] == 1)
    f1 = f0.copy(); f1[0, 11, 17, :3] = (255, 255, 255)
    changed = R.cook_both(f1[0, 11, 17], 17, 11, 16, 10)[1] != R.cook_both(f0[0, 11, 17], 17, 11, 16, 10)[1]     # the edit changes the cooked value
    add("one_changed_pixel", np.concatenate([f0, f1]), lambda r: changed and r[1]["compatible"] == 1 and r[0]["depth"] == r[1]["depth"] == 16)
    f2 = f0.copy(); f2[0, 9, :, :3] = f2[0, 10, ::-1, :3]
    add("one_changed_row", np.concatenate([f0, f2, f0]), lambda r: r[1]["compatible"] == 1 and r[2]["compatible"] == 1)
    add("bit_splits_differ", np.concatenate([few(40, 24, 6, 5), noise(40, 24, 6), noise(40, 24, 6)]),
        lambda r: r[1]["compatible"] == 0 and r[1]["depth"] != r[0]["depth"] and r[2]["compatible"] == 1)
    # ---- transparency
    a = few(16, 8, 5, 8); a[0, :, 0::2, 3] = 9; a[0, :, 1::2, 3] = 10
    add("alpha_9_and_10", a, lambda r: r[0]["has_transparent"] == 1 and r[0]["count"] >= 1)
    t = few(9, 7, 3, 9); t[..., 3] = 0
    add("fully_transparent", t, lambda r: r[0]["has_transparent"] == 1 and r[0]["count"] == 0 and r[0]["table_bits"] == 2)
    g = few(20, 10, 4, 10, frames=2); g[0, 3, 4, 3] = 0
    add("transparent_in_frame_0_only", g, lambda r: r[0]["has_transparent"] == 1 and r[1]["has_transparent"] == 0)
    g = few(20, 10, 4, 11, frames=3); g[2] = g[1]; g[1] = g[0]; g[1, 5, 6, 3] = 3
    add("transparent_in_frame_2_of_3", g, lambda r: [x["has_transparent"] for x in r] == [0, 1, 0] and r[1]["compatible"] == 0 and r[2]["compatible"] == 1)
    g = few(12, 6, 4, 12); g[0, ::2, :, 3] = 0
    add("alpha_threshold_0", g, lambda r: r[0]["has_transparent"] == 0, alpha_threshold=0)
    # ---- sub-block framing
    add("stream_below_255", few(30, 4, 3, 1), lambda r: r[0]["sub_blocks"] == 1 and r[0]["last_kind"] == R.LAST_PARTIAL)
    add("last_sub_block_exactly_full", few(FRAMING_EXACTLY_FULL_W, 4, 3, 1), lambda r: r[0]["last_kind"] == R.LAST_EXACTLY_FULL)
    add("nothing_left_after_rollover", few(FRAMING_NOTHING_LEFT_W, 4, 3, 1), lambda r: r[0]["last_kind"] == R.LAST_NONE_AFTER_ROLLOVER)
    # ---- argument clamps
    m = np.concatenate([noise(33, 9, 13), few(33, 9, 7, 14)])
    for d in (1, 5, 8, 16, 0, 40):
        add(f"max_bit_depth_{d}", m, lambda r, d=d: all(x["depth"] <= max(1, min(16, d)) for x in r) and (d != 0 or r[0]["depth"] == 1), max_bit_depth=d)
    for cs in (0, 7, 65535, 70000):
        add(f"centiseconds_{cs}", few(6, 5, 3, 15), on_file(lambda r, data, cs=cs: data[32 + 4:32 + 6] == (cs & 0xFFFF).to_bytes(2, "little")), centiseconds=cs)
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(name, frames, kwargs, reference file bytes, report)], every case checked against its own name"""
    out = []
    for name, frames, kw, expect in _cases():
        data, rep = R.encode(frames, **kw)
        assert expect(rep, data) if getattr(expect, "wants_file", False) else expect(rep), (name, rep)
        out.append((name, frames, kw, data, rep))
    return out
