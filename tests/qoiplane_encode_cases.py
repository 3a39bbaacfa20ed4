"""Named images for the QOI-Plane encoder: (name, (h, w, 1 | 2) uint8 array).  HAND_WORKED carries the stream behind the header, worked
out by hand from the format description, as hex.  Cases that depend on the encoder's geometry take the segment size S
(gamut_hip_qoix_plane_encode_segment()) as an argument and use no literal.

A full segment of S >= 258 pixels without a pixel that differs still emits its REPEAT2 ops of 258, so "a segment that emits nothing" is
here a segment in which no pixel differs: what it emits is the closed form of the run count that enters it."""
import functools

import numpy as np

import qoiplane_gen as P


def image(raster, w, ch):
    """a flat list of l values (1 channel) or (l, a) pairs -> (h, w, ch)"""
    return np.asarray(raster, np.uint8).reshape(-1, w, ch)


def row(raster, ch):
    return image(raster, len(raster), ch)


HAND_WORKED = [
    # 100 from 0: DIRECT a 64; 103: +3 DIFF1 7; 87: -16 DIFF2 80
    ("direct_diff1_diff2", row([100, 103, 87], 1), "a64780ffffffffff"),
    # 254 from 0: (int8)254 = -2, DIFF1 2; 2 from 254: (int8)(2 - 254) = 4, DIFF2 94
    ("int8_wraps_254_then_2", row([254, 2], 1), "294fffffffff"),
    # 77 (DIRECT a 4d), then 600 repeats: 258 (f fe), 258 (f fe), and 84 at the last pixel (f 50)
    ("run_of_600_cut_258_258_84", row([77] * 601, 1), "a4dffeffef50ffffffffff"),
    # 99 (DIRECT a 63), then two repeats ending at the last pixel: REPEAT1 d
    ("run_ending_at_the_last_pixel", row([99, 99, 99], 1), "a63dffffffffff"),
    # (5, 200): LA b0 05 c8; (5, 202): ADIFF +2 ba, DIFF1 0 4; the repeat at the last pixel: c
    ("la_adiff_repeat", row([(5, 200), (5, 202), (5, 202)], 2), "b005c8ba4cffffffffff"),
    # two pixels equal to the initial state {0, 255}: one REPEAT1 of 2
    ("run_from_pixel_0", row([(0, 255), (0, 255)], 2), "dfffffffff"),
    # (50, 250): ADIFF -5 b3, DIRECT a 32; (50, 251): ADIFF +1 b9 and DIFF1 0 (4) although only alpha changed; (60, 252): b9, DIFF2 +10 9a
    ("adiff_in_front_of_direct_diff1_diff2", row([(50, 250), (50, 251), (60, 252)], 2), "b3a32b94b99affffffffff"),
    # 10 from 0: DIFF2 9a; 13: DIFF1 7.  Row 1, column 0: ref is 13 (the row above's last pixel), top is 10: average (10 + 13 + 1) / 2 = 12,
    # so 12 is DIFF1 0 (4); then 13 against (13 + 12 + 1) / 2 = 13: 4.  Five nibbles and nine: no tenth f
    ("column_0_of_row_1", image([10, 13, 12, 13], 2, 1), "9a744fffffffff"),
]

KIND_NIBBLES = {"1": 1, "2": 2, "D": 3, "L": 6, "A": 3, "a": 3}


def from_kinds(kinds, ch):
    """one row from op kinds: 1 DIFF1 (+1), 2 DIFF2 (+10), D DIRECT (+100), L an LA (both + 100), A ADIFF and DIFF1 (both + 1), a an
    alpha-only step (ADIFF, DIFF1 of 0), R a repeat"""
    l, a, out = 0, 255, []
    for k in kinds:
        l = (l + {"1": 1, "2": 10, "D": 100, "L": 100, "A": 1}.get(k, 0)) & 255
        a = (a + {"L": 100, "A": 1, "a": 1}.get(k, 0)) & 255
        out.append((l, a) if ch == 2 else l)
    assert ch == 2 or not set(kinds) & set("LAa")
    return row(out, ch)


def shape_for(n):
    """(w, h) with w * h == n and, where n has a small factor, more than one row"""
    for h in range(2, 70):
        if n % h == 0:
            return n // h, h
    return n, 1


def distinct(n):
    """n luminance values, no two neighbours equal"""
    return [(i * 37) % 251 for i in range(n)]


def with_plateau(n, p, length, ch):
    """n pixels, no two neighbours equal, except that the `length` pixels behind pixel p repeat it"""
    v = distinct(n)
    assert p >= 0 and p + length <= n - 1 and (length + 1) % 251
    v[p + 1:p + 1 + length] = [v[p]] * length
    return [(x, (x * 3) & 255) for x in v] if ch == 2 else v


@functools.lru_cache(maxsize=None)
def geometry(S):
    out = []
    for w in (1, 3, 63, 64, 65):
        for h in (1, 2, 40):
            for ch in (1, 2):
                out.append((f"geometry_{w}x{h}_{ch}ch", P.noisy(w, h, ch, 7 * w + h + ch)))
    for n in (S - 1, S, S + 1, 2 * S + 1, 3 * S + 7):
        w, h = shape_for(n)
        for ch in (1, 2):
            out.append((f"pixels_{n}_as_{w}x{h}_{ch}ch", P.noisy(w, h, ch, n + ch)))
    for ch in (1, 2):
        out.append((f"width_1_height_{2 * S + 5}_{ch}ch", P.noisy(1, 2 * S + 5, ch, 3 + ch)))
        out.append((f"photo_like_201x149_{ch}ch", P.photo_like(201, 149, ch, ch)))
        out.append((f"flat_199x151_{ch}ch", P.flat_image(199, 151, ch, 2 + ch)))
        out.append((f"few_levels_130x70_{ch}ch", P.few_levels(130, 70, ch, 5 + ch)))
    out.append(("alpha_ramp_77x131", P.alpha_ramp(77, 131, 3)))
    out.append(("alpha_ramp_step_9_90x100", P.alpha_ramp(90, 100, 4, step=9)))
    return out


@functools.lru_cache(maxsize=None)
def runs(S):
    out = []
    for ch in (1, 2):
        for r in (1, 2, 3, 4, 257, 258, 259, 516, 517, 520):
            n = r + 9
            out.append((f"run_of_{r}_{ch}ch", row(with_plateau(n, 3, r, ch), ch)))
            init = [(0, 255)] * r + [(9, 255), (9, 250)] if ch == 2 else [0] * r + [9, 11]
            out.append((f"run_of_{r}_from_pixel_0_{ch}ch", row(init, ch)))
            out.append((f"run_of_{r}_is_the_whole_image_{ch}ch", row(init[:r], ch)))
        flat = np.full((3 * S // 64, 64, ch), 77, np.uint8)
        out.append((f"flat_{3 * S}_pixels_{ch}ch", flat))
        out.append((f"flat_{3 * S}_pixels_of_the_initial_state_{ch}ch", np.full((3 * S // 64, 64, ch), (0, 255)[:ch], np.uint8)))
        n = 2 * S + 40
        out.append((f"run_reaches_258_on_a_segments_last_pixel_{ch}ch", row(with_plateau(n, S - 1 - 258, 300, ch), ch)))
        out.append((f"run_reaches_258_on_a_segments_first_pixel_{ch}ch", row(with_plateau(n, S - 258, 300, ch), ch)))
        out.append((f"run_reaches_258_twice_at_segment_ends_{ch}ch", image(with_plateau(n, 2 * S - 1 - 516, 520, ch), n // 2, ch)))
        out.append((f"run_of_258_ends_at_the_last_pixel_{ch}ch", row(with_plateau(S + 300, S + 300 - 1 - 258, 258, ch), ch)))
        out.append((f"run_of_258_ends_at_the_last_pixel_of_a_full_segment_{ch}ch", row(with_plateau(2 * S, 2 * S - 1 - 258, 258, ch), ch)))
        out.append((f"run_of_259_ends_at_the_last_pixel_{ch}ch", row(with_plateau(S + 300, S + 300 - 1 - 259, 259, ch), ch)))
        out.append((f"run_across_two_segment_boundaries_{ch}ch", row(with_plateau(3 * S + 11, S - 5, 2 * S + 7, ch), ch)))
    return out


@functools.lru_cache(maxsize=None)
def shared_bytes(S):
    """one row; the first segment ends on an odd nibble, so that the boundary byte is shared"""
    out = []
    heads = {"direct": "1" * (S - 2) + "2" + "D", "diff2": "1" * (S - 1) + "2", "la": "1" * (S - 1) + "L"}
    first = {"direct": "D", "diff2": "2", "la": "L"}
    for name, head in heads.items():                                        # the op kind on both sides of the boundary
        ch = 2 if "L" in head else 1
        assert len(head) == S and sum(KIND_NIBBLES[k] for k in head) % 2 == 1
        out.append((f"{name}_on_both_sides_of_an_odd_boundary_{ch}ch", from_kinds(head + first[name] + "1" * 70 + "D2" * 9, ch)))
    head = "1" * (S - 1) + "2"
    for ch in (1, 2):
        out.append((f"segment_without_a_differing_pixel_between_two_that_share_a_byte_{ch}ch", from_kinds(head + "R" * S + "D" + "12" * 20, ch)))
        out.append((f"two_odd_boundaries_in_a_row_{ch}ch", from_kinds(head + "1" * (S - 1) + "D" + "2" * 30, ch)))
        out.append((f"even_boundaries_{ch}ch", from_kinds("1" * S + "12" * (S // 2) + "D" * 30, ch)))
    out.append(("adiff_pairs_across_an_odd_boundary_2ch", from_kinds("1" * (S - 3) + "2" + "A" + "a" + "A" * 40 + "L" * 3, 2)))
    return out


def thresholds():
    out = []
    ds = (-17, -16, -5, -4, 3, 4, 15, 16, -128, 127, 0, 1, -1)
    for base in (100, 250, 3, 0, 255, 128):                                  # one row: the average is the predecessor
        seq = []
        for d in ds:
            seq += [base, (base + d) & 255] if d else [base, (base + 50) & 255]
        out.append((f"d_thresholds_from_{base}", row(seq, 1)))
    rng = np.random.default_rng(11)                                          # two rows: the average is that of the pixel above and the predecessor
    for k in range(4):
        w = 60
        img = np.zeros((2, w, 1), np.uint8)
        img[0, :, 0] = rng.integers(0, 256, w)
        ref = int(img[0, -1, 0])
        for x in range(w):
            avg = (int(img[0, x, 0]) + ref + 1) // 2
            d = ds[(x + k) % 10] or 1
            ref = (avg + d) & 255
            img[1, x, 0] = ref
        out.append((f"d_thresholds_against_the_average_{k}", img))
    for a0 in (100, 3, 250, 255, 0):
        seq, l = [], 10
        for va in (-8, -7, 7, 8, -1, 1, 127, -128):
            l = (l + 5) & 255
            seq += [(l, a0), (l, (a0 + va) & 255), ((l + 40) & 255, (a0 + 2 * va) & 255)]        # alpha alone, then alpha and luminance
        out.append((f"va_thresholds_from_{a0}", row(seq, 2)))
    out.append(("alpha_only_changes", row([(80, 10 + 3 * k) for k in range(40)] + [(80, 200), (80, 20)], 2)))
    return out


@functools.lru_cache(maxsize=None)
def named(S):
    return [(n, im) for n, im, _ in HAND_WORKED] + geometry(S) + runs(S) + shared_bytes(S) + thresholds() + boundary_images() + [byu32_image()]


# lz4Size + 4 - datalen of -1, 0 and +1: found by a seed search over few_levels(w, 3, ch, seed, levels) (see find_boundary)
BOUNDARY_SEEDS = [(20, 2, 37, 3, 0), (24, 2, 41, 4, -1), (40, 1, 20, 4, -1), (42, 1, 22, 3, 1), (46, 1, 100, 3, 0), (53, 2, 33, 2, 1)]


def find_boundary(want=(-1, 0, 1), tries=4000):
    """the search that produced BOUNDARY_SEEDS"""
    import qoiplane_write_ref_c as ref
    found = {}
    for seed in range(tries):
        w, ch, levels = 20 + seed % 37, 1 + seed % 2, 2 + seed % 3
        d = ref.encode_ex(P.few_levels(w, 3, ch, seed, levels))[1]
        if d in want and (d, ch) not in found:
            found[(d, ch)] = (w, ch, seed, levels, d)
    return sorted(found.values())


def boundary_images():
    return [(f"container_choice_diff_{d:+d}_{w}x3_{ch}ch", P.few_levels(w, 3, ch, seed, levels)) for w, ch, seed, levels, d in BOUNDARY_SEEDS]


def boundary_diffs():
    return [d for *_, d in BOUNDARY_SEEDS]


def byu32_image():
    """an op stream of at least 65547 bytes: LZ4's byU32 form"""
    return "noise_256x184_1ch", np.random.default_rng(5).integers(0, 256, (184, 256, 1), dtype=np.uint8)


def parse_ops(body, pixels, ch):
    """the stream behind the header -> op kinds, as a decoder reads them for `pixels` pixels; also the number of nibbles in front of the
    closing ones"""
    nib = [x for b in body for x in (b >> 4, b & 15)]
    kinds, p, done = [], 0, 0
    while done < pixels:
        t = nib[p]
        if t < 8:
            kinds.append("DIFF1"); p += 1; done += 1
        elif t < 10:
            kinds.append("DIFF2"); p += 2; done += 1
        elif t == 10:
            kinds.append("DIRECT"); p += 3; done += 1
        elif t == 11:
            if nib[p + 1] == 0:
                kinds.append("LA"); p += 6; done += 1
            else:
                kinds.append("ADIFF"); p += 2
        elif t < 15:
            kinds.append("REPEAT1"); p += 1; done += (t & 3) + 1
        else:
            kinds.append("REPEAT2"); done += (nib[p + 1] << 4 | nib[p + 2]) + 4; p += 3
    assert done == pixels
    return kinds, p
