"""Named QOI-Plane test files: (name, file bytes, expectation) with expectation "ok" or "refused", as the library sees them with
gamut_hip_qoix_set_plane(1).  The name says what a case is about.  hand_worked() carries the pixels worked out by hand as a fourth
element.  Cases that depend on the kernel's geometry take it as an argument (gamut_hip_qoix_plane_row_capacity()) and use no literal."""
import functools
import struct

import numpy as np

import qoiplane_gen as P
import qoix_cases
import qoix_gen as G
from qoiplane_gen import ADIFF, CLOSING, DIFF1, DIFF2, DIRECT, LA, REPEAT1, REPEAT2, TO_END

FOURS = [4] * 8                                                             # closing bytes 44 44 44 44: eight DIFF1 ops that add nothing


def hand_worked():
    """(name, file, expectation, channels asked for, the pixels)"""
    n = lambda s: [int(c, 16) for c in s.split()]
    return [
        ("direct_diff1_diff2_3x1", P.stored(3, 1, n("a 6 4 7 8 0")), "ok", 0, [100, 103, 87]),
        ("left_of_a_rows_first_pixel_is_the_row_aboves_last_and_the_average_rounds_up_2x2", P.stored(2, 2, n("a 0 a a 0 d 4 4")), "ok", 0, [10, 13, 12, 13]),
        ("luminance_wraps_254_plus_3_2x1", P.stored(2, 1, n("a f e 7")), "ok", 0, [254, 1]),
        ("to_the_end_run_5x3", P.stored(5, 3, n("a 0 7 f f f")), "ok", 0, [7] * 15),
        ("no_body_29_bytes_4x2_2ch", P.stored(4, 2, [], 2), "ok", 0, [0, 255] * 8),
        ("la_adiff_repeat_3x1_2ch", P.stored(3, 1, n("b 0 0 5 c 8 b a 4 d"), 2), "ok", 0, [5, 200, 5, 202, 5, 202]),
        ("of_three_adiffs_the_last_counts_2x1_2ch", P.stored(2, 1, n("b 0 0 5 c 8 b b b 7 4"), 2), "ok", 0, [5, 200, 5, 199]),
        ("alpha_ops_in_a_1_channel_file_asked_for_2", P.stored(3, 1, n("b 9 a 1 2 b 0 3 3 4 4 4")), "ok", 2, [18, 0, 51, 68, 51, 68]),
        ("closing_bytes_are_decoded_5x2", P.stored(5, 2, n("a 0 9 4"), closing=FOURS), "ok", 0, [9] * 10),
        ("deviation_p1_closing_bytes_run_out_5x4", P.stored(5, 4, n("a 0 9 4"), closing=FOURS), "refused", 0, None),
    ]


def ops():
    out = []
    for name, k in (("diff1", DIFF1(-3)), ("diff2", DIFF2(-11)), ("direct", DIRECT(99)), ("la", LA(77, 31)), ("repeat1", REPEAT1(2)), ("repeat2", REPEAT2(5))):
        body = DIRECT(10) + k + DIRECT(200) + k + DIFF1(2) + k + DIFF2(9) + k + k + k
        for ch in (1, 2):
            out.append((f"op_{name}_on_row0_at_posx0_and_inside_{ch}ch", P.stored(4, 4, body, ch), "ok"))
            out.append((f"adiff_in_front_of_{name}_{ch}ch", P.stored(4, 3, DIRECT(50) + ADIFF(-3) + k + DIRECT(1) + ADIFF(7) + k + ADIFF(-7) + ADIFF(2) + k + k, ch), "ok"))
    out += [
        ("adiff_in_front_of_a_repeat_gives_the_run_the_new_alpha", P.stored(7, 2, LA(9, 100) + ADIFF(5) + REPEAT2(6) + ADIFF(-2) + REPEAT1(3) + DIFF1(1) * 4, 2), "ok"),
        ("three_adiff_chain_then_each_colour_op", P.stored(4, 1, LA(1, 50) + ADIFF(1) + ADIFF(2) + ADIFF(3) + DIFF1(0) + ADIFF(4) + ADIFF(-4) + ADIFF(-1) + DIRECT(8) + ADIFF(1) * 3 + DIFF2(-9), 2), "ok"),
        ("adiff_then_la_the_la_wins", P.stored(2, 1, LA(1, 50) + ADIFF(5) + LA(2, 60), 2), "ok"),
        ("adiff_wraps_255_plus_3_and_0_minus_4", P.stored(3, 1, ADIFF(3) + DIRECT(9) + LA(1, 0) + ADIFF(-4) + DIFF1(0), 2), "ok"),
        ("direct_in_a_2_channel_file_sets_luminance_only", P.stored(3, 1, LA(5, 40) + DIRECT(200) + DIFF1(1), 2), "ok"),
        ("repeat_as_the_first_op_repeats_0_255", P.stored(5, 2, REPEAT1(3) + DIRECT(7) + REPEAT2(4), 2), "ok"),
        ("repeat2_of_258_then_more", P.stored(40, 9, DIRECT(3) + REPEAT2(258) + DIFF1(3) + REPEAT2(100), 1), "ok"),
        ("run_across_a_row_end_then_diff_at_posx_1", P.stored(5, 3, DIRECT(40) + DIFF1(1) + DIFF1(2) + REPEAT2(8) + DIFF1(3) + DIFF2(-12) * 3, 1), "ok"),
        ("run_past_the_image_end_is_cut", P.stored(3, 3, DIRECT(40) + REPEAT2(200) + DIRECT(1), 1), "ok"),
        ("surplus_ops_are_ignored", P.stored(2, 1, DIRECT(1) + DIRECT(2) + DIRECT(3) + ADIFF(1) + LA(1, 2)), "ok"),
        ("stream_ends_mid_image_and_repeats_the_last_pixel", P.stored(5, 3, DIRECT(1) + DIFF1(3) + ADIFF(1) + DIFF2(6), 2), "ok"),
        ("colorspace_1_version_0", P.stored(2, 2, DIRECT(9) + DIFF1(0) * 3, 1, colorspace=1, version=0), "ok"),
        ("header_par_and_dpi_bits_are_kept", P.stored(1, 1, DIRECT(1), 2, par=b"\x7f\xc0\x12\x34", dpi=b"\x80\x00\x00\x00"), "ok"),
    ]
    return out


def deviation_p1():
    return [
        ("deviation_p1_stream_of_diffs_runs_out", P.stored(9, 9, DIRECT(5) + DIFF1(1) * 30, 1, closing=[4] * 8), "refused"),
        ("deviation_p1_adiff_chain_through_the_closing_bytes", P.stored(1, 1, ADIFF(1), 2, closing=ADIFF(1) * 4), "refused"),
        ("deviation_p1_la_whose_last_nibble_is_behind_the_file", P.stored(2, 1, [], 2, closing=DIRECT(1) + LA(3, 4)[:5]), "refused"),
        ("deviation_p1_repeat2_operand_behind_the_file", P.stored(8, 1, [], 1, closing=[4] * 6 + [15, 0]), "refused"),
        ("deviation_p1_diff2_operand_behind_the_file", P.stored(8, 1, [], 1, closing=[4] * 7 + [8]), "refused"),
        ("an_op_that_ends_with_the_files_last_nibble", P.stored(6, 1, [], 1, closing=[4] * 5 + DIRECT(77)), "ok"),
        ("an_la_that_ends_with_the_files_last_nibble", P.stored(3, 1, [], 2, closing=[4] * 2 + LA(3, 4)), "ok"),
        ("deviation_p1_in_the_inflated_stream", P.compressed(9, 9, DIRECT(5) + DIFF1(1) * 30, 1, closing=[4] * 8), "refused"),
    ]


def geometry():
    out = []
    for w, h in ((1, 1), (1, 7), (2, 9), (3, 11), (7, 1), (63, 3), (64, 3), (65, 3), (129, 9)):
        for ch in (1, 2):
            out.append((f"geometry_{w}x{h}_{ch}ch", P.encode(P.noisy(w, h, ch, w * 10 + h + ch)), "ok"))
    out.append(("geometry_65x3_2ch_lz4", P.encode(P.noisy(65, 3, 2, 5), lz4=True), "ok"))
    out.append(("geometry_3x40_1ch_lz4", P.encode(P.noisy(3, 40, 1, 6), lz4=True), "ok"))
    return out


def groups():
    """what a group of 64 nibbles can do to an op: the stream starts on a group boundary"""
    out = []
    for k in range(58, 64):                                                 # a 6-nibble LA starting at nibble k of the first group
        body = DIRECT(100)[:3] + DIFF1(1) * (k - 3) + LA(7, 9) + DIFF2(-5) + DIFF1(2) * 70
        out.append((f"la_starting_at_nibble_{k}_of_a_group", P.stored(37, 4, body, 2), "ok"))
    for n in (64, 65):
        out.append((f"diff_chain_of_{n}_ops_from_a_group_start", P.stored(11, 7, DIFF1(3) * n + DIRECT(9) + DIFF2(-16) * 11, 1), "ok"))
        out.append((f"diff_chain_of_{n}_ops_on_a_row_of_2", P.stored(2, 40, DIFF1(2) * n + DIFF2(7) * 15, 1), "ok"))
    for phase in (0, 1):
        lead = DIRECT(50) + DIFF1(1) * (55 + phase)
        out.append((f"repeat2_of_258_across_row_and_group_ends_phase_{phase}", P.stored(50, 9, lead + DIFF2(3) * 3 + REPEAT2(258) + DIFF1(-1) * 70, 1), "ok"))
        out.append((f"repeat2_straddling_the_group_end_phase_{phase}", P.stored(50, 9, lead + DIFF2(3) + DIFF1(0) * (1 + phase) + REPEAT2(258) + ADIFF(3) + REPEAT2(40) + DIFF1(-1) * 70, 2), "ok"))
        out.append((f"to_the_end_run_across_row_and_group_ends_phase_{phase}", P.stored(50, 9, lead + DIFF2(3) * 3 + TO_END, 2), "ok"))
    out.append(("twenty_one_repeat2_ops_in_one_group", P.stored(301, 19, DIRECT(1) + sum((REPEAT2(258 - k) + DIFF1(1) for k in range(21)), []) + DIFF1(0) * 300, 1), "ok"))
    out.append(("a_group_of_nothing_but_adiffs", P.stored(3, 2, DIRECT(1) + ADIFF(1) * 40 + DIFF1(0) + ADIFF(-1) * 33 + DIFF1(1) * 4, 2), "ok"))
    return out


def headers():
    base = P.stored(2, 2, DIRECT(9) + DIFF1(0) * 3, 2)
    w = lambda pos, value, b=base: qoix_cases._with(pos, value, b)
    return [
        ("colorspace_2_with_2_channels_is_lap8_and_refused_by_the_sub_codec", w(15, [2]), "refused"),
        ("colorspace_2_with_1_channel_is_refused", w(13, [1, 8, 2]), "refused"),
        ("header_bad_signature", w(0, b"qoif"), "refused"),
        ("header_width_0", w(4, struct.pack(">I", 0)), "refused"),
        ("header_height_0", w(8, struct.pack(">I", 0)), "refused"),
        ("header_20000_x_20000_is_too_many_pixels", w(4, struct.pack(">II", 20000, 20000)), "refused"),
        ("header_version_2", w(12, [2]), "refused"),
        ("header_size_28", base[:28], "refused"),
        ("header_size_29_is_a_file_of_no_ops", base[:25] + b"\xff" * 4, "ok"),
        ("lz4_orig_3_leaves_no_room_for_the_closing_bytes", G.compressed(1, 1, b"", 1, pad=b"", block=b"\x30abc", orig=3), "refused"),
        ("lz4_orig_beyond_what_the_block_can_produce", G.compressed(1, 1, b"", 2, pad=b"", block=b"\x40" + G.PAD, orig=255 * 5 + 1), "refused"),
        ("ten_bit_1_channel_is_still_unsupported", w(13, [1, 10]), "refused"),
    ]


def lz4():
    """the LZ4 cases of tests/qoix_cases.py with the channel byte set to 1 or 2: their literals are bytes below 0x80, two DIFF1 ops each"""
    keep_ok = ("lz4_literal_length_", "lz4_match_length_", "lz4_offset_1_", "lz4_offset_8_", "lz4_offset_64_", "lz4_offset_65535_",
               "lz4_matches_back_to_back", "lz4_garbage_behind")
    keep_refused = ("lz4_offset_0_deviation_2", "lz4_match_from_one_byte_before_the_output_deviation_2", "lz4_truncated_inside_the_literals",
                    "lz4_truncated_inside_the_offset", "lz4_final_literal_run_overshooting_orig", "lz4_match_ending_at_oend_minus_4")
    out = []
    for k, (name, f, e) in enumerate(qoix_cases.lz4()):
        if (e == "ok" and name.startswith(keep_ok)) or (e == "refused" and name in keep_refused):
            out.append((f"{name}_{1 + k % 2}ch", f[:13] + bytes([1 + k % 2]) + f[14:], e))
    return out


@functools.lru_cache(maxsize=None)
def content():
    out = []
    for name, img in (("photo_like_201x149_l8", P.photo_like(201, 149, 1, 1)), ("flat_199x151_la8", P.flat_image(199, 151, 2, 2)),
                      ("alpha_ramp_77x31", P.alpha_ramp(77, 31, 3))):
        out.append((name + "_stored", P.encode(img), "ok", img))
        out.append((name + "_lz4", P.encode(img, lz4=True), "ok", img))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """every named case that does not depend on the kernel's geometry"""
    return [c[:3] for c in hand_worked()] + ops() + deviation_p1() + geometry() + groups() + headers() + lz4() + [c[:3] for c in content()]


@functools.lru_cache(maxsize=None)
def row_capacity(cap):
    """a row of exactly `cap` pixels (the last kept in LDS) and one of cap + 1 (the first in global scratch), height 3, 1 and 2 channels"""
    out = []
    for w, ch in ((cap, 1), (cap + 1, 2), (cap + 1, 1), (cap, 2)):
        img = P.flat_image(w, 3, ch, seed=w + ch)
        img[:, ::7] = P.noisy(w, 3, ch, w)[:, ::7]
        img[1, -3:] = (img[1, -3:].astype(int) + 9) % 256
        out.append((f"row_of_{'capacity' if w == cap else 'capacity_plus_1'}_{ch}ch", P.encode(img, lz4=ch == 2), "ok"))
    return out


def mutated(seed=0, per_file=6):
    """named cases with 1..3 bytes changed (not the width and height fields) or the tail cut"""
    rng = np.random.default_rng(seed)
    out = []
    for name, f, _ in ops() + deviation_p1() + geometry()[:10] + groups() + lz4():
        if len(f) < 26 or len(f) > 5000:
            continue
        for k in range(per_file):
            b = bytearray(f)
            for _ in range(int(rng.integers(1, 4))):
                pos = int(rng.integers(12, len(b)))
                b[pos] = int(rng.integers(0, 256)) if pos > 16 else int(rng.integers(0, 3))
            if k == 0:
                b = b[:int(rng.integers(25, len(b) + 1))]
            out.append((f"{name}_mutation_{k}", bytes(b)))
    return out
