"""Named QOIX test files: (name, file bytes, expectation) with expectation "ok", "refused" or "unsupported".  The name says what a case is
about.  Cases that depend on the kernel's geometry take it as an argument (gamut_hip_qoix_row_capacity()) and use no literal."""
import functools
import struct

import numpy as np

import qoix_gen as G
from qoix_gen import ADIFF, END, GRAY, INDEX, LUMA, LUMA2, LUMA3, PAD, RGB, RGBA, RUN, RUN2

KINDS = {"luma": LUMA(-2, 1, 3), "index": INDEX(1), "luma2": LUMA2(-9, 3, 12), "luma3": LUMA3(40, 5, 60), "gray": GRAY(99), "rgb": RGB(7, 8, 9),
         "rgba": RGBA(1, 2, 3, 4), "run": RUN(3), "run2": RUN2(6)}


def ops():
    out = []
    for name, k in KINDS.items():                                           # 4 x 4 rgba: index 1 is on row 0, index 4 at posx 0 of row 1, index 6 in the interior
        body = RGB(10, 20, 30) + k + GRAY(77) + RGB(200, 100, 50) + k + RGB(90, 80, 70) + k + GRAY(5) + LUMA(1, 2, 0) + k + LUMA2(3, 9, 1) + k + k
        out.append((f"op_{name}_on_row0_at_posx0_and_inside", G.stored(4, 4, body, 4), "ok"))
        out.append((f"adiff_in_front_of_{name}", G.stored(4, 3, GRAY(50) + ADIFF(-3) + k + RGB(1, 1, 1) + ADIFF(2) + k + GRAY(3) + ADIFF(1) + k + k, 4), "ok"))
    # LOCO-I: a = left (row 1, x 0), b = up (row 0, x 1), c = up-left (row 0, x 0); LUMA(0, 2, 2) adds nothing to the prediction
    triples = [(10, 20, 30), (30, 20, 10), (10, 30, 20), (20, 20, 20), (20, 20, 5), (20, 20, 40), (15, 30, 15), (30, 15, 30), (15, 30, 30), (0, 255, 128), (255, 0, 0)]
    for i in range(len(triples)):
        (ar, br, cr), (ag, bg, cg), (ab, bb, cb) = triples[i], triples[(i + 3) % len(triples)], triples[(i + 7) % len(triples)]
        body = RGB(cr, cg, cb) + RGB(br, bg, bb) + RGB(1, 2, 3) + RGB(ar, ag, ab) + LUMA(0, 2, 2) + LUMA(0, 2, 2)
        out.append((f"loco_branches_{triples[i]}_per_channel_rotated".replace(" ", ""), G.stored(3, 2, body, 3), "ok"))
    out += [
        ("luma_bias_1_for_a_negative_green_delta_and_2_otherwise", G.stored(4, 1, RGB(100, 100, 100) + LUMA(-1, 0, 3) + LUMA(0, 0, 3) + LUMA(3, 3, 0), 3), "ok"),
        ("bytes_wrap_250_plus_10_and_2_minus_16", G.stored(4, 2, RGB(250, 250, 250) + LUMA2(10, 15, 15) + RGB(2, 2, 2) + LUMA2(-16, 0, 0) + LUMA(3, 3, 3) * 4, 3), "ok"),
        ("luma3_extremes", G.stored(3, 2, RGB(128, 128, 128) + LUMA3(-64, 0, 0) + LUMA3(63, 63, 63) + LUMA3(-64, 63, 0) + LUMA3(63, 0, 63) + LUMA3(0, 32, 32), 4), "ok"),
        ("adiff_single", G.stored(2, 1, ADIFF(-3) + LUMA(0, 2, 2) + GRAY(1), 4), "ok"),
        ("adiff_chained_five_times", G.stored(2, 1, ADIFF(-4) * 5 + GRAY(9) + ADIFF(3) + ADIFF(3) + GRAY(1), 4), "ok"),
        ("adiff_wraps_255_plus_3_and_0_minus_4", G.stored(3, 1, ADIFF(3) + GRAY(9) + RGBA(1, 1, 1, 0) + ADIFF(-4) + GRAY(2), 4), "ok"),
        ("index_replaces_the_alpha_an_adiff_just_set", G.stored(3, 1, RGBA(5, 6, 7, 200) + ADIFF(3) + INDEX(0) + ADIFF(-1) + INDEX(9), 4), "ok"),
        ("run_repeats_the_alpha_an_adiff_just_set", G.stored(5, 1, GRAY(4) + ADIFF(-2) + RUN(4), 4), "ok"),
        ("fifo_slot_never_written_is_0_0_0_0", G.stored(2, 1, INDEX(5) + INDEX(63), 4), "ok"),
        ("fifo_wraps_at_64_writes", G.stored(23, 3, b"".join(GRAY(v) for v in range(1, 66)) + INDEX(0) + INDEX(1) + INDEX(63) + INDEX(2), 4), "ok"),
        ("index_does_not_write_the_fifo", G.stored(6, 1, GRAY(9) + INDEX(0) + INDEX(0) + GRAY(8) + INDEX(1) + INDEX(2), 4), "ok"),
        ("rgba_and_adiff_ops_in_a_3_channel_file", G.stored(4, 2, RGBA(1, 2, 3, 4) + ADIFF(2) + LUMA(1, 1, 1) + INDEX(0) + ADIFF(-4) + RUN(2) + GRAY(8) + ADIFF(1) + LUMA2(0, 8, 8), 3), "ok"),
        ("colorspace_2_with_4_channels_is_rgbap8", G.stored(2, 2, RGBA(9, 8, 7, 6) + LUMA(0, 2, 2) * 3, 4, colorspace=2), "ok"),
        ("colorspace_1_version_0", G.stored(2, 2, RGB(9, 8, 7) + LUMA(0, 2, 2) * 3, 3, colorspace=1, version=0), "ok"),
    ]
    return out


def runs():
    return [
        ("run_of_1_as_the_first_op", G.stored(3, 1, RUN(1) + GRAY(2) + GRAY(3), 3), "ok"),
        ("run_of_8", G.stored(10, 1, GRAY(2) + RUN(8) + GRAY(3), 4), "ok"),
        ("run2_of_9", G.stored(11, 1, GRAY(2) + RUN2(9) + GRAY(3), 3), "ok"),
        ("run2_of_1024_then_more", G.stored(130, 9, GRAY(3) + RUN2(1024) + GRAY(9) + RUN2(144), 3), "ok"),
        ("run2_as_the_first_op_of_the_file", G.stored(7, 3, RUN2(10) + RGB(1, 2, 3) + RUN(8), 4), "ok"),
        ("run_across_a_row_end_then_luma_at_posx_1", G.stored(5, 3, RGB(40, 50, 60) + GRAY(1) + GRAY(2) + RUN(8) + LUMA(1, 2, 2) + LUMA(-1, 1, 1) * 3, 3), "ok"),
        ("run_ending_exactly_at_the_image_end", G.stored(3, 3, RGB(40, 50, 60) + RUN(8), 4), "ok"),
        ("run_past_the_image_end_is_cut", G.stored(3, 3, RGB(40, 50, 60) + RUN2(1024) + GRAY(1), 3), "ok"),
        ("runs_over_several_rows_with_predictions_between", G.stored(64, 4, GRAY(100) + RUN2(70) + LUMA(1, 2, 2) * 9 + RUN2(100) + LUMA2(4, 8, 8) * 20, 4), "ok"),
    ]


def stream_length():
    return [
        ("no_ops_at_all_size_29", G.stored(3, 2, b"", 3), "ok"),
        ("no_ops_at_all_size_29_rgba", G.stored(3, 2, b"", 4), "ok"),
        ("stream_ends_mid_image", G.stored(5, 3, RGB(1, 2, 3) + GRAY(4) + LUMA(1, 1, 1) + ADIFF(1) + GRAY(6), 4), "ok"),
        ("surplus_ops_are_ignored", G.stored(2, 1, GRAY(1) + GRAY(2) + GRAY(3) + END + RGB(1, 2, 3) + ADIFF(1), 3), "ok"),
        ("rgba_op_whose_operands_are_the_last_four_bytes", G.stored(2, 1, GRAY(1) + b"\xfe", 4, pad=bytes([9, 8, 7, 6])), "ok"),
        ("luma3_op_whose_operands_lie_in_the_last_four_bytes", G.stored(2, 1, GRAY(1) + LUMA3(1, 2, 3)[:1], 3, pad=LUMA3(1, 2, 3)[1:] + b"\0\0"), "ok"),
        ("adiff_chain_into_the_last_four_bytes_then_a_whole_op", G.stored(1, 1, ADIFF(0), 4, pad=ADIFF(1) + GRAY(5) + b"\0"), "ok"),
        ("deviation_3_end_executed", G.stored(1, 1, END, 3), "refused"),
        ("deviation_3_end_executed_mid_image_rgba", G.stored(3, 3, GRAY(1) * 4 + END + GRAY(2) * 4, 4), "refused"),
        ("deviation_3_end_through_an_adiff_chain", G.stored(1, 1, ADIFF(0) + END, 4), "refused"),
        ("deviation_3_end_in_the_last_four_bytes_through_adiff", G.stored(1, 1, ADIFF(0), 4), "refused"),
        ("deviation_4_adiff_chain_through_the_last_four_bytes", G.stored(1, 1, ADIFF(0), 4, pad=ADIFF(0) * 4), "refused"),
        ("deviation_4_operand_behind_the_file", G.stored(1, 1, ADIFF(0), 3, pad=ADIFF(0) * 3 + b"\xfc"), "refused"),
        ("deviation_4_rgba_operands_behind_the_file", G.stored(2, 2, GRAY(3) + ADIFF(0), 4, pad=ADIFF(0) * 2 + b"\xfe\x01"), "refused"),
    ]


def _noisy(w, h, ch, seed):
    """photo-like with flat stretches: every op kind and runs"""
    img = G.photo_like(w, h, ch, seed)
    rng = np.random.default_rng(seed + 1000)
    for _ in range(3):
        x0 = int(rng.integers(0, w))
        img[int(rng.integers(0, h)), x0:x0 + int(rng.integers(1, w + 1))] = rng.integers(0, 256, ch)
    img[rng.integers(0, h, 4), rng.integers(0, w, 4)] = rng.integers(0, 256, (4, ch))
    return img


def geometry():
    out = []
    for w, h in ((1, 1), (1, 7), (7, 1), (63, 3), (64, 3), (65, 3), (129, 9)):
        for ch in (3, 4):
            out.append((f"geometry_{w}x{h}_{ch}ch", G.encode(_noisy(w, h, ch, w * 10 + h + ch)), "ok"))
    out.append(("geometry_65x3_4ch_lz4", G.encode(_noisy(65, 3, 4, 5), lz4=True), "ok"))
    return out


@functools.lru_cache(maxsize=None)
def row_capacity(cap):
    """a row of exactly `cap` pixels (the last one kept in LDS) and one of cap + 1 (the first in global scratch), height 3, 3 and 4 channels"""
    out = []
    for w, ch in ((cap, 3), (cap + 1, 4), (cap + 1, 3), (cap, 4)):
        img = G.flat_image(w, 3, ch, seed=w + ch)
        img[:, ::7] = _noisy(w, 3, ch, w)[:, ::7]
        img[1, -3:] = (img[1, -3:].astype(int) + 9) % 256                    # something to predict from at the row's end
        out.append((f"row_of_{'capacity' if w == cap else 'capacity_plus_1'}_{ch}ch", G.encode(img, lz4=ch == 4), "ok"))
    return out


BASE = G.stored(2, 2, RGB(9, 8, 7) + LUMA(0, 2, 2) * 3, 3)


def _with(pos, value, base=BASE):
    return base[:pos] + bytes(value) + base[pos + len(bytes(value)):]


def headers():
    out = [
        ("header_bad_signature", _with(0, b"qoif"), "refused"),
        ("header_width_0", _with(4, struct.pack(">I", 0)), "refused"),
        ("header_height_0", _with(8, struct.pack(">I", 0)), "refused"),
        ("header_width_above_int_max", _with(4, struct.pack(">I", 0x80000001)), "refused"),
        ("header_20000_x_20000_is_too_many_pixels", _with(4, struct.pack(">II", 20000, 20000)), "refused"),
        ("header_channels_0", _with(13, [0]), "refused"),
        ("header_channels_5", _with(13, [5]), "refused"),
        ("header_bitdepth_9", _with(14, [9]), "refused"),
        ("header_bitdepth_16", _with(14, [16]), "refused"),
        ("header_colorspace_3", _with(15, [3]), "refused"),
        ("header_version_2", _with(12, [2]), "refused"),
        ("header_compression_2", _with(16, [2]), "refused"),
        ("header_compression_255", _with(16, [255]), "refused"),
        ("header_size_24", BASE[:24], "refused"),
        ("header_size_25", BASE[:25], "refused"),
        ("header_size_28", BASE[:28], "refused"),
        ("header_size_29_is_a_file_of_no_ops", BASE[:29], "ok"),
        ("header_size_0", b"", "refused"),
        ("header_size_3", b"qoi", "refused"),
        ("header_lz4_size_28", _with(16, [1])[:28], "refused"),
        ("lz4_size_29_with_nothing_behind_orig", _with(16, [1])[:25] + struct.pack(">I", 4), "refused"),
        ("header_par_and_dpi_bits_are_kept", G.stored(1, 1, GRAY(1), 3, par=b"\x7f\xc0\x12\x34", dpi=b"\x80\x00\x00\x00"), "ok"),
    ]
    for depth, ch in ((10, 1), (10, 2), (10, 3), (10, 4), (8, 1), (8, 2)):
        out.append((f"unsupported_{depth}bit_{ch}ch", _with(13, [ch, depth]), "unsupported"))
    out.append(("unsupported_8bit_2ch_premultiplied_lz4", G.header(2, 2, 2, colorspace=2, compression=1) + struct.pack(">I", 10) + b"\0" * 8, "unsupported"))
    out.append(("unsupported_codec_with_zero_width_is_still_unsupported", _with(4, struct.pack(">I", 0), _with(13, [1])), "unsupported"))
    return out


def _lits(n, seed):
    """n literal bytes below 0x80: one-byte LUMA ops, so the op stream is valid whatever the LZ4 layer does with them"""
    return bytes(np.random.default_rng(seed).integers(0, 0x80, n, dtype=np.uint8))


def lz_file(seqs, last, orig=None, trail=b"", cut=None, ch=3):
    """an LZ4 file whose block is exactly these sequences; the image is 16 pixels wide and tall enough for every op byte"""
    n = sum(len(l) + m for l, _, m in seqs) + len(last)
    f = G.compressed(16, max(1, (n + 15) // 16), b"", ch, pad=b"", block=G.lz4_block(seqs, last) + trail, orig=n if orig is None else orig)
    return f if cut is None else f[:cut]


def lz4():
    out = []
    for n in (0, 14, 15, 15 + 255, 15 + 255 + 1, 15 + 255 + 255):           # literal lengths: nibble only, 15 + 0, 15 + 255 + 0, 15 + 255 + 1
        out.append((f"lz4_literal_length_{n}", lz_file([(_lits(20, 1), 4, 8), (_lits(n, 2), 8, 4)], _lits(12, 3)), "ok"))
    for m in (4, 18, 19, 19 + 255, 19 + 255 + 1):
        out.append((f"lz4_match_length_{m}", lz_file([(_lits(20, 4), 7, m)], _lits(12, 5)), "ok"))
    for off in (1, 2, 3, 7, 8, 63, 64, 65, 200, 65535):
        out.append((f"lz4_offset_{off}_match_150", lz_file([(_lits(off + 5, off), off, 150), (_lits(3, 6), off, 70)], _lits(13, 7), ch=4), "ok"))
    two = [(_lits(70, 8), 64, 64), (b"", 128, 129), (b"", 70, 5)]
    out += [
        ("lz4_match_from_the_very_first_output_byte", lz_file([(_lits(9, 9), 9, 30)], _lits(12, 10)), "ok"),
        ("lz4_match_from_one_byte_before_the_output_deviation_2", lz_file([(_lits(9, 9), 10, 30)], _lits(12, 10)), "refused"),
        ("lz4_match_with_no_literals_in_front_at_output_0_deviation_2", lz_file([(b"", 1, 30)], _lits(12, 10)), "refused"),
        ("lz4_offset_0_deviation_2", lz_file([(_lits(9, 9), 0, 30)], _lits(12, 10)), "refused"),
        ("lz4_matches_back_to_back_reading_what_the_last_step_wrote", lz_file(two, _lits(12, 11)), "ok"),
        ("lz4_final_literals_only", lz_file([], _lits(40, 12)), "ok"),
        ("lz4_final_literal_run_ending_inside_the_last_8_bytes", lz_file([(_lits(20, 13), 4, 8)], _lits(12, 14), orig=20 + 8 + 12 + 3), "refused"),
        ("lz4_final_literal_run_overshooting_orig", lz_file([(_lits(20, 13), 4, 8)], _lits(12, 14), orig=20 + 8 + 12 - 1), "refused"),
        ("lz4_match_ending_at_oend_minus_12", lz_file([(_lits(20, 15), 4, 8)], _lits(12, 16)), "ok"),
        ("lz4_match_ending_at_oend_minus_5", lz_file([(_lits(20, 15), 4, 8)], _lits(5, 16)), "ok"),
        ("lz4_match_ending_at_oend_minus_4", lz_file([(_lits(20, 15), 4, 8)], _lits(4, 16)), "refused"),
        ("lz4_match_running_past_orig", lz_file([(_lits(20, 15), 4, 80)], _lits(5, 16), orig=60), "refused"),
        ("lz4_garbage_behind_the_final_sequence_is_ignored", lz_file([(_lits(20, 17), 3, 9)], _lits(12, 18), trail=b"\xff\x00garbage\xff\xff"), "ok"),
        ("lz4_orig_0", G.compressed(1, 1, b"", 3, pad=b"", block=b"\x00", orig=0), "refused"),
        ("lz4_orig_3", G.compressed(1, 1, b"", 3, pad=b"", block=b"\x30abc", orig=3), "refused"),
        ("lz4_orig_4_is_a_file_of_no_ops", G.compressed(2, 2, b"", 4, pad=b"", block=b"\x40" + PAD, orig=4), "ok"),
        ("lz4_orig_0x80000000", G.compressed(1, 1, b"", 3, pad=b"", block=b"\x40" + PAD, orig=0x80000000), "refused"),
        ("lz4_orig_beyond_what_the_block_can_produce", G.compressed(1, 1, b"", 3, pad=b"", block=b"\x40" + PAD, orig=255 * 5 + 1), "refused"),
        ("lz4_orig_at_the_most_the_block_could_produce", G.compressed(1, 1, b"", 3, pad=b"", block=b"\x40" + PAD, orig=255 * 5), "refused"),
        ("lz4_compression_byte_2", _with(16, [2], lz_file([], _lits(40, 12))), "refused"),
        ("lz4_end_executed_in_the_inflated_stream_deviation_3", G.compressed(2, 2, GRAY(1) + END + GRAY(2), 3), "refused"),
    ]
    long_lit = lz_file([(_lits(15 + 255 + 7, 19), 9, 19 + 255 + 3)], _lits(12, 20))
    # 29 header bytes, token, 2 extension bytes, 277 literals, 2 offset bytes, 2 extension bytes
    out += [
        ("lz4_truncated_behind_the_token", long_lit[:30], "refused"),
        ("lz4_truncated_inside_the_literal_length_extension", long_lit[:31], "refused"),
        ("lz4_truncated_inside_the_literals", long_lit[:32 + 100], "refused"),
        ("lz4_truncated_inside_the_offset", long_lit[:32 + 277 + 1], "refused"),
        ("lz4_truncated_inside_the_match_length_extension", long_lit[:32 + 277 + 2 + 1], "refused"),
        ("lz4_truncated_inside_the_final_literals", long_lit[:-3], "refused"),
        ("lz4_not_truncated", long_lit, "ok"),
    ]
    return out


@functools.lru_cache(maxsize=None)
def content():
    """one photo-like and one flat image of about 200 x 150, stored both ways"""
    out = []
    for name, img in (("photo_like_201x149_rgb", G.photo_like(201, 149, 3, 1)), ("flat_199x151_rgba", G.flat_image(199, 151, 4, 2))):
        out.append((name + "_stored", G.encode(img), "ok", img))
        out.append((name + "_lz4", G.encode(img, lz4=True), "ok", img))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """every named case that does not depend on the kernel's geometry, the content images included"""
    return ops() + runs() + stream_length() + geometry() + headers() + lz4() + [c[:3] for c in content()]


def mutated(seed=0, per_file=6):
    """named cases with 1..3 bytes changed (not the width and height fields: a damaged size only makes a case slow) or the tail cut"""
    rng = np.random.default_rng(seed)
    out = []
    for name, f, _ in ops() + runs() + stream_length() + geometry()[:6] + lz4():
        if len(f) < 26 or len(f) > 5000:
            continue
        for k in range(per_file):
            b = bytearray(f)
            for _ in range(int(rng.integers(1, 4))):
                pos = int(rng.integers(12, len(b)))
                b[pos] = int(rng.integers(0, 256)) if pos > 16 else int(rng.integers(0, 5))
            if k == 0:
                b = b[:int(rng.integers(25, len(b) + 1))]
            out.append((f"{name}_mutation_{k}", bytes(b)))
    return out
