"""The named TGA cases of the tests: the variant matrix, the run-length edge cases, the header-rule refusals and the truncations."""
import numpy as np

import tga_gen

GEOMETRIES = [(1, 1), (3, 2), (5, 3), (33, 5), (257, 7), (1100, 2)]


def variant_files(seed=0):
    """every variant at every geometry; row order, ID length, colour-map start and descriptor junk bits vary with the position"""
    out = []
    for vi, (name, typ, bpp, cmap) in enumerate(tga_gen.variants()):
        for gi, (w, h) in enumerate(GEOMETRIES):
            k = vi + gi
            out.append((f"{name}_{w}x{h}", tga_gen.make(w, h, typ, bpp, cmap, pal_start=(0, 5)[k % 2] if cmap else 0, id_len=(0, 7, 255)[k % 3],
                                                        top_down=bool(k // 2 % 2), desc_extra=(0, 0x08, 0x1F, 0xC0)[k % 4], seed=seed + k,
                                                        trailer=b"TRUEVISION-XFILE.\0" if k % 5 == 0 else b"")))
    return out


def _fit(target, s1, s2):
    """a, b >= 0 with a * s1 + b * s2 == target"""
    for b in range(target // s2 + 1):
        if (target - b * s2) % s1 == 0:
            return (target - b * s2) // s1, b
    raise ValueError((target, s1, s2))


def window_case(win, image_type=10, bpp=32, cmap=0, width=257, top_down=False, seed=0):
    """a stream over more than three of the decoder's windows of `win` bytes (counted from the first packet byte): a packet whose
    command byte is the last byte of window 0, a packet that starts in window 1 and ends in window 2, and pixels beyond.  -> (file, marks)"""
    bps = tga_gen.source_bytes(image_type, bpp, cmap)
    s_run, s_raw2 = 1 + bps, 1 + 2 * bps
    a, b = _fit(win - 1, s_run, s_raw2)
    pkts = [(True, 3)] * a + [(False, 2)] * b                              # window 0 up to its last byte
    pos = win - 1
    pkts.append((False, 128)); cmd_last = pos; pos += 1 + 128 * bps        # command byte at win - 1, pixels in window 1
    while pos + 1 + 3 * bps < 2 * win - 2:
        pkts.append((False, 3)); pos += 1 + 3 * bps
    straddle = pos
    pkts.append((False, 128)); pos += 1 + 128 * bps                        # starts inside window 1, ends inside window 2
    assert straddle < 2 * win - 1 and pos > 2 * win
    while pos < 3 * win + 64:
        pkts.append((True, 128)); pos += s_run
        pkts.append((False, 5)); pos += 1 + 5 * bps
    npix = sum(c for _, c in pkts)
    h = npix // width                                                      # the last packets overrun width * height
    assert h >= 2
    f = tga_gen.make(width, h, image_type, bpp, cmap, top_down=top_down, seed=seed, pkts=pkts, id_len=3)
    return f, dict(cmd_last=cmd_last, straddle=straddle, stream_bytes=pos, windows=pos // win + 1)


def rle_edge_cases(win):
    """(name, file) -- each must decode; the names say what they are about"""
    g = tga_gen.make
    out = [("run_and_raw_cross_row_end", g(5, 4, 10, 24, seed=1, pkts=[(True, 7), (False, 6), (True, 4), (False, 3)])),
           ("packets_of_128", g(130, 9, 10, 32, policy="max", seed=2)),
           ("packets_of_128_bottom_up_l8", g(257, 3, 11, 8, policy="max", seed=3)),
           ("one_pixel_packets", g(33, 5, 10, 24, policy="one", seed=4)),
           ("one_pixel_packets_l8_two_byte_packets", g(1100, 5, 11, 8, policy="one", seed=5)),
           ("last_packet_overruns", g(7, 3, 10, 32, seed=6, pkts=[(False, 20), (True, 128)])),
           ("last_raw_packet_overruns_and_is_cut_by_the_file_end", g(7, 3, 10, 32, seed=7, pkts=[(True, 20), (False, 128)])[:18 + 5 + 1 + 4 * 1]),
           ("index_past_the_palette_8", g(33, 5, 9, 8, 24, pal_len=100, bad_index=True, seed=8)),
           ("index_past_the_palette_16", g(33, 5, 9, 16, 32, pal_len=300, bad_index=True, pal_start=3, seed=9)),
           ("index_past_the_palette_unpacked", g(33, 5, 1, 8, 15, pal_len=17, bad_index=True, seed=10)),
           ("rgb16_runs", g(257, 7, 10, 16, policy="run", seed=11)),
           ("la8_raw", g(65, 3, 11, 16, policy="raw", seed=12))]
    for k, (typ, bpp, cmap, td) in enumerate([(10, 32, 0, False), (10, 24, 0, True), (9, 8, 24, False), (11, 8, 0, False), (10, 15, 0, True)]):
        out.append((f"three_windows_t{typ}_b{bpp}", window_case(win, typ, bpp, cmap, top_down=td, seed=20 + k)[0]))
    return out


def header_refusals():
    """(name, file, detected) -- one header rule broken at a time on a good 3x2 file; `detected` is what detectTGA must say"""
    good = tga_gen.make(3, 2, 2, 24, seed=1)
    idx = tga_gen.make(3, 2, 1, 8, 24, pal_len=4, seed=2)

    def put(f, pos, *vals):
        return f[:pos] + bytes(vals) + f[pos + len(vals):]
    return [("cmap_type_2", put(good, 1, 2), False), ("cmap_with_type_2", put(idx, 2, 2), False), ("cmap_with_type_10", put(idx, 2, 10), False),
            ("empty_palette", put(idx, 5, 0, 0), False), ("cmap_size_12", put(idx, 7, 12), False), ("type_0", put(good, 2, 0), False),
            ("type_1_without_cmap", put(good, 2, 1), False), ("type_9_without_cmap", put(good, 2, 9), False), ("type_4", put(good, 2, 4), False),
            ("width_0", put(good, 12, 0, 0), False), ("height_0", put(good, 14, 0, 0), False), ("index_of_24_bits", put(idx, 16, 24), False),
            ("bpp_12", put(good, 16, 12), False), ("bpp_0", put(good, 16, 0), False),
            ("id_field_past_the_end", put(good, 0, 200), True), ("too_large", tga_gen.header(40000, 40000, 2, 32), True),
            ("len_0", b"", False), ("len_16", good[:16], False), ("len_17", good[:17], True)]


def truncations(win):
    """(name, file) -- every one must be refused as a whole: the stream ends at a command byte, inside pixel data, inside the palette"""
    g = tga_gen.make
    out = []
    f = g(9, 4, 10, 32, seed=1, pkts=[(False, 10), (True, 10), (False, 16)])
    out += [("rle_cut_at_command_byte", f[:18 + 41]), ("rle_cut_inside_run_pixel", f[:18 + 41 + 3]), ("rle_cut_inside_raw_pixels", f[:len(f) - 5]),
            ("rle_cut_after_header", f[:18]), ("rle_one_byte_short", f[:-1])]
    f = g(9, 4, 9, 8, 24, pal_len=16, id_len=2, seed=2)
    out += [("palette_cut", f[:18 + 2 + 40]), ("palette_cut_at_its_last_byte", f[:18 + 2 + 47]), ("rle_indexed_no_pixels", f[:18 + 2 + 48])]
    f = g(9, 4, 1, 16, 15, pal_len=16, pal_start=600, seed=3)
    out += [("palette_start_past_the_end", f[:300]), ("unpacked_indexed_one_byte_short", f[:-1])]
    out += [("unpacked_24_one_byte_short", g(33, 5, 2, 24, seed=4)[:-1]), ("unpacked_rgb16_half", g(33, 5, 2, 16, seed=5)[:18 + 165]),
            ("unpacked_header_only", g(33, 5, 3, 8, seed=6)[:18])]
    wf, marks = window_case(win, seed=7)
    off = 18 + 3
    out += [("windows_cut_at_the_command_byte_that_ends_window_0", wf[:off + marks["cmd_last"]]),
            ("windows_cut_inside_the_straddling_packet", wf[:off + marks["straddle"] + 200]),
            ("windows_cut_in_the_last_window", wf[:off + 3 * win + 10])]
    return out
