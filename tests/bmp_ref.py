"""A numpy reading of the reference's BMP loader (stbi__bmp_parse_header + stbi__bmp_load, codecs/stbdec.d:2147-2465), written
independently of tests/c/bmp_ref.c: that one walks a cursor as the reference does, this one works from positions in the file and on
whole arrays.  Same conventions: bytes past the end read as 0; a negative palette size, a zero width or height are refused; palette
entries past the palette size are (0, 0, 0).  decode(data, req_comp) -> None | (pixels (h, w, comps), info dict, (ppmx, ppmy, ratio))."""
import numpy as np

MUL = [0, 0xff, 0x55, 0x49, 0x11, 0x21, 0x41, 0x81, 0x01]                    # :2495-2502
DOWN = [0, 0, 0, 1, 0, 2, 4, 6, 0]


def _s32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def parse(data, req_comp=0):
    b = bytes(data)

    def u8(p):
        return b[p] if p < len(b) else 0

    def u16(p):
        return u8(p) | u8(p + 1) << 8

    def u32(p):
        return u16(p) | u16(p + 2) << 16

    if u8(0) != 0x42 or u8(1) != 0x4d:
        return None
    offset, hsz = _s32(u32(10)), _s32(u32(14))
    if offset < 0 or hsz not in (12, 40, 56, 108, 124):                       # :2163-2165
        return None
    ppmx = ppmy = ratio = -1.0
    mr = mg = mb = ma = 0
    comp = 0
    hdr_end = 14 + hsz
    if hsz == 12:
        w, hraw, planes, bpp = u16(18), u16(20), u16(22), u16(24)
    else:
        w, hraw, planes, bpp, comp = u32(18), _s32(u32(22)), u16(26), u16(28), _s32(u32(30))
    if planes != 1:
        return None
    cand = False
    if hsz != 12:
        if comp in (1, 2) or comp >= 4 or (comp == 3 and bpp not in (16, 32)):    # :2177-2179
            return None
        x, y = _s32(u32(38)), _s32(u32(42))
        if x > 1:
            ppmx = float(x)
        if y > 1:
            ppmy = float(y)
        if ppmx != -1 and ppmy != -1:
            ratio = float(np.float32(ppmx) / np.float32(ppmy))
        defaults = {16: (31 << 10, 31 << 5, 31, 0), 32: (0xff0000, 0xff00, 0xff, 0xff000000)}
        if hsz in (40, 56):
            if bpp in (16, 32):
                if comp == 0:
                    mr, mg, mb, ma = defaults[bpp]
                    cand = bpp == 32
                elif comp == 3:
                    mr, mg, mb = u32(hdr_end), u32(hdr_end + 4), u32(hdr_end + 8)
                    hdr_end += 12
                    if mr == mg == mb:
                        return None
                else:
                    return None
        else:
            mr, mg, mb, ma = u32(54), u32(58), u32(62), u32(66)
            if comp == 0:
                if bpp == 16:
                    mr, mg, mb = defaults[16][:3]                             # set_mask_defaults leaves the file's alpha mask alone at 16 bits (:2128-2131)
                else:
                    mr, mg, mb, ma = defaults.get(bpp, (0, 0, 0, 0))
                cand = bpp == 32
    top_down = hraw <= 0
    h = abs(hraw)
    if w > 1 << 24 or h > 1 << 24 or w == 0 or h == 0:
        return None
    psize = 0
    if hsz == 12:
        if bpp < 24:
            psize = int((offset - 14 - 24) / 3)                               # C division truncates towards zero
    elif bpp < 16:
        psize = (offset - hdr_end) >> 2
    if psize < 0:
        return None
    pix = offset
    if psize == 0:
        if not (hdr_end <= offset <= hdr_end + 1024):                         # :2307
            return None
        if bpp >= 16:
            pix = offset + (offset - hdr_end)                                 # the second skip :2389
    img_n = 3 if (bpp == 24 and ma == 0xff000000) else (4 if ma else 3)
    target = req_comp if req_comp >= 3 else img_n
    if target * w * h > 0x7fffffff:
        return None
    if bpp < 16:
        if psize == 0 or psize > 256 or bpp not in (1, 4, 8):
            return None
    else:
        easy = bpp == 24 or (bpp == 32 and (mr, mg, mb, ma) == (0xff0000, 0xff00, 0xff, 0xff000000))
        if not easy:
            if not mr or not mg or not mb:
                return None
            if max(bin(m).count("1") for m in (mr, mg, mb, ma)) > 8:
                return None
    info = dict(width=w, height=h, bpp=bpp, header_size=hsz, compression=comp & 0xffffffff, channels_in_file=img_n, top_down=int(top_down),
                pixel_offset=pix, palette_size=psize, mask_r=mr, mask_g=mg, mask_b=mb, mask_a=ma)
    return info, (ppmx, ppmy, ratio), dict(hdr_end=hdr_end, cand=cand, target=target)


def _channel(v, mask):
    if mask == 0:
        return None
    bits = bin(mask).count("1")
    shift = mask.bit_length() - 1 - 7
    x = v & np.uint64(mask)
    x = (x << np.uint64(-shift)) if shift < 0 else (x >> np.uint64(shift))
    x = x >> np.uint64(8 - bits)
    return ((x * np.uint64(MUL[bits])) >> np.uint64(DOWN[bits])) & np.uint64(255)


def decode(data, req_comp=0):
    p = parse(data, req_comp)
    if p is None:
        return None
    info, dens, x = p
    w, h, bpp, pix = info["width"], info["height"], info["bpp"], info["pixel_offset"]
    rbpp = bpp if bpp < 16 else (16 if bpp == 16 else 24 if bpp == 24 else 32)
    stride = ((w * rbpp + 7) // 8 + 3) & ~3
    need = pix + stride * h
    buf = np.zeros(need, np.uint8)
    src = np.frombuffer(bytes(data[:need]), np.uint8)
    buf[:src.size] = src
    rows = buf[pix:].reshape(h, stride)
    rgba = np.empty((h, w, 4), np.uint8)
    if bpp < 16:
        esz = 3 if info["header_size"] == 12 else 4
        pal = np.zeros((256, 4), np.uint8); pal[:, 3] = 255
        e = buf[x["hdr_end"]:x["hdr_end"] + info["palette_size"] * esz].reshape(-1, esz)
        pal[:len(e), 0] = e[:, 2]; pal[:len(e), 1] = e[:, 1]; pal[:len(e), 2] = e[:, 0]
        if bpp == 8:
            idx = rows[:, :w]
        elif bpp == 4:
            idx = np.stack([rows >> 4, rows & 15], axis=2).reshape(h, -1)[:, :w]
        else:
            idx = np.unpackbits(rows, axis=1)[:, :w]
        rgba = pal[idx]
    elif bpp == 24:
        t = rows[:, :3 * w].reshape(h, w, 3)
        rgba[..., 0] = t[..., 2]; rgba[..., 1] = t[..., 1]; rgba[..., 2] = t[..., 0]; rgba[..., 3] = 255
    else:
        n = 2 if bpp == 16 else 4
        t = rows[:, :n * w].reshape(h, w, n).astype(np.uint64)
        v = t[..., 0] | t[..., 1] << np.uint64(8)
        if n == 4:
            v |= t[..., 2] << np.uint64(16) | t[..., 3] << np.uint64(24)
        for c, m in enumerate((info["mask_r"], info["mask_g"], info["mask_b"], info["mask_a"])):
            ch = _channel(v, m)
            rgba[..., c] = 255 if ch is None else ch.astype(np.uint8)
    target = x["target"]
    if x["cand"] and target == 4 and not rgba[..., 3].any():                  # the all_a rule :2439-2443
        rgba[..., 3] = 255
    if not info["top_down"]:
        rgba = rgba[::-1]
    comps = req_comp or info["channels_in_file"]
    if comps >= 3:
        out = rgba[..., :comps]
    else:
        r, g, b = (rgba[..., k].astype(np.uint32) for k in range(3))
        y = ((r * 77 + g * 150 + b * 29) >> 8).astype(np.uint8)               # stbi__compute_y
        out = y[..., None] if comps == 1 else np.stack([y, rgba[..., 3] if target == 4 else np.full_like(y, 255)], axis=2)
    return np.ascontiguousarray(out), info, dens
