"""TGADecoder (codecs/tga.d:313-647) read a second time, independently of tests/c/tga_ref.c: numpy on file positions instead of a cursor
walk -- the header by slices, the colour map and the pixels as arrays, the run-length chain packet by packet with whole-packet copies.
parse() gives the two verdicts and the header fields, decode() the pixels (req_comp 3 / 4: convertTo(rgb8 / rgba8))."""
import numpy as np

CMAP_SIZES = BPPS = (8, 15, 16, 24, 32)


def _comp(bits, grey):
    """stbi__tga_get_comp -> (components, rgb16)"""
    if bits == 8:
        return 1, False
    if bits == 16 and grey:
        return 2, False
    if bits in (15, 16):
        return 3, True
    return bits // 8, False


def parse(data):
    """-> (detected, loadable, info dict: the fields known at the point where the header stopped)"""
    d = bytes(data)
    info = {}
    if len(d) < 3 or d[1] > 1:
        return False, False, info
    cmap_type, typ = d[1], d[2]
    if cmap_type == 1:
        if typ not in (1, 9) or len(d) < 8:
            return False, False, info
        pal_start, pal_len, cmap_size = d[3] | d[4] << 8, d[5] | d[6] << 8, d[7]
        if pal_len == 0 or cmap_size not in CMAP_SIZES:
            return False, False, info
    else:
        if typ not in (2, 3, 10, 11):
            return False, False, info
        pal_start = pal_len = cmap_size = 0
    if len(d) < 17:                                                        # bytes 8..11 are skipped, 12..16 read
        return False, False, info
    w, h, bpp = d[12] | d[13] << 8, d[14] | d[15] << 8, d[16]
    if w < 1 or h < 1 or (cmap_type == 1 and bpp not in (8, 16)) or bpp not in BPPS:
        return False, False, info
    info = dict(width=w, height=h, bpp=bpp, indexed=cmap_type, palette_start=pal_start, palette_len=pal_len, cmap_size=cmap_size, detected=1,
                rle=int(typ >= 8), image_type=typ & 7)
    if len(d) < 18:
        return True, False, info
    info["bottom_up"] = 1 - ((d[17] >> 5) & 1)
    comps, rgb16 = _comp(cmap_size, False) if cmap_type else _comp(bpp, (typ & 7) == 3)
    info["channels_in_file"], info["rgb16"] = comps, int(rgb16)
    if 18 + d[0] > len(d):
        return True, False, info
    info["data_offset"] = 18 + d[0]
    if w * h * comps > 0x7fffffff:                                         # the project's deviation
        return True, False, info
    return True, True, info


def _rgb16(v):
    v = v.astype(np.uint32)
    return np.stack([((v >> 10) & 31) * 255 // 31, ((v >> 5) & 31) * 255 // 31, (v & 31) * 255 // 31], -1).astype(np.uint8)


def decode(data, req_comp=0):
    """-> None when the load is refused, else (pixels (h, w, comps) uint8, info dict)"""
    det, ok, info = parse(data)
    if not ok:
        return None
    d = np.frombuffer(bytes(data), np.uint8)
    w, h, comps, rgb16, indexed = info["width"], info["height"], info["channels_in_file"], info["rgb16"], info["indexed"]
    target = req_comp or comps
    npix = w * h
    if npix * target > 0x7fffffff:
        return None
    pos = info["data_offset"]
    palette = None
    if indexed:
        pos += info["palette_start"]                                        # BYTES, not entries
        esz = 2 if rgb16 else comps
        end = pos + info["palette_len"] * esz
        if end > d.size:
            return None
        ent = d[pos:end].reshape(info["palette_len"], esz)
        palette = _rgb16(ent[:, 0].astype(np.uint16) | ent[:, 1].astype(np.uint16) << 8) if rgb16 else ent
        pos = end
    bps = info["bpp"] // 8 if indexed else 2 if rgb16 else comps
    if not info["rle"]:
        if pos + npix * bps > d.size:
            return None
        src = d[pos:pos + npix * bps]
    else:
        parts, made = [], 0
        while made < npix:
            if pos >= d.size:
                return None                                                # the command byte is missing
            cmd = int(d[pos]); cnt = (cmd & 127) + 1; need = min(cnt, npix - made)
            if cmd & 0x80:
                if pos + 1 + bps > d.size:
                    return None
                parts.append(np.tile(d[pos + 1:pos + 1 + bps], need)); pos += 1 + bps
            else:
                if pos + 1 + need * bps > d.size:
                    return None                                            # a pixel that is needed is missing
                parts.append(d[pos + 1:pos + 1 + need * bps]); pos += 1 + cnt * bps
            made += need
        src = np.concatenate(parts)
    src = src.reshape(npix, bps)
    if indexed:
        idx = src[:, 0].astype(np.int64) if bps == 1 else src[:, 0].astype(np.int64) | src[:, 1].astype(np.int64) << 8
        idx[idx >= info["palette_len"]] = 0
        px = palette[idx]
    elif rgb16:
        px = _rgb16(src[:, 0].astype(np.uint16) | src[:, 1].astype(np.uint16) << 8)
    else:
        px = src
    if comps >= 3 and not rgb16:
        px = px[:, [2, 1, 0, 3][:comps]]
    px = px.reshape(h, w, comps)
    if info["bottom_up"]:
        px = px[::-1]
    if target != comps:
        rgb = np.repeat(px[..., :1], 3, -1) if comps <= 2 else px[..., :3]
        if target == 4:
            a = px[..., comps - 1:comps] if comps in (2, 4) else np.full((h, w, 1), 255, np.uint8)
            rgb = np.concatenate([rgb, a], -1)
        px = rgb
    return np.ascontiguousarray(px), info
