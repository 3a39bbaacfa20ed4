/* tga_ref.c -- TGADecoder.getImageInfo + decodeImage (source/gamut/codecs/tga.d:313-647) restated serially, as a cursor walk over a
 * memory stream with the reference's semantics (io.d: a read past the end fails, a skip up to and including the end succeeds), plus
 * convertTo(rgb8 / rgba8) for req_comp 3 / 4.  The test suite's first reference; tests/tga_ref.py is the second, independent one.
 *
 * tgaref_load returns a bit set: 1 detected (getImageInfo), 2 header loadable (descriptor, ID skip, size), 4 pixels decoded into
 * `out` (only when out != NULL and the bits 1 | 2 are set).  info[0..13]: width, height, bpp, image_type, rle, indexed, rgb16,
 * channels_in_file, bottom_up, palette_start, palette_len, cmap_size, data_offset, detected. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { const uint8_t* p; long len, pos; int err; } stream;

static int rd8(stream* s) { if (s->pos < s->len) return s->p[s->pos++]; s->err = 1; return 0; }
static int rd16(stream* s)
{
    if (s->len - s->pos >= 2) { int v = s->p[s->pos] | s->p[s->pos + 1] << 8; s->pos += 2; return v; }
    s->err = 1; return 0;
}
static int skip(stream* s, long n) { if (s->pos + n <= s->len) { s->pos += n; return 1; } return 0; }
static long rdn(stream* s, uint8_t* dst, long n)
{
    long have = s->len - s->pos; if (have > n) have = n;
    memcpy(dst, s->p + s->pos, (size_t)have); s->pos += have; return have;
}

static int get_comp(int bits, int is_grey, int* rgb16)
{
    *rgb16 = 0;
    switch (bits) {
    case 8: return 1;
    case 16: if (is_grey) return 2; /* fallthrough */
    case 15: *rgb16 = 1; return 3;
    case 24: case 32: return bits / 8;
    default: return 0;
    }
}

static void read_rgb16(stream* s, uint8_t* o)
{
    int px = rd16(s);
    if (s->err) return;
    o[0] = (uint8_t)((((px >> 10) & 31) * 255) / 31);
    o[1] = (uint8_t)((((px >> 5) & 31) * 255) / 31);
    o[2] = (uint8_t)(((px & 31) * 255) / 31);
}

int tgaref_load(const uint8_t* data, long len, int req_comp, uint8_t* out, long out_cap, int32_t* info)
{
    stream s = { data, len, 0, 0 };
    int id_len, cmap_type, type, pal_start = 0, pal_len = 0, cmap_size = 0, w, h, bpp, rle = 0, inverted, comps, rgb16 = 0, indexed;
    memset(info, 0, 14 * sizeof(int32_t));
    id_len = rd8(&s); if (s.err) return 0;
    cmap_type = rd8(&s); if (s.err || cmap_type > 1) return 0;
    type = rd8(&s); if (s.err) return 0;
    if (cmap_type == 1) {
        if (type != 1 && type != 9) return 0;
        pal_start = rd16(&s); if (s.err) return 0;
        pal_len = rd16(&s); if (s.err) return 0;
        if (pal_len == 0) return 0;
        cmap_size = rd8(&s); if (s.err) return 0;
        if (cmap_size != 8 && cmap_size != 15 && cmap_size != 16 && cmap_size != 24 && cmap_size != 32) return 0;
        if (!skip(&s, 4)) return 0;
    } else {
        if (type != 2 && type != 3 && type != 10 && type != 11) return 0;
        if (!skip(&s, 9)) return 0;
    }
    w = rd16(&s); if (s.err) return 0;
    h = rd16(&s); if (s.err) return 0;
    if (w < 1 || h < 1) return 0;
    bpp = rd8(&s); if (s.err) return 0;
    if (cmap_type == 1 && bpp != 8 && bpp != 16) return 0;
    if (bpp != 8 && bpp != 15 && bpp != 16 && bpp != 24 && bpp != 32) return 0;
    info[13] = 1; info[0] = w; info[1] = h; info[2] = bpp; info[5] = cmap_type; info[9] = pal_start; info[10] = pal_len; info[11] = cmap_size;
    /* decodeImage */
    if (type >= 8) { type -= 8; rle = 1; }
    info[3] = type; info[4] = rle;
    inverted = rd8(&s); if (s.err) return 1;
    inverted = 1 - ((inverted >> 5) & 1);
    info[8] = inverted;
    indexed = cmap_type != 0;
    comps = indexed ? get_comp(cmap_size, 0, &rgb16) : get_comp(bpp, type == 3, &rgb16);
    info[6] = rgb16; info[7] = comps;
    if (!skip(&s, id_len)) return 1;
    info[12] = (int32_t)s.pos;
    if ((int64_t)w * h * comps > 0x7fffffffLL) return 1;                    /* the project's deviation: the reference's ints wrap */
    if (!out) return 3;
    {
        const int target = req_comp ? req_comp : comps;
        const long npix = (long)w * h;
        uint8_t* px; uint8_t* palette = NULL;
        long i; int j;
        if ((int64_t)npix * target > 0x7fffffffLL || npix * target > out_cap) return 3;
        px = (uint8_t*)malloc((size_t)(npix * comps));
        if (!px) return 3;
        if (!indexed && !rle && !rgb16) {
            for (i = 0; i < h; ++i) {
                long row = inverted ? h - i - 1 : i, bytes = (long)w * comps;
                if (rdn(&s, px + row * w * comps, bytes) != bytes) { free(px); return 3; }
            }
        } else {
            int count = 0, repeating = 0, read_next = 1;
            uint8_t raw[4] = { 0, 0, 0, 0 };
            if (indexed) {
                if (!skip(&s, pal_start)) { free(px); return 3; }
                palette = (uint8_t*)malloc((size_t)pal_len * comps);
                if (rgb16) {
                    for (i = 0; i < pal_len; ++i) { read_rgb16(&s, palette + i * comps); if (s.err) { free(palette); free(px); return 3; } }
                } else if (rdn(&s, palette, (long)pal_len * comps) != (long)pal_len * comps) { free(palette); free(px); return 3; }
            }
            for (i = 0; i < npix; ++i) {
                if (rle) {
                    if (count == 0) {
                        int cmd = rd8(&s);
                        if (s.err) goto fail;
                        count = 1 + (cmd & 127); repeating = cmd >> 7; read_next = 1;
                    } else if (!repeating) read_next = 1;
                } else read_next = 1;
                if (read_next) {
                    if (indexed) {
                        int idx = bpp == 8 ? rd8(&s) : rd16(&s);
                        if (s.err) goto fail;
                        if (idx >= pal_len) idx = 0;
                        for (j = 0; j < comps; ++j) raw[j] = palette[idx * comps + j];
                    } else if (rgb16) {
                        read_rgb16(&s, raw);
                        if (s.err) goto fail;
                    } else {
                        for (j = 0; j < comps; ++j) { raw[j] = (uint8_t)rd8(&s); if (s.err) goto fail; }
                    }
                    read_next = 0;
                }
                for (j = 0; j < comps; ++j) px[i * comps + j] = raw[j];
                --count;
            }
            if (inverted) {
                long row_bytes = (long)w * comps, y, k;
                for (y = 0; y * 2 < h; ++y)
                    for (k = 0; k < row_bytes; ++k) {
                        uint8_t t = px[y * row_bytes + k];
                        px[y * row_bytes + k] = px[(h - 1 - y) * row_bytes + k];
                        px[(h - 1 - y) * row_bytes + k] = t;
                    }
            }
            free(palette); palette = NULL;
        }
        if (comps >= 3 && !rgb16)
            for (i = 0; i < npix; ++i) { uint8_t t = px[i * comps]; px[i * comps] = px[i * comps + 2]; px[i * comps + 2] = t; }
        /* convertTo(rgb8 / rgba8): grey replicated, missing alpha 255, alpha dropped */
        for (i = 0; i < npix; ++i) {
            const uint8_t* p = px + i * comps; uint8_t* o = out + i * target;
            if (target == comps) { for (j = 0; j < comps; ++j) o[j] = p[j]; continue; }
            if (comps <= 2) { o[0] = o[1] = o[2] = p[0]; if (target == 4) o[3] = comps == 2 ? p[1] : 255; }
            else { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; if (target == 4) o[3] = comps == 4 ? p[3] : 255; }
        }
        free(px);
        return 7;
    fail:
        free(palette); free(px);
        return 3;
    }
}
