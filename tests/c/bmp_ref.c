/* bmp_ref.c -- a serial restatement of the reference's BMP loader and writer, for the tests: stbi__bmp_load with its header parse
 * (source/gamut/codecs/stbdec.d:2112-2512) as a STREAM reader, the way the reference is written (get8 / skip on a cursor; where the
 * pixels start falls out of the skips), and write_bmp (source/gamut/codecs/bmpenc.d:25-114) with saveBMP's limits
 * (source/gamut/plugins/bmp.d:174-189).  Bytes past the end of the input read as 0 (stbi__get8).  bytes_read_so_far (:2297) is the
 * cursor.  Three deliberate deviations, the library's: a negative palette size is refused; width or height 0 is refused; palette
 * entries from the palette size on are (0, 0, 0) instead of uninitialised; and, in the writer, row pad bytes are 0.
 * gcc -O2 -std=c99 -shared -fPIC tests/c/bmp_ref.c */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { const uint8_t* p; long len, pos; } ctx;
static int get8(ctx* s) { int v = (s->pos >= 0 && s->pos < s->len) ? s->p[s->pos] : 0; s->pos++; return v; }
static int get16le(ctx* s) { int z = get8(s); return z + (get8(s) << 8); }
static uint32_t get32le(ctx* s) { uint32_t z = (uint32_t)get16le(s); return z + ((uint32_t)get16le(s) << 16); }
static void skip(ctx* s, int n) { s->pos += n; }

typedef struct { int bpp, offset, hsz; uint32_t mr, mg, mb, ma, all_a; int extra_read; int compress; } bmp_data;

static int set_mask_defaults(bmp_data* info, int compress)                 /* :2121 */
{
    if (compress == 3) return 1;
    if (compress == 0) {
        if (info->bpp == 16) { info->mr = 31u << 10; info->mg = 31u << 5; info->mb = 31u << 0; }
        else if (info->bpp == 32) { info->mr = 0xffu << 16; info->mg = 0xffu << 8; info->mb = 0xffu << 0; info->ma = 0xffu << 24; info->all_a = 0; }
        else info->mr = info->mg = info->mb = info->ma = 0;
        return 1;
    }
    return 0;
}

static int parse_header(ctx* s, bmp_data* info, uint32_t* img_x, uint32_t* img_y, float* dens)   /* :2147 */
{
    int hsz;
    if (get8(s) != 'B' || get8(s) != 'M') return 0;
    get32le(s); get16le(s); get16le(s);
    info->offset = (int)get32le(s);
    info->hsz = hsz = (int)get32le(s);
    info->mr = info->mg = info->mb = info->ma = 0;
    info->extra_read = 14;
    info->compress = 0;
    dens[0] = dens[1] = dens[2] = -1;
    if (info->offset < 0) return 0;
    if (hsz != 12 && hsz != 40 && hsz != 56 && hsz != 108 && hsz != 124) return 0;
    if (hsz == 12) { *img_x = (uint32_t)get16le(s); *img_y = (uint32_t)get16le(s); }
    else { *img_x = get32le(s); *img_y = get32le(s); }
    if (get16le(s) != 1) return 0;
    info->bpp = get16le(s);
    if (hsz != 12) {
        int compress = (int)get32le(s);
        info->compress = compress;
        if (compress == 1 || compress == 2) return 0;
        if (compress >= 4) return 0;
        if (compress == 3 && info->bpp != 16 && info->bpp != 32) return 0;
        get32le(s);
        {
            int xp = (int)get32le(s), yp = (int)get32le(s);
            if (xp > 1) dens[0] = (float)xp;
            if (yp > 1) dens[1] = (float)yp;
            if (dens[0] != -1 && dens[1] != -1) dens[2] = dens[0] / dens[1];
        }
        get32le(s); get32le(s);
        if (hsz == 40 || hsz == 56) {
            if (hsz == 56) { get32le(s); get32le(s); get32le(s); get32le(s); }
            if (info->bpp == 16 || info->bpp == 32) {
                if (compress == 0) set_mask_defaults(info, compress);
                else if (compress == 3) {
                    info->mr = get32le(s); info->mg = get32le(s); info->mb = get32le(s);
                    info->extra_read += 12;
                    if (info->mr == info->mg && info->mg == info->mb) return 0;
                } else return 0;
            }
        } else {
            int i;
            info->mr = get32le(s); info->mg = get32le(s); info->mb = get32le(s); info->ma = get32le(s);
            if (compress != 3) set_mask_defaults(info, compress);
            get32le(s);
            for (i = 0; i < 12; ++i) get32le(s);
            if (hsz == 124) { get32le(s); get32le(s); get32le(s); get32le(s); }
        }
    }
    return 1;
}

static int high_bit(uint32_t z)                                              /* :2468 */
{
    int n = 0;
    if (z == 0) return -1;
    if (z >= 0x10000) { n += 16; z >>= 16; }
    if (z >= 0x00100) { n += 8; z >>= 8; }
    if (z >= 0x00010) { n += 4; z >>= 4; }
    if (z >= 0x00004) { n += 2; z >>= 2; }
    if (z >= 0x00002) { n += 1; }
    return n;
}
static int bitcount(uint32_t a)                                              /* :2480 */
{
    a = (a & 0x55555555) + ((a >> 1) & 0x55555555);
    a = (a & 0x33333333) + ((a >> 2) & 0x33333333);
    a = (a + (a >> 4)) & 0x0f0f0f0f;
    a = (a + (a >> 8));
    a = (a + (a >> 16));
    return (int)(a & 0xff);
}
static int shiftsigned(uint32_t v, int shift, int bits)                      /* :2493 */
{
    static const uint32_t mul_table[9] = { 0, 0xff, 0x55, 0x49, 0x11, 0x21, 0x41, 0x81, 0x01 };
    static const uint32_t shift_table[9] = { 0, 0, 0, 1, 0, 2, 4, 6, 0 };
    if (shift < 0) v <<= -shift; else v >>= shift;
    v >>= (8 - bits);
    return (int)(v * mul_table[bits]) >> shift_table[bits];
}
static uint8_t compute_y(int r, int g, int b) { return (uint8_t)(((r * 77) + (g * 150) + (29 * b)) >> 8); }

static int mad3_valid(long a, long b, long c) { return a >= 0 && b >= 0 && c >= 0 && (b == 0 || a <= 2147483647L / b) && (c == 0 || a * b <= 2147483647L / c); }

/* returns 1 and fills info / dens (and out, when it is not NULL and out_cap suffices) or 0 when the file is refused.
 * info: width height bpp hsz compress img_n top_down pixel_offset psize mr mg mb ma */
int bmpref_load(const uint8_t* data, long len, int req_comp, uint8_t* out, long out_cap, uint32_t* oinfo, float* dens)
{
    ctx S = { data, data ? len : 0, 0 }; ctx* s = &S;
    uint8_t* o;
    uint32_t mr, mg, mb, ma, all_a, img_x = 0, img_y = 0;
    static uint8_t pal[256][4];
    int psize = 0, i, j, width, flip_vertically, pad, target, img_n;
    long pixel_offset = -1;
    bmp_data info;
    memset(pal, 0, sizeof(pal));                                              /* DEVIATION: entries past psize are (0, 0, 0) */
    info.all_a = 255;
    if (!parse_header(s, &info, &img_x, &img_y, dens)) return 0;
    flip_vertically = ((int)img_y) > 0;
    if ((int)img_y < 0) img_y = 0u - img_y;
    if (img_y > (1u << 24)) return 0;
    if (img_x > (1u << 24)) return 0;
    if (img_x == 0 || img_y == 0) return 0;                                   /* DEVIATION */
    mr = info.mr; mg = info.mg; mb = info.mb; ma = info.ma; all_a = info.all_a;
    if (info.hsz == 12) { if (info.bpp < 24) psize = (info.offset - info.extra_read - 24) / 3; }
    else { if (info.bpp < 16) psize = (info.offset - info.extra_read - info.hsz) >> 2; }
    if (psize < 0) return 0;                                                  /* DEVIATION */
    if (psize == 0) {
        int bytes_read_so_far = (int)s->pos;
        if (bytes_read_so_far <= 0 || bytes_read_so_far > 1024) return 0;
        if (info.offset < bytes_read_so_far || info.offset - bytes_read_so_far > 1024) return 0;
        skip(s, info.offset - bytes_read_so_far);
    }
    if (info.bpp == 24 && ma == 0xff000000) img_n = 3; else img_n = ma ? 4 : 3;
    target = (req_comp && req_comp >= 3) ? req_comp : img_n;
    if (!mad3_valid(target, img_x, img_y)) return 0;
    o = out ? (uint8_t*)malloc((size_t)target * img_x * img_y) : NULL;      /* out == NULL: the verdict and the header fields only */
    if (out && !o) return 0;
    if (info.bpp < 16) {
        long z = 0;
        if (psize == 0 || psize > 256) { free(o); return 0; }
        for (i = 0; i < psize; ++i) {
            pal[i][2] = (uint8_t)get8(s); pal[i][1] = (uint8_t)get8(s); pal[i][0] = (uint8_t)get8(s);
            if (info.hsz != 12) get8(s);
            pal[i][3] = 255;
        }
        skip(s, info.offset - info.extra_read - info.hsz - psize * (info.hsz == 12 ? 3 : 4));
        if (info.bpp == 1) width = (int)((img_x + 7) >> 3);
        else if (info.bpp == 4) width = (int)((img_x + 1) >> 1);
        else if (info.bpp == 8) width = (int)img_x;
        else { free(o); return 0; }
        pad = (-width) & 3;
        pixel_offset = s->pos;
        if (!out) goto done;
        if (info.bpp == 1) {
            for (j = 0; j < (int)img_y; ++j) {
                int bit_offset = 7, v = get8(s);
                for (i = 0; i < (int)img_x; ++i) {
                    int color = (v >> bit_offset) & 0x1;
                    o[z++] = pal[color][0]; o[z++] = pal[color][1]; o[z++] = pal[color][2];
                    if (target == 4) o[z++] = 255;
                    if (i + 1 == (int)img_x) break;
                    if ((--bit_offset) < 0) { bit_offset = 7; v = get8(s); }
                }
                skip(s, pad);
            }
        } else {
            for (j = 0; j < (int)img_y; ++j) {
                for (i = 0; i < (int)img_x; i += 2) {
                    int v = get8(s), v2 = 0;
                    if (info.bpp == 4) { v2 = v & 15; v >>= 4; }
                    o[z++] = pal[v][0]; o[z++] = pal[v][1]; o[z++] = pal[v][2];
                    if (target == 4) o[z++] = 255;
                    if (i + 1 == (int)img_x) break;
                    v = (info.bpp == 8) ? get8(s) : v2;
                    o[z++] = pal[v][0]; o[z++] = pal[v][1]; o[z++] = pal[v][2];
                    if (target == 4) o[z++] = 255;
                }
                skip(s, pad);
            }
        }
    } else {
        int rshift = 0, gshift = 0, bshift = 0, ashift = 0, rcount = 0, gcount = 0, bcount = 0, acount = 0;
        long z = 0;
        int easy = 0;
        if (info.offset - info.extra_read - info.hsz < 0) { free(o); return 0; }  /* (cannot happen behind the tests above) */
        skip(s, info.offset - info.extra_read - info.hsz);
        if (info.bpp == 24) width = (int)(3 * img_x);
        else if (info.bpp == 16) width = (int)(2 * img_x);
        else width = 0;
        pad = (-width) & 3;
        if (info.bpp == 24) easy = 1;
        else if (info.bpp == 32) { if (mb == 0xff && mg == 0xff00 && mr == 0x00ff0000 && ma == 0xff000000) easy = 2; }
        if (!easy) {
            if (!mr || !mg || !mb) { free(o); return 0; }
            rshift = high_bit(mr) - 7; rcount = bitcount(mr);
            gshift = high_bit(mg) - 7; gcount = bitcount(mg);
            bshift = high_bit(mb) - 7; bcount = bitcount(mb);
            ashift = high_bit(ma) - 7; acount = bitcount(ma);
            if (rcount > 8 || gcount > 8 || bcount > 8 || acount > 8) { free(o); return 0; }
        }
        pixel_offset = s->pos;
        if (!out) goto done;
        for (j = 0; j < (int)img_y; ++j) {
            if (easy) {
                for (i = 0; i < (int)img_x; ++i) {
                    uint8_t a;
                    o[z + 2] = (uint8_t)get8(s); o[z + 1] = (uint8_t)get8(s); o[z + 0] = (uint8_t)get8(s);
                    z += 3;
                    a = (uint8_t)(easy == 2 ? get8(s) : 255);
                    all_a |= a;
                    if (target == 4) o[z++] = a;
                }
            } else {
                int bpp = info.bpp;
                for (i = 0; i < (int)img_x; ++i) {
                    uint32_t v = (bpp == 16 ? (uint32_t)get16le(s) : get32le(s));
                    uint32_t a;
                    o[z++] = (uint8_t)(shiftsigned(v & mr, rshift, rcount) & 255);
                    o[z++] = (uint8_t)(shiftsigned(v & mg, gshift, gcount) & 255);
                    o[z++] = (uint8_t)(shiftsigned(v & mb, bshift, bcount) & 255);
                    a = (ma ? (uint32_t)shiftsigned(v & ma, ashift, acount) : 255);
                    all_a |= a;
                    if (target == 4) o[z++] = (uint8_t)(a & 255);
                }
            }
            skip(s, pad);
        }
    }
    if (target == 4 && all_a == 0)
        for (long k = 4L * img_x * img_y - 1; k >= 0; k -= 4) o[k] = 255;
    if (flip_vertically) {
        for (j = 0; j < (int)img_y >> 1; ++j) {
            uint8_t* p1 = o + (size_t)j * img_x * target;
            uint8_t* p2 = o + (size_t)(img_y - 1 - j) * img_x * target;
            for (i = 0; i < (int)img_x * target; ++i) { uint8_t t = p1[i]; p1[i] = p2[i]; p2[i] = t; }
        }
    }
    {
        const int final = req_comp ? req_comp : target;
        const long npx = (long)img_x * img_y;
        if (out && npx * final <= out_cap) {
            if (final == target) memcpy(out, o, (size_t)npx * final);
            else {                                                            /* stbi__convert_format, the pairs that occur: 3 / 4 -> 1 / 2 */
                for (long k = 0; k < npx; ++k) {
                    const uint8_t* q = o + k * target;
                    out[k * final] = compute_y(q[0], q[1], q[2]);
                    if (final == 2) out[k * final + 1] = target == 4 ? q[3] : 255;
                }
            }
        }
    }
done:
    free(o);
    oinfo[0] = img_x; oinfo[1] = img_y; oinfo[2] = (uint32_t)info.bpp; oinfo[3] = (uint32_t)info.hsz; oinfo[4] = (uint32_t)info.compress;
    oinfo[5] = (uint32_t)img_n; oinfo[6] = flip_vertically ? 0 : 1; oinfo[7] = (uint32_t)pixel_offset; oinfo[8] = (uint32_t)psize;
    oinfo[9] = mr; oinfo[10] = mg; oinfo[11] = mb; oinfo[12] = ma;
    return 1;
}

static void le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* saveBMP + write_bmp: the file at out (122 + h * padded row bytes), its length, or 0 when refused; rows `pitch` bytes apart */
long bmpref_write(const uint8_t* px, long pitch, int w, int h, int comp, int ppm_x, int ppm_y, uint8_t* out)
{
    if ((comp != 3 && comp != 4) || w < 1 || h < 1 || w > 32767 || h > 32767) return 0;   /* plugins/bmp.d:174-189 */
    const int linesize = w * comp, pad = 3 - ((linesize - 1) & 3);
    const long filesize = 122 + (long)h * (linesize + pad);
    uint8_t* hdr = out;
    memset(hdr, 0, 122);
    hdr[0] = 0x42; hdr[1] = 0x4d;
    le32(hdr + 2, (uint32_t)filesize);
    le32(hdr + 10, 122); le32(hdr + 14, 108);
    le32(hdr + 18, (uint32_t)w); le32(hdr + 22, (uint32_t)h);
    hdr[26] = 1; hdr[27] = 0; hdr[28] = (uint8_t)(comp * 8); hdr[29] = 0;
    le32(hdr + 30, comp == 3 ? 0 : 3);
    le32(hdr + 38, (uint32_t)ppm_x); le32(hdr + 42, (uint32_t)ppm_y);
    if (comp == 4) { static const uint8_t b[16] = { 0, 0, 0xff, 0, 0, 0xff, 0, 0, 0xff, 0, 0, 0, 0, 0, 0, 0xff }; memcpy(hdr + 54, b, 16); }
    memcpy(hdr + 70, "BGRs", 4);
    uint8_t* o = out + 122;
    for (int y = 0; y < h; ++y) {
        const uint8_t* in = px + (long)(h - 1 - y) * pitch;
        for (int x = 0; x < w; ++x) {
            o[x * comp + 0] = in[x * comp + 2]; o[x * comp + 1] = in[x * comp + 1]; o[x * comp + 2] = in[x * comp + 0];
            if (comp == 4) o[x * comp + 3] = in[x * comp + 3];
        }
        for (int k = 0; k < pad; ++k) o[linesize + k] = 0;                    /* DEVIATION: uninitialised in the reference */
        o += linesize + pad;
    }
    return filesize;
}
