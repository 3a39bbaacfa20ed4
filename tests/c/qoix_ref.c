/* qoix_ref.c -- the 8-bit colour slice of the reference's QOIX loader restated serially, for the tests: the container
 * (source/gamut/plugins/qoix.d:350-473 qoix_lz4_decode, :476-507 identifyTypeFromStream), the LZ4 block
 * (source/gamut/codecs/lz4.d:760-978, LZ4_decompress_generic as LZ4_decompress_fast calls it: endOnOutputSize, full, withPrefix64k) and
 * the QOI2AVG op stream (source/gamut/codecs/qoi2avg.d:624-897 qoix_decode, two scanline buffers as there).
 *
 * The four deliberate deviations of gamut_amd/csrc/qoix.hip are part of this reading -- in each the reference touches memory it does
 * not own, so there is no behaviour to reproduce:
 *   1. LZ4: a read at or past the end of the file refuses the file;
 *   2. LZ4: offset 0, or a match starting before the first output byte, refuses the file;
 *   3. QOI2AVG: an END opcode that is executed refuses the file;
 *   4. QOI2AVG: an op byte read at index >= size refuses the file.
 * The library's early refusal of an `orig` above 255 * (length - 29) is NOT here: tests/test_qoix_cpu.py asserts that it never
 * disagrees with what this file decides.
 *
 * qoixref_load(data, len, channels, out, out_cap, info) -> header verdict (0 ok, 1 refused, 2 codec not built) | detected << 4 |
 * decoded << 5.  info: 12 words in the order of gamut_hip_qoix_info, the two floats as their bits.  out == NULL: header only. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef const uint8_t* bytes_t;

static uint32_t rd32(bytes_t p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

enum { T_L8 = 0, T_L16 = 1, T_LA8 = 3, T_LA16 = 4, T_LAP8 = 6, T_LAP16 = 7, T_RGB8 = 9, T_RGB16 = 10, T_RGBA8 = 12, T_RGBA16 = 13,
       T_RGBAP8 = 15, T_RGBAP16 = 16 };                                      /* PixelType, types.d:62-86 */

/* qoix.d:476-507 */
static int type_from_stream(int channels, int bitdepth, int premul)
{
    if (bitdepth == 8)
        switch (channels) { case 1: return T_L8; case 2: return premul ? T_LAP8 : T_LA8; case 3: return T_RGB8; case 4: return premul ? T_RGBAP8 : T_RGBA8; default: return -1; }
    if (bitdepth == 10)
        switch (channels) { case 1: return T_L16; case 2: return premul ? T_LAP16 : T_LA16; case 3: return T_RGB16; case 4: return premul ? T_RGBAP16 : T_RGBA16; default: return -1; }
    return -1;
}

/* qoi2avg.d:634-666 on the bytes the sub-codec is handed (size, and the header with its compression byte reset) */
static int avg_header_ok(bytes_t hdr, long size, int compression_seen)
{
    uint32_t w = rd32(hdr + 4), h = rd32(hdr + 8);
    if (size < 25 + 4) return 0;
    if (w == 0 || h == 0) return 0;
    if (hdr[13] < 3 || hdr[13] > 4) return 0;
    if (hdr[15] > 2) return 0;
    if (hdr[14] != 8) return 0;
    if (hdr[12] > 1) return 0;
    if (compression_seen != 0) return 0;
    if (rd32(hdr) != 0x716F6978u) return 0;
    if (h >= 400000000u / w) return 0;
    return 1;
}

/* 0 ok, 1 refused, 2 codec not built; *sub: the size qoix_decode sees */
static int header(bytes_t d, long len, int32_t* info, long* sub)
{
    int i, type;
    for (i = 0; i < 12; ++i) info[i] = 0;
    info[10] = -1;
    info[11] = len >= 4 && d[0] == 0x71 && d[1] == 0x6f && d[2] == 0x69 && d[3] == 0x78;     /* detectQOIX :149-153 */
    *sub = 0;
    if (len > 0x7fffffffL) return 1;                                          /* loadQOIX :76, int len */
    if (len < 25) return 1;                                                   /* :356 */
    info[0] = (int32_t)rd32(d + 4); info[1] = (int32_t)rd32(d + 8);
    info[2] = d[12]; info[3] = d[13]; info[4] = d[14]; info[5] = d[15]; info[6] = d[16];
    info[7] = (int32_t)rd32(d + 17); info[8] = (int32_t)rd32(d + 21);
    type = type_from_stream(d[13], d[14], d[15] == 2);                        /* :367-375 */
    if (type < 0) return 1;
    info[10] = type;
    if (d[16] == 1) {                                                         /* :381-391 */
        if (len < 25 + 4) return 1;
        info[9] = (int32_t)rd32(d + 25);
        if (info[9] < 0) return 1;
        *sub = 25 + (long)info[9];
    } else if (d[16] == 0) *sub = len;                                        /* :412-416 */
    else return 1;                                                            /* :417-418 */
    if (d[14] == 10 || d[13] < 3) return 2;                                   /* :422-454 the other three codecs */
    return avg_header_ok(d, *sub, 0) ? 0 : 1;                                 /* the compression byte is reset before the call :397 */
}

/* lz4.d:776-963 with endOnInput = 0, partialDecoding = 0.  ip / iend index the whole file, op / oend the output. */
static int lz4_fast(bytes_t src, long ip, long iend, uint8_t* dst, long oend)
{
    long op = 0;
    for (;;) {
        unsigned token, s;
        long length, cpy, off, k;
        if (ip >= iend) return 0;                                             /* DEVIATION 1 */
        token = src[ip++];                                                    /* :807 */
        length = token >> 4;
        if (length == 15) {                                                   /* :808-816 */
            do {
                if (ip >= iend) return 0;                                     /* DEVIATION 1 */
                s = src[ip++];
                length += s;
            } while (s == 255);
        }
        cpy = op + length;                                                    /* :828 */
        if (cpy > oend - 8) {                                                 /* :830 COPYLENGTH */
            if (cpy != oend) return 0;                                        /* :842-845 */
            if (length > iend - ip) return 0;                                 /* DEVIATION 1 */
            memcpy(dst + op, src + ip, (size_t)length);                       /* :851 */
            return 1;                                                         /* :854 */
        }
        if (length > iend - ip) return 0;                                     /* DEVIATION 1 */
        memcpy(dst + op, src + ip, (size_t)length);                           /* :856 (the wild copy's surplus is overwritten later) */
        ip += length; op = cpy;
        if (iend - ip < 2) return 0;                                          /* DEVIATION 1 */
        off = src[ip] | src[ip + 1] << 8; ip += 2;                            /* :860 */
        if (off == 0 || off > op) return 0;                                   /* DEVIATION 2 */
        length = token & 15;                                                  /* :867-882 */
        if (length == 15) {
            do {
                if (ip >= iend) return 0;                                     /* DEVIATION 1 */
                s = src[ip++];
                length += s;
            } while (s == 255);
        }
        length += 4;
        cpy = op + length;                                                    /* :922 */
        if (cpy > oend - 12 && cpy > oend - 5) return 0;                      /* :935-940 */
        for (k = 0; k < length; ++k) dst[op + k] = dst[op + k - off];         /* :923-950, net effect */
        op = cpy;
    }
}

typedef struct { uint8_t r, g, b, a; } rgba_t;

/* qoi2avg.d:843-861, the scalar description of locoIntraPredictionSIMD */
static uint8_t loco(int a, int b, int c)
{
    int max_ab = a > b ? a : b, min_ab = a < b ? a : b;
    if (c <= min_ab) return (uint8_t)max_ab;                                  /* the SIMD code applies the max mask last: it wins a tie */
    if (c >= max_ab) return (uint8_t)min_ab;
    return (uint8_t)(a + b - c);
}

/* qoi2avg.d:668-838; bytes / size as the sub-codec sees them */
static int avg_decode(bytes_t bytes, long size, int channels, uint8_t* out)
{
    uint32_t width = rd32(bytes + 4), height = rd32(bytes + 8), posx, posy;
    rgba_t index[64], px, px_ref;
    long chunks_len = size - 4, p = 25;
    int run = 0, index_pos = 0, ok = 1;
    rgba_t* cur = (rgba_t*)calloc((size_t)width, sizeof(rgba_t));
    rgba_t* last = (rgba_t*)calloc((size_t)width, sizeof(rgba_t));
    if (!cur || !last) { free(cur); free(last); return 0; }
    memset(index, 0, sizeof(index));
    px.r = 0; px.g = 0; px.b = 0; px.a = 255;
    for (posy = 0; posy < height && ok; ++posy) {
        rgba_t* t;
        uint8_t* line = out + (size_t)posy * width * (size_t)channels;
        for (posx = 0; posx < width; ++posx) {
            if (run > 0) run--;
            else if (p < chunks_len) {
                int b1;
                px_ref = px;
                if (posy > 0) {
                    if (posx == 0) { px_ref.r = last[0].r; px_ref.g = last[0].g; px_ref.b = last[0].b; }
                    else {
                        px_ref.r = loco(px.r, last[posx].r, last[posx - 1].r);
                        px_ref.g = loco(px.g, last[posx].g, last[posx - 1].g);
                        px_ref.b = loco(px.b, last[posx].b, last[posx - 1].b);
                    }
                }
            decode_op:
                if (p >= size) { ok = 0; break; }                             /* DEVIATION 4 */
                b1 = bytes[p++];
#define NEED(n) if (p + (n) > size) { ok = 0; break; }                        /* DEVIATION 4 */
                if (b1 < 0x80) {
                    int vg = ((b1 >> 4) & 7) - 4;
                    px.g = (uint8_t)(px_ref.g + vg);
                    if (vg < 0) { px.r = (uint8_t)(px_ref.r + vg - 1 + ((b1 >> 2) & 3)); px.b = (uint8_t)(px_ref.b + vg - 1 + (b1 & 3)); }
                    else { px.r = (uint8_t)(px_ref.r + vg - 2 + ((b1 >> 2) & 3)); px.b = (uint8_t)(px_ref.b + vg - 2 + (b1 & 3)); }
                    index[index_pos++ & 63] = px;
                } else if (b1 < 0xc0) {
                    px = index[b1 & 63];
                } else if (b1 < 0xe0) {
                    int b2, vg = (b1 & 0x1f) - 16;
                    NEED(1) b2 = bytes[p++];
                    px.r = (uint8_t)(px_ref.r + vg - 8 + ((b2 >> 4) & 15));
                    px.g = (uint8_t)(px_ref.g + vg);
                    px.b = (uint8_t)(px_ref.b + vg - 8 + (b2 & 15));
                    index[index_pos++ & 63] = px;
                } else if (b1 < 0xe8) {
                    int dv, vg;
                    NEED(2) dv = (b1 << 8) | bytes[p++];
                    dv = (dv << 8) | bytes[p++];
                    vg = ((dv >> 12) & 0x7f) - 64;
                    px.r = (uint8_t)(px_ref.r + vg + ((dv >> 6) & 0x3f) - 32);
                    px.g = (uint8_t)(px_ref.g + vg);
                    px.b = (uint8_t)(px_ref.b + vg + (dv & 0x3f) - 32);
                    index[index_pos++ & 63] = px;
                } else if (b1 < 0xf0) {
                    px.a = (uint8_t)(px.a + (b1 & 7) - 4);
                    goto decode_op;
                } else if (b1 < 0xf8) {
                    run = b1 & 7;
                } else if (b1 < 0xfc) {
                    NEED(1) run = ((b1 & 3) << 8) | bytes[p++];
                } else if (b1 == 0xfc) {
                    NEED(1) px.r = px.g = px.b = bytes[p++];
                    index[index_pos++ & 63] = px;
                } else if (b1 == 0xfd) {
                    NEED(3) px.r = bytes[p++]; px.g = bytes[p++]; px.b = bytes[p++];
                    index[index_pos++ & 63] = px;
                } else if (b1 == 0xfe) {
                    NEED(4) px.r = bytes[p++]; px.g = bytes[p++]; px.b = bytes[p++]; px.a = bytes[p++];
                    index[index_pos++ & 63] = px;
                } else { ok = 0; break; }                                     /* DEVIATION 3 */
#undef NEED
            }
            cur[posx] = px;
        }
        if (!ok) break;
        for (posx = 0; posx < width; ++posx) {                                /* :807-828 */
            line[posx * (size_t)channels + 0] = cur[posx].r; line[posx * (size_t)channels + 1] = cur[posx].g; line[posx * (size_t)channels + 2] = cur[posx].b;
            if (channels == 4) line[posx * 4u + 3] = cur[posx].a;
        }
        t = cur; cur = last; last = t;
    }
    free(cur); free(last);
    return ok;
}

long qoixref_load(const uint8_t* data, long len, int channels, uint8_t* out, long out_cap, int32_t* info)
{
    long sub = 0, res;
    int rc = header(data, len, info, &sub), ok;
    res = rc | (long)info[11] << 4;
    if (rc != 0 || !out) return res;
    if (channels != 0 && channels != 3 && channels != 4) return res;          /* qoi2avg.d:636 */
    if (channels == 0) channels = info[3];
    if ((long)(uint32_t)info[0] * (uint32_t)info[1] * channels > out_cap) return res;
    if (info[6] == 1) {
        uint8_t* dec = (uint8_t*)malloc((size_t)sub + 1);                     /* :394-397 */
        if (!dec) return res;
        memcpy(dec, data, 25);
        dec[16] = 0;
        ok = lz4_fast(data, 29, len, dec + 25, sub - 25) && avg_header_ok(dec, sub, dec[16]) && avg_decode(dec, sub, channels, out);
        free(dec);
    } else ok = avg_decode(data, sub, channels, out);
    return res | (long)(ok != 0) << 5;
}
