/* png_write_ref.c -- a serial restatement of the reference's PNG writer around its compressor (stbi_write_png_to_mem and
 * stbiw__encode_png_line, codecs/stb_image_write.d:254-451), for the tests: pwr_filt returns the `filt` buffer that the reference
 * hands to stbi_zlib_compress, pwr_file the complete file it writes around a given zlib payload.  Written from the behaviour the
 * cited lines describe; no text of the reference is copied. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int iabs(int v) { return v < 0 ? -v : v; }

/* :262-268 */
static int paeth(int a, int b, int c)
{
    int p = a + b - c, pa = iabs(p - a), pb = iabs(p - b), pc = iabs(p - c);
    if (pa <= pb && pa <= pc) return a & 255;
    if (pb <= pc) return b & 255;
    return c & 255;
}

/* one row under one filter into line (:271-352).  Row 0 is remapped (:279): Up -> None, Average -> 5, Paeth -> 6. */
static void encode_line(const uint8_t* pixels, long stride, int width, int y, int n, int is16, int filter, int8_t* line)
{
    static const int first_row[5] = { 0, 1, 0, 5, 6 };
    const int type = y ? filter : first_row[filter];
    const uint8_t* z = pixels + stride * y;
    const int line_bytes = width * n * (is16 ? 2 : 1);
    const int sample = n * (is16 ? 2 : 1);           /* bytes per pixel: the first pixel has no left neighbour, and the left offset */
    int i;
    if (type == 0) {                                 /* :286-303: a copy; 16-bit samples go out big-endian */
        if (is16) for (i = 0; i < width * n; ++i) { line[2 * i] = (int8_t)z[2 * i + 1]; line[2 * i + 1] = (int8_t)z[2 * i]; }
        else memcpy(line, z, (size_t)line_bytes);
        return;
    }
    for (i = 0; i < sample; ++i) {                   /* :309-320 */
        switch (type) {
            case 2: line[i] = (int8_t)(z[i] - z[i - stride]); break;
            case 3: line[i] = (int8_t)(z[i] - (z[i - stride] >> 1)); break;
            case 4: line[i] = (int8_t)(z[i] - paeth(0, z[i - stride], 0)); break;
            default: line[i] = (int8_t)z[i]; break;  /* 1, 5, 6 */
        }
    }
    for (i = sample; i < line_bytes; ++i) {          /* :321-329 */
        switch (type) {
            case 1: line[i] = (int8_t)(z[i] - z[i - sample]); break;
            case 2: line[i] = (int8_t)(z[i] - z[i - stride]); break;
            case 3: line[i] = (int8_t)(z[i] - ((z[i - sample] + z[i - stride]) >> 1)); break;
            case 4: line[i] = (int8_t)(z[i] - paeth(z[i - sample], z[i - stride], z[i - stride - sample])); break;
            case 5: line[i] = (int8_t)(z[i] - (z[i - sample] >> 1)); break;
            default: line[i] = (int8_t)(z[i] - paeth(z[i - sample], 0, 0)); break;   /* 6 */
        }
    }
    if (is16)                                        /* :331-351: prediction ran on the native (little-endian) bytes; swap now */
        for (i = 0; i < width * n; ++i) { int8_t t = line[2 * i]; line[2 * i] = line[2 * i + 1]; line[2 * i + 1] = t; }
}

/* the filt buffer (:363-412): (line_bytes + 1) * y bytes into filt; returns that length, or -1 */
long pwr_filt(const uint8_t* pixels, long stride, int x, int y, int n, int is16, int force_filter, uint8_t* filt)
{
    const int line_bytes = x * n * (is16 ? 2 : 1);
    int8_t* line = (int8_t*)malloc((size_t)line_bytes + 1);
    int j;
    if (!line) return -1;
    if (force_filter >= 5) force_filter = -1;        /* :365 */
    for (j = 0; j < y; ++j) {
        int filter;
        if (force_filter > -1) {
            filter = force_filter;
            encode_line(pixels, stride, x, j, n, is16, filter, line);
        } else {                                     /* :384-405 */
            int best = 0, best_val = 0x7fffffff, i;
            for (filter = 0; filter < 5; ++filter) {
                int est = 0;
                encode_line(pixels, stride, x, j, n, is16, filter, line);
                for (i = 0; i < x * n; ++i) est += iabs(line[i]);          /* :394: x * n entries, whatever the sample size */
                if (est < best_val) { best_val = est; best = filter; }
            }
            if (filter != best) { encode_line(pixels, stride, x, j, n, is16, best, line); filter = best; }
        }
        filt[(long)j * (line_bytes + 1)] = (uint8_t)filter;                /* :409: the unmapped type */
        memcpy(filt + (long)j * (line_bytes + 1) + 1, line, (size_t)line_bytes);
    }
    free(line);
    return (long)(line_bytes + 1) * y;
}

static uint32_t crc32_of(const uint8_t* p, long n)
{
    uint32_t c = 0xFFFFFFFFu;
    long i; int k;
    for (i = 0; i < n; ++i) { c ^= p[i]; for (k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; }
    return ~c;
}
static uint8_t* be32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; return o + 4; }

/* the file around a zlib payload (:419-449): 8 + 25 + 12 + zlen + 12 bytes into out; returns that length */
long pwr_file(int x, int y, int n, int is16, const uint8_t* zlib, long zlen, uint8_t* out)
{
    static const uint8_t sig[8] = { 137, 80, 78, 71, 13, 10, 26, 10 };
    static const int ctype[5] = { -1, 0, 4, 2, 6 };
    uint8_t* o = out;
    uint8_t* tag;
    memcpy(o, sig, 8); o += 8;
    o = be32(o, 13); tag = o; memcpy(o, "IHDR", 4); o += 4;
    o = be32(o, (uint32_t)x); o = be32(o, (uint32_t)y);
    *o++ = is16 ? 16 : 8; *o++ = (uint8_t)ctype[n]; *o++ = 0; *o++ = 0; *o++ = 0;
    o = be32(o, crc32_of(tag, 17));
    o = be32(o, (uint32_t)zlen); tag = o; memcpy(o, "IDAT", 4); o += 4;
    memcpy(o, zlib, (size_t)zlen); o += zlen;
    o = be32(o, crc32_of(tag, zlen + 4));
    o = be32(o, 0); tag = o; memcpy(o, "IEND", 4); o += 4;
    o = be32(o, crc32_of(tag, 4));
    return (long)(o - out);
}
