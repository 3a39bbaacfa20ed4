/* qoix_write_ref.c -- the QOIX writer for 8-bit rgb / rgba restated serially: qoix_encode (source/gamut/codecs/qoi2avg.d:376-615),
 * LZ4_compress on a 64-bit build (codecs/lz4.d:289-554: byU16 below 65547 input bytes, byU32 from there), LZ4_compressBound, and the
 * "smaller one wins" container of qoix_lz4_encode (plugins/qoix.d:251-339).  The oracle of the GPU encoder, and the host-core
 * yardstick of tools/qoix_encode_bench.py.
 *
 * Every access is bounded; a row is read as width * channels bytes whatever the pitch is (the reference's memcpy of pitchBytes for
 * 4 channels is the GPU encoder's deviation 1), and the pitch may be negative.  Results: a length, -1 when the reference refuses
 * the description, -2 when `cap` is too small or memory runs out. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { HEADER = 25, PIXELS_MAX = 400000000 };

static uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

/* ---- LZ4 ----------------------------------------------------------------------------------------------------------------------- */

long qoixwref_lz4_bound(long n) { return n < 0 || n > 0x7E000000L ? 0 : n + n / 255 + 16; }

static uint32_t lz_hash(uint32_t seq, int u16) { return (seq * 2654435761u) >> (u16 ? 19 : 20); }            /* 13 / 12 bits */

/* length field behind a nibble of 15: the reference's loops (255-byte steps; the match form's 510 step writes the same bytes) */
static long put_len(uint8_t* out, long op, long cap, long n)
{
    for (; n >= 255; n -= 255) { if (op >= cap) return -2; out[op++] = 255; }
    if (op >= cap) return -2;
    out[op++] = (uint8_t)n;
    return op;
}

long qoixwref_lz4_compress(const uint8_t* src, long n, uint8_t* out, long cap)
{
    if (n < 0 || n > 0x7E000000L) return 0;
    const int u16 = n < 65547;
    uint32_t* table = (uint32_t*)calloc(8192, sizeof(uint32_t));                  /* entries hold positions; byU16's fit 16 bits */
    if (!table) return -2;
    long ip = 0, anchor = 0, op = 0;
    const long mflimit = n - 12, matchlimit = n - 5;
#define FAIL do { free(table); return -2; } while (0)
    if (n >= 13) {
        table[lz_hash(rd32(src), u16)] = 0;
        ip = 1;
        for (;;) {
            long match, fwd = ip;
            uint32_t attempts = 64;
            long step = 1;
            int over = 0;
            for (;;) {                                                            /* the search :399-426 */
                ip = fwd;
                fwd += step;
                step = attempts++ >> 6;
                if (fwd > mflimit) { over = 1; break; }
                const uint32_t h = lz_hash(rd32(src + ip), u16);
                match = table[h];
                table[h] = (uint32_t)ip;
                if (!u16 && match + 65535 < ip) continue;
                if (rd32(src + match) == rd32(src + ip)) break;
            }
            if (over) break;
            while (ip > anchor && match > 0 && src[ip - 1] == src[match - 1]) { --ip; --match; }      /* catch up :430 */
            const long lit = ip - anchor;
            long token = op++;
            if (token >= cap) FAIL;
            if (lit >= 15) { out[token] = 0xF0; if ((op = put_len(out, op, cap, lit - 15)) < 0) FAIL; }
            else out[token] = (uint8_t)(lit << 4);
            if (op + lit > cap) FAIL;
            memcpy(out + op, src + anchor, (size_t)lit); op += lit;
            for (;;) {                                                            /* _next_match :452-521 */
                if (op + 2 > cap) FAIL;
                out[op++] = (uint8_t)(ip - match); out[op++] = (uint8_t)((ip - match) >> 8);
                long ml = 0;
                while (ip + 4 + ml < matchlimit && src[match + 4 + ml] == src[ip + 4 + ml]) ++ml;     /* LZ4_count */
                ip += 4 + ml;
                if (ml >= 15) { out[token] += 15; if ((op = put_len(out, op, cap, ml - 15)) < 0) FAIL; }
                else out[token] += (uint8_t)ml;
                anchor = ip;
                if (ip > mflimit) break;
                table[lz_hash(rd32(src + ip - 2), u16)] = (uint32_t)(ip - 2);
                const uint32_t h = lz_hash(rd32(src + ip), u16);
                match = table[h];
                table[h] = (uint32_t)ip;
                if (match + 65535 >= ip && rd32(src + match) == rd32(src + ip)) {
                    token = op++;
                    if (token >= cap) FAIL;
                    out[token] = 0;
                    continue;
                }
                break;
            }
            if (ip > mflimit) break;
            ++ip;
        }
    }
    {                                                                             /* _last_literals :527-537 */
        const long last = n - anchor;
        if (op >= cap) FAIL;
        if (last >= 15) { out[op++] = 0xF0; if ((op = put_len(out, op, cap, last - 15)) < 0) FAIL; }
        else out[op++] = (uint8_t)(last << 4);
        if (op + last > cap) FAIL;
        memcpy(out + op, src + anchor, (size_t)last); op += last;
    }
#undef FAIL
    free(table);
    return op;
}

/* ---- QOI2AVG ------------------------------------------------------------------------------------------------------------------- */

static int refused(const uint8_t* src, int w, int h, int channels, int colorspace)
{
    return !src || w <= 0 || h <= 0 || channels < 3 || channels > 4 || colorspace < 0 || colorspace > 2 ||
           (uint32_t)h >= (uint32_t)PIXELS_MAX / (uint32_t)w;
}

static int loco(int a, int b, int c)                                              /* left, up, up-left */
{
    const int mx = a > b ? a : b, mn = a > b ? b : a;
    if (c <= mn) return mx;
    if (c >= mx) return mn;
    return a + b - c;
}

typedef struct { uint8_t r, g, b, a; } Px;

static Px pixel_at(const uint8_t* src, long pitch, int channels, int x, int y)
{
    const uint8_t* p = src + (ptrdiff_t)pitch * y + (ptrdiff_t)x * channels;
    Px v = { p[0], p[1], p[2], channels == 4 ? p[3] : 255 };
    return v;
}

static uint32_t word_of(Px p) { return p.r | (uint32_t)p.g << 8 | (uint32_t)p.b << 16 | (uint32_t)p.a << 24; }

/* the stored file: header, ops, four 0xff.  par_bits / dpi_bits: the two floats' bit patterns. */
long qoixwref_encode_stored(const uint8_t* src, long pitch, int w, int h, int channels, int colorspace, uint32_t par_bits,
                            uint32_t dpi_bits, uint8_t* out, long cap)
{
    if (refused(src, w, h, channels, colorspace)) return -1;
    const long long need = (long long)w * h * (channels + 1) + HEADER + 4;
    if (cap < need) return -2;                                                    /* the reference's own max_size */
    long p = 0;
    const uint32_t head[3] = { 0x716F6978u, (uint32_t)w, (uint32_t)h };
    for (int k = 0; k < 3; ++k) for (int s = 24; s >= 0; s -= 8) out[p++] = (uint8_t)(head[k] >> s);
    out[p++] = 1; out[p++] = (uint8_t)channels; out[p++] = 8; out[p++] = (uint8_t)colorspace; out[p++] = 0;
    for (int s = 24; s >= 0; s -= 8) out[p++] = (uint8_t)(par_bits >> s);
    for (int s = 24; s >= 0; s -= 8) out[p++] = (uint8_t)(dpi_bits >> s);

    uint8_t lookup[1024]; uint32_t fifo[64]; uint32_t fifo_pos = 0;
    memset(lookup, 0, sizeof lookup); memset(fifo, 0, sizeof fifo);
    Px px = { 0, 0, 0, 255 };
    int run = 0;
    const long long last = (long long)w * h - 1;
    long long at = 0;
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x, ++at) {
        const Px left = px;
        px = pixel_at(src, pitch, channels, x, y);
        if (word_of(px) == word_of(left)) {
            ++run;
            if (run == 1024 || at == last) { --run; out[p++] = (uint8_t)(0xf8 | ((run >> 8) & 3)); out[p++] = (uint8_t)run; run = 0; }
            continue;
        }
        if (run > 0) {
            --run;
            if (run < 8) out[p++] = (uint8_t)(0xf0 | run);
            else { out[p++] = (uint8_t)(0xf8 | ((run >> 8) & 3)); out[p++] = (uint8_t)run; }
            run = 0;
        }
        const uint32_t v = word_of(px), hash = ((v * 2654435769u) >> 22) & 1023u;
        if (fifo[lookup[hash]] == v) { out[p++] = (uint8_t)(0x80 | lookup[hash]); continue; }
        lookup[hash] = (uint8_t)fifo_pos; fifo[fifo_pos] = v; fifo_pos = (fifo_pos + 1) & 63;
        const int8_t va = (int8_t)(px.a - left.a);
        if (va) {
            if (va >= -4 && va <= 3) out[p++] = (uint8_t)(0xe8 | (va + 4));
            else { out[p++] = 0xfe; out[p++] = px.r; out[p++] = px.g; out[p++] = px.b; out[p++] = px.a; continue; }
        }
        int rr = left.r, rg = left.g, rb = left.b;
        if (y > 0) {
            const Px up = pixel_at(src, pitch, channels, x, y - 1);
            if (x == 0) { rr = up.r; rg = up.g; rb = up.b; }
            else {
                const Px ul = pixel_at(src, pitch, channels, x - 1, y - 1);
                rr = loco(left.r, up.r, ul.r); rg = loco(left.g, up.g, ul.g); rb = loco(left.b, up.b, ul.b);
            }
        }
        const int8_t vg = (int8_t)(px.g - rg), vr = (int8_t)(px.r - rr - vg), vb = (int8_t)(px.b - rb - vg);
        if (vg >= -4 && vg < 0 && vr >= -1 && vr <= 2 && vb >= -1 && vb <= 2)
            out[p++] = (uint8_t)((vg + 4) << 4 | (vr + 1) << 2 | (vb + 1));
        else if (vg >= 0 && vg <= 3 && vr >= -2 && vr <= 1 && vb >= -2 && vb <= 1)
            out[p++] = (uint8_t)((vg + 4) << 4 | (vr + 2) << 2 | (vb + 2));
        else if (px.g == px.r && px.g == px.b) { out[p++] = 0xfc; out[p++] = px.g; }
        else if (vr >= -8 && vr <= 7 && vg >= -16 && vg <= 15 && vb >= -8 && vb <= 7) {
            out[p++] = (uint8_t)(0xc0 | (vg + 16)); out[p++] = (uint8_t)((vr + 8) << 4 | (vb + 8));
        } else if (vr >= -32 && vr <= 31 && vg >= -64 && vg <= 63 && vb >= -32 && vb <= 31) {
            const int dv = (vg + 64) << 12 | (vr + 32) << 6 | (vb + 32);
            out[p++] = (uint8_t)(0xe0 | ((dv >> 16) & 31)); out[p++] = (uint8_t)(dv >> 8); out[p++] = (uint8_t)dv;
        } else { out[p++] = 0xfd; out[p++] = px.r; out[p++] = px.g; out[p++] = px.b; }
    }
    for (int k = 0; k < 4; ++k) out[p++] = 0xff;
    return p;
}

long long qoixwref_bound(int w, int h, int channels, int colorspace)
{
    static const uint8_t some = 0;
    if (refused(&some, w, h, channels, colorspace)) return -1;
    const long long datalen_max = (long long)w * h * (channels + 1) + 4;
    return HEADER + 4 + datalen_max + datalen_max / 255 + 16;
}

/* qoix_lz4_encode: mode 0 the reference's choice, mode 1 always stored.  *diff (may be NULL) receives lz4Size + 4 - datalen. */
long qoixwref_encode(const uint8_t* src, long pitch, int w, int h, int channels, int colorspace, uint32_t par_bits, uint32_t dpi_bits,
                     int mode, uint8_t* out, long cap, long* diff)
{
    if (refused(src, w, h, channels, colorspace)) return -1;
    const long long bound = qoixwref_bound(w, h, channels, colorspace);
    if (bound > 0x7fffffffLL) return -1;                                          /* the GPU encoder's deviation 2 */
    if (cap < bound) return -2;
    uint8_t* stored = (uint8_t*)malloc((size_t)bound);
    if (!stored) return -2;
    const long n = qoixwref_encode_stored(src, pitch, w, h, channels, colorspace, par_bits, dpi_bits, stored, (long)bound);
    if (n < 0) { free(stored); return n; }
    const long datalen = n - HEADER;
    long result = n;
    const long lz = qoixwref_lz4_compress(stored + HEADER, datalen, out + HEADER + 4, cap - HEADER - 4);
    if (lz < 0) { free(stored); return -2; }
    if (diff) *diff = lz + 4 - datalen;
    if (mode == 0 && lz + 4 < datalen) {
        memcpy(out, stored, HEADER);
        out[16] = 1;
        out[25] = (uint8_t)(datalen >> 24); out[26] = (uint8_t)(datalen >> 16); out[27] = (uint8_t)(datalen >> 8); out[28] = (uint8_t)datalen;
        result = HEADER + 4 + lz;
    } else memcpy(out, stored, (size_t)n);
    free(stored);
    return result;
}
