/* qoiplane_write_ref.c -- qoiplane_encode (source/gamut/codecs/qoiplane.d:109-365) restated serially in C for the tests: the 25 header
 * bytes, the ops on nibble boundaries and the closing nibbles of an 8-bit image with 1 or 2 channels, one pixel after the other with the
 * encoder's own state (px, px_ref, run, the nibble cursor).  The LZ4 step of qoix_lz4_encode is tests/c/qoix_write_ref.c's.
 *
 * qoipwref_bound is the size a caller of the GPU encoder must provide: the stored stream behind the header has at most
 * (w * h * n + 10) / 2 bytes, n = 3 nibbles a pixel for 1 channel and 6 for 2 (every pixel its worst op, nine closing nibbles, one more
 * to end on a byte), and the bound is 29 + that + that / 255 + 16.  The reference's own buffer, (w * h * n + 1) / 2 + 29, is one byte
 * short when w * h * n is even and every pixel takes its worst op; qoipwref_reference_alloc returns it so that a test can show that. */
#include <stdint.h>
#include <string.h>

typedef struct { uint8_t* bytes; long cap; long p; int hi; int overflow; } out_t;

static void put_nibble(out_t* o, unsigned nibble)
{
    if (o->p >= o->cap) { o->overflow = 1; return; }
    if (o->hi) o->bytes[o->p] = (uint8_t)(nibble << 4);
    else o->bytes[o->p++] |= (uint8_t)nibble;
    o->hi = !o->hi;
}

static void put_byte(out_t* o, unsigned b)
{
    put_nibble(o, b >> 4);
    put_nibble(o, b & 15u);
}

static void put_run(out_t* o, int* run)
{
    if (*run <= 3) put_nibble(o, 0xcu | (unsigned)(*run - 1));
    else { put_nibble(o, 0xf); put_byte(o, (unsigned)(*run - 4)); }
    *run = 0;
}

static void put_be32(out_t* o, uint32_t v)
{
    put_byte(o, v >> 24); put_byte(o, (v >> 16) & 255u); put_byte(o, (v >> 8) & 255u); put_byte(o, v & 255u);
}

long long qoipwref_datalen_max(int w, int h, int channels)
{
    return ((long long)w * h * (channels == 1 ? 3 : 6) + 10) / 2;
}

long long qoipwref_reference_alloc(int w, int h, int channels)
{
    return ((long long)w * h * (channels == 1 ? 3 : 6) + 1) / 2 + 25 + 4;
}

long long qoipwref_bound(int w, int h, int channels, int colorspace)
{
    if (w <= 0 || h <= 0 || (channels != 1 && channels != 2) || colorspace < 0 || colorspace > 2) return -1;
    if ((uint32_t)h >= 400000000u / (uint32_t)w) return -1;
    if ((long long)w * h * 6 > 2147483647LL && channels == 2) return -1;
    long long d = qoipwref_datalen_max(w, h, channels);
    long long b = 25 + 4 + d + d / 255 + 16;
    return b > 2147483647LL ? -1 : b;
}

/* data: row y begins at data + y * pitch (pitch may be negative or padded).  Returns the stored file's length, -1 for a refused
 * description, -2 when `cap` bytes do not hold the file. */
long qoipwref_encode(const uint8_t* data, long pitch, int w, int h, int channels, int colorspace, uint32_t par_bits, uint32_t dpi_bits,
                     uint8_t* out, long cap)
{
    if (qoipwref_bound(w, h, channels, colorspace) < 0) return -1;
    out_t o = { out, cap, 0, 1, 0 };
    put_be32(&o, 0x716F6978u);
    put_be32(&o, (uint32_t)w);
    put_be32(&o, (uint32_t)h);
    put_byte(&o, 1);
    put_byte(&o, (unsigned)channels);
    put_byte(&o, 8);
    put_byte(&o, (unsigned)colorspace);
    put_byte(&o, 0);
    put_be32(&o, par_bits);
    put_be32(&o, dpi_bits);

    uint8_t px_l = 0, px_a = 255, ref_l, ref_a;
    int run = 0;
    long encoded = 0, num_pixels = (long)w * h;
    for (int y = 0; y < h; ++y) {
        const uint8_t* line = data + pitch * y;
        const uint8_t* above = y > 0 ? data + pitch * (y - 1) : 0;
        for (int x = 0; x < w; ++x, ++encoded) {
            ref_l = px_l; ref_a = px_a;
            px_l = line[x * channels];
            if (channels == 2) px_a = line[x * channels + 1];
            if (px_l == ref_l && px_a == ref_a) {
                ++run;
                if (run == 258 || encoded + 1 == num_pixels) put_run(&o, &run);
                continue;
            }
            if (run > 0) put_run(&o, &run);
            int8_t va = (int8_t)(uint8_t)(px_a - ref_a);
            if (va != 0 && (va < -7 || va > 7)) {
                put_nibble(&o, 0xb); put_nibble(&o, 0);
                put_byte(&o, px_l); put_byte(&o, px_a);
                continue;
            }
            if (va != 0) { put_nibble(&o, 0xb); put_nibble(&o, (unsigned)(va + 8)); }
            uint8_t top = above ? above[x * channels] : ref_l;
            uint8_t avg = (uint8_t)((top + ref_l + 1) / 2);
            int8_t d = (int8_t)(uint8_t)(px_l - avg);
            if (d >= -4 && d <= 3) put_nibble(&o, (unsigned)(d + 4));
            else if (d >= -16 && d <= 15) put_byte(&o, 0x80u | (unsigned)(d + 16));
            else { put_nibble(&o, 0xa); put_byte(&o, px_l); }
        }
    }
    for (int k = 0; k < 9; ++k) put_nibble(&o, 0xf);
    if (!o.hi) put_nibble(&o, 0xf);
    return o.overflow ? -2 : o.p;
}
