/* jpeg_write_ref.c -- a serial baseline JPEG writer, the test suite's oracle for the GPU encoder (gamut_amd/csrc/jpeg_encode.hip).
 *
 * Written from the JPEG standard (ITU T.81: Annex K.1 quantisation tables, K.3 Huffman tables, F.1.2 entropy coding) and the
 * behaviour the project reproduces: AAN float DCT, three components for every input, 4:2:0 at quality <= 90,
 * edge clamping per MCU, EOB / ZRL rules, 7 fill bits, 0xFF stuffing.  Built by the tests with
 *   gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC
 * so every float operation rounds on its own (x86-64 SSE).  tests/jpeg_encode_ref.py is the independent numpy reading; the CPU
 * suite checks that the two agree byte for byte.
 *
 * long jwr_encode(data, w, h, comp, pitch, quality, out, cap): the stream length, 0 when refused, -1 when cap is too small.
 */
#include <stdint.h>
#include <string.h>

static const uint8_t kZigzag[64] = {  /* natural (row-major) index -> zig-zag position */
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63 };

/* T.81 Table K.1 / K.2, natural order */
static const int kLumaQ[64] = { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
static const int kChromaQ[64] = { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };

/* T.81 Tables K.3-K.6 (DC) and K.5/K.6 (AC): BITS (codes per length 1..16) and HUFFVAL */
static const uint8_t kDcLumaBits[16] = { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 };
static const uint8_t kDcChromaBits[16] = { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 };
static const uint8_t kDcVals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
static const uint8_t kAcLumaBits[16] = { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d };
static const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };
static const uint8_t kAcChromaBits[16] = { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 };
static const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };

typedef struct { uint16_t code[256]; uint8_t len[256]; } Huff;   /* indexed by symbol; unused symbols have length 0 */

static void huff_build(Huff* t, const uint8_t* bits, const uint8_t* vals)  /* T.81 C.2 canonical codes */
{
    int k = 0, l, i;
    unsigned code = 0;
    memset(t, 0, sizeof *t);
    for (l = 1; l <= 16; ++l) {
        for (i = 0; i < bits[l - 1]; ++i, ++k) { t->code[vals[k]] = (uint16_t)code++; t->len[vals[k]] = (uint8_t)l; }
        code <<= 1;
    }
}

typedef struct { uint8_t* out; long cap, n; int overflow; uint32_t acc; int nacc; } Writer;

static void put(Writer* w, int b)
{
    if (w->n < w->cap) w->out[w->n] = (uint8_t)b; else w->overflow = 1;
    ++w->n;
}
static void put_bits(Writer* w, uint32_t v, int n)   /* MSB first; every 0xFF data byte is followed by 0x00 */
{
    int i;
    for (i = n - 1; i >= 0; --i) {
        w->acc = (w->acc << 1) | ((v >> i) & 1u);
        if (++w->nacc == 8) { put(w, (int)w->acc); if (w->acc == 0xFF) put(w, 0); w->acc = 0; w->nacc = 0; }
    }
}

static void dct8(float* d, int s)   /* AAN forward DCT of d[0], d[s], ..., d[7s]; every statement on its own, no contraction */
{
    float d0 = d[0], d1 = d[s], d2 = d[2 * s], d3 = d[3 * s], d4 = d[4 * s], d5 = d[5 * s], d6 = d[6 * s], d7 = d[7 * s];
    float t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    float t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    float z1, z2, z3, z4, z5, z11, z13;
    d0 = t10 + t11;
    d4 = t10 - t11;
    z1 = (t12 + t13) * 0.707106781f;
    d2 = t13 + z1;
    d6 = t13 - z1;
    t10 = t4 + t5;
    t11 = t5 + t6;
    t12 = t6 + t7;
    z5 = (t10 - t12) * 0.382683433f;
    z2 = t10 * 0.541196100f + z5;
    z4 = t12 * 1.306562965f + z5;
    z3 = t11 * 0.707106781f;
    z11 = t7 + z3;
    z13 = t7 - z3;
    d[5 * s] = z13 + z2;
    d[3 * s] = z13 - z2;
    d[s] = z11 + z4;
    d[7 * s] = z11 - z4;
    d[0] = d0; d[2 * s] = d2; d[4 * s] = d4; d[6 * s] = d6;
}

static int cat_of(int v) { int a = v < 0 ? -v : v, n = 1; while (a >>= 1) ++n; return n; }   /* 1 for 0 too */

/* one 8x8 block at p (row stride s floats); returns its DC */
static int block(Writer* w, float* p, int s, const float* fdtbl, int dc_prev, const Huff* dc, const Huff* ac)
{
    int du[64], i, k, diff, end, r, c;
    for (r = 0; r < 8; ++r) dct8(p + r * s, 1);
    for (c = 0; c < 8; ++c) dct8(p + c, s);
    for (r = 0, k = 0; r < 8; ++r)
        for (c = 0; c < 8; ++c, ++k) {
            float v = p[r * s + c] * fdtbl[k];
            du[kZigzag[k]] = (int)(v < 0 ? v - 0.5f : v + 0.5f);
        }
    diff = du[0] - dc_prev;
    if (diff == 0) put_bits(w, dc->code[0], dc->len[0]);
    else {
        int n = cat_of(diff);
        put_bits(w, dc->code[n], dc->len[n]);
        put_bits(w, (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << n) - 1)), n);
    }
    for (end = 63; end > 0 && du[end] == 0; --end) {}
    if (end == 0) { put_bits(w, ac->code[0], ac->len[0]); return du[0]; }
    for (i = 1; i <= end; ++i) {
        int start = i, zeros, n;
        while (du[i] == 0) ++i;
        zeros = i - start;
        for (; zeros >= 16; zeros -= 16) put_bits(w, ac->code[0xF0], ac->len[0xF0]);
        n = cat_of(du[i]);
        put_bits(w, ac->code[((zeros << 4) + n) & 255], ac->len[((zeros << 4) + n) & 255]);
        put_bits(w, (uint32_t)((du[i] < 0 ? du[i] - 1 : du[i]) & ((1 << n) - 1)), n);
    }
    if (end != 63) put_bits(w, ac->code[0], ac->len[0]);
    return du[0];
}

static void load_yuv(const uint8_t* data, long pitch, int width, int height, int comp, int x0, int y0, int size, float* Y, float* U, float* V)
{
    int r, c, og = comp > 2 ? 1 : 0, ob = comp > 2 ? 2 : 0;
    for (r = 0; r < size; ++r)
        for (c = 0; c < size; ++c) {
            int yy = y0 + r < height ? y0 + r : height - 1, xx = x0 + c < width ? x0 + c : width - 1;
            const uint8_t* q = data + (long)yy * pitch + (long)xx * comp;
            float R = q[0], G = q[og], B = q[ob];
            Y[r * size + c] = 0.29900f * R + 0.58700f * G + 0.11400f * B - 128;
            U[r * size + c] = -0.16874f * R - 0.33126f * G + 0.50000f * B;
            V[r * size + c] = 0.50000f * R - 0.41869f * G - 0.08131f * B;
        }
}

long jwr_encode(const uint8_t* data, int width, int height, int comp, long pitch, int quality, uint8_t* out, long cap)
{
    static const float aasf[8] = { 1.0f * 2.828427125f, 1.387039845f * 2.828427125f, 1.306562965f * 2.828427125f,
        1.175875602f * 2.828427125f, 1.0f * 2.828427125f, 0.785694958f * 2.828427125f, 0.541196100f * 2.828427125f,
        0.275899379f * 2.828427125f };
    uint8_t qy[64], quv[64];
    float fy[64], fuv[64];
    Huff hdc[2], hac[2];
    Writer w;
    int sub, i, k, r, c, x, y, dcy = 0, dcu = 0, dcv = 0;
    if (!data || width < 1 || height < 1 || width > 65535 || height > 65535 || comp < 1 || comp > 4) return 0;
    quality = quality ? quality : 90;
    sub = quality <= 90;
    quality = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    quality = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (i = 0; i < 64; ++i) {
        int a = (kLumaQ[i] * quality + 50) / 100, b = (kChromaQ[i] * quality + 50) / 100;
        qy[kZigzag[i]] = (uint8_t)(a < 1 ? 1 : a > 255 ? 255 : a);
        quv[kZigzag[i]] = (uint8_t)(b < 1 ? 1 : b > 255 ? 255 : b);
    }
    for (r = 0, k = 0; r < 8; ++r)
        for (c = 0; c < 8; ++c, ++k) {
            fy[k] = 1 / ((float)qy[kZigzag[k]] * aasf[r] * aasf[c]);
            fuv[k] = 1 / ((float)quv[kZigzag[k]] * aasf[r] * aasf[c]);
        }
    huff_build(&hdc[0], kDcLumaBits, kDcVals); huff_build(&hdc[1], kDcChromaBits, kDcVals);
    huff_build(&hac[0], kAcLumaBits, kAcLumaVals); huff_build(&hac[1], kAcChromaBits, kAcChromaVals);

    memset(&w, 0, sizeof w); w.out = out; w.cap = cap;
    {   /* SOI, APP0 JFIF 1.1 (no units, 1:1), DQT (both tables), SOF0, DHT (four tables), SOS */
        static const uint8_t app0[20] = { 0xFF, 0xD8, 0xFF, 0xE0, 0, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
        const uint8_t* bits[4] = { kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits };
        const uint8_t* vals[4] = { kDcVals, kAcLumaVals, kDcVals, kAcChromaVals };
        const int nv[4] = { 12, 162, 12, 162 }, cls[4] = { 0x00, 0x10, 0x01, 0x11 };
        for (i = 0; i < 20; ++i) put(&w, app0[i]);
        put(&w, 0xFF); put(&w, 0xDB); put(&w, 0); put(&w, 0x84);
        put(&w, 0); for (i = 0; i < 64; ++i) put(&w, qy[i]);
        put(&w, 1); for (i = 0; i < 64; ++i) put(&w, quv[i]);
        put(&w, 0xFF); put(&w, 0xC0); put(&w, 0); put(&w, 0x11); put(&w, 8);
        put(&w, (height >> 8) & 255); put(&w, height & 255); put(&w, (width >> 8) & 255); put(&w, width & 255);
        put(&w, 3); put(&w, 1); put(&w, sub ? 0x22 : 0x11); put(&w, 0); put(&w, 2); put(&w, 0x11); put(&w, 1); put(&w, 3); put(&w, 0x11); put(&w, 1);
        put(&w, 0xFF); put(&w, 0xC4); put(&w, 0x01); put(&w, 0xA2);
        for (k = 0; k < 4; ++k) {
            put(&w, cls[k]);
            for (i = 0; i < 16; ++i) put(&w, bits[k][i]);
            for (i = 0; i < nv[k]; ++i) put(&w, vals[k][i]);
        }
        {
            static const uint8_t sos[14] = { 0xFF, 0xDA, 0, 0x0C, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0 };
            for (i = 0; i < 14; ++i) put(&w, sos[i]);
        }
    }
    if (sub) {
        float Y[256], U[256], V[256], su[64], sv[64];
        for (y = 0; y < height; y += 16)
            for (x = 0; x < width; x += 16) {
                load_yuv(data, pitch, width, height, comp, x, y, 16, Y, U, V);
                dcy = block(&w, Y, 16, fy, dcy, &hdc[0], &hac[0]);
                dcy = block(&w, Y + 8, 16, fy, dcy, &hdc[0], &hac[0]);
                dcy = block(&w, Y + 128, 16, fy, dcy, &hdc[0], &hac[0]);
                dcy = block(&w, Y + 136, 16, fy, dcy, &hdc[0], &hac[0]);
                for (r = 0; r < 8; ++r)
                    for (c = 0; c < 8; ++c) {
                        int j = r * 32 + c * 2;
                        su[r * 8 + c] = (U[j] + U[j + 1] + U[j + 16] + U[j + 17]) * 0.25f;
                        sv[r * 8 + c] = (V[j] + V[j + 1] + V[j + 16] + V[j + 17]) * 0.25f;
                    }
                dcu = block(&w, su, 8, fuv, dcu, &hdc[1], &hac[1]);
                dcv = block(&w, sv, 8, fuv, dcv, &hdc[1], &hac[1]);
            }
    } else {
        float Y[64], U[64], V[64];
        for (y = 0; y < height; y += 8)
            for (x = 0; x < width; x += 8) {
                load_yuv(data, pitch, width, height, comp, x, y, 8, Y, U, V);
                dcy = block(&w, Y, 8, fy, dcy, &hdc[0], &hac[0]);
                dcu = block(&w, U, 8, fuv, dcu, &hdc[1], &hac[1]);
                dcv = block(&w, V, 8, fuv, dcv, &hdc[1], &hac[1]);
            }
    }
    put_bits(&w, 0x7F, 7);                     /* fill: a partial last byte is completed with 1-bits, the rest dropped */
    put(&w, 0xFF); put(&w, 0xD9);
    return w.overflow ? -1 : w.n;
}
