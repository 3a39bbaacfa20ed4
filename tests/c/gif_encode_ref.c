/* gif_encode_ref.c -- a serial restatement of the GIF writer the GPU encoder must match byte for byte: saveGIF (plugins/gif.d:105-147)
 * over msf_gif (codecs/msf_gif.d: begin, one frame per layer, end).  Written from the reference's behaviour for the tests; besides the
 * file it reports, per frame, what the named cases of tests/gif_encode_cases.py assert about themselves.
 *
 * The cooking is restated twice, as the reference has it: the 4-pixel body in 16-bit lanes (wrapping multiply, saturating add, the
 * blue lane shifted out of a 32-bit word that holds red below it) and the scalar tail in ints with a clamp.
 *
 * report: 8 int32 per frame -- depth, used colours, table bits, table resets, sub-blocks written (the terminator not counted),
 * last sub-block (1: a partial one; 2: none, nothing was left after a rollover; 3: the flush at the end wrote a sub-block of exactly
 * 255 bytes), has-transparent, frames-compatible. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int bit_log(int i) { int n = 0; if (i <= 0) return 1; while (i) { ++n; i >>= 1; } return n; }   /* msf_bit_log: 1 for 0 */
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static const int RD[17] = { 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5 };
static const int GD[17] = { 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6 };
static const int BD[17] = { 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5 };
static const int DITHER[16] = { 0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5 };

typedef struct { uint32_t* px; int depth, count, rb, gb, bb; } Cooked;

static uint16_t adds16(uint16_t a, uint16_t b) { uint32_t s = (uint32_t)a + b; return (uint16_t)(s > 65535u ? 65535u : s); }

/* -> the depth settled on; used[] and *count as the last pass left them */
static int cook(Cooked* fr, const uint8_t* raw, uint8_t* used, int w, int h, long pitch, int depth, int athr)
{
    int count;
    do {
        const int rb = RD[depth], gb = GD[depth], bb = BD[depth];
        const int palette = (1 << (rb + gb + bb)) + 1;
        const int rdiff = (1 << (8 - rb)) - 1, gdiff = (1 << (8 - gb)) - 1, bdiff = (1 << (8 - bb)) - 1;
        const short rmul = (short)((255.0f - rdiff) / 255.0f * 257);
        const short gmul = (short)((255.0f - gdiff) / 255.0f * 257);
        const short bmul = (short)((255.0f - bdiff) / 255.0f * 257);
        const int gmask = ((1 << gb) - 1) << rb, bmask = ((1 << bb) - 1) << rb << gb;
        memset(used, 0, (size_t)palette);
        for (int y = 0; y < h; ++y) {
            int x = 0;
            for (; x < w - 3; x += 4) {                                  /* the vector body, one 32-bit lane at a time */
                for (int l = 0; l < 4; ++l) {
                    const uint8_t* p = raw + y * pitch + (long)(x + l) * 4;
                    const uint32_t k = (uint32_t)DITHER[(y & 3) * 4 + l] << 12;
                    const uint32_t k2 = (k >> rb) | ((k >> bb) << 16);
                    const uint16_t r1 = (uint16_t)(p[0] * (uint16_t)rmul), b1 = (uint16_t)(p[2] * (uint16_t)bmul);
                    const uint32_t rb2 = (uint32_t)adds16(r1, (uint16_t)k2) | (uint32_t)adds16(b1, (uint16_t)(k2 >> 16)) << 16;
                    const uint32_t r3 = (rb2 & 0xFFFFu) >> (16 - rb);
                    const uint32_t b3 = (rb2 >> (32 - rb - gb - bb)) & (uint32_t)bmask;
                    const uint32_t kg = k >> gb;
                    const uint32_t g2 = (uint32_t)adds16((uint16_t)(p[1] * (uint16_t)gmul), (uint16_t)kg) | (uint32_t)adds16(0, (uint16_t)(kg >> 16)) << 16;
                    const uint32_t g3 = (g2 >> (16 - rb - gb)) & (uint32_t)gmask;
                    uint32_t o = r3 | g3 | b3;
                    if ((int)p[3] < athr) o = (uint32_t)(palette - 1);
                    fr->px[(size_t)y * w + x + l] = o;
                }
            }
            for (; x < w; ++x) {                                         /* the scalar tail */
                const uint8_t* p = raw + y * pitch + (long)x * 4;
                if (p[3] < athr) { fr->px[(size_t)y * w + x] = (uint32_t)(palette - 1); continue; }
                const int k3 = DITHER[(y & 3) * 4 + (x & 3)] << 12;
                fr->px[(size_t)y * w + x] = (uint32_t)(
                    ((imin(65535, p[2] * bmul + (k3 >> bb)) >> (16 - rb - gb - bb)) & bmask) |
                    ((imin(65535, p[1] * gmul + (k3 >> gb)) >> (16 - rb - gb)) & gmask) |
                    (imin(65535, p[0] * rmul + (k3 >> rb)) >> (16 - rb)));
            }
        }
        for (long i = 0; i < (long)w * h; ++i) used[fr->px[i]] = 1;
        count = 0;
        for (int j = 0; j < palette - 1; ++j) count += used[j];
    } while (count >= 256 && --depth);
    fr->depth = depth; fr->count = count; fr->rb = RD[depth]; fr->gb = GD[depth]; fr->bb = BD[depth];
    return depth;
}

typedef struct { uint8_t* head; uint32_t bits; int blocks; } Writer;

static void put_code(Writer* wr, int len, uint32_t code)
{
    const int idx = (int)(wr->bits / 8), bit = (int)(wr->bits % 8);
    wr->head[idx + 0] |= (uint8_t)(code << bit);
    wr->head[idx + 1] |= (uint8_t)(code >> (8 - bit));
    wr->head[idx + 2] |= (uint8_t)(code >> (16 - bit));
    wr->bits += (uint32_t)len;
    if (wr->bits >= 256 * 8) {
        wr->bits -= 255 * 8;
        wr->head += 256;
        wr->head[2] = wr->head[1]; wr->head[1] = wr->head[0]; wr->head[0] = 255;
        memset(wr->head + 4, 0, 256);
        wr->blocks++;
    }
}

/* one frame block -> bytes written; *has_t: the frame has transparent pixels */
static long compress(uint8_t* out, int w, int h, int centis, const Cooked* cur, const Cooked* prev, const uint8_t* used, int16_t* lzw, int32_t* rep, int* has_t)
{
    uint8_t* const out0 = out;
    const int total = cur->rb + cur->gb + cur->bb, tlb_size = (1 << total) + 1;
    static uint8_t tlb[(1 << 16) + 1];
    uint8_t table[256 * 3];
    memset(table, 0, sizeof table);
    int idx = 1;
    tlb[tlb_size - 1] = 0;
    for (int i = 0; i < tlb_size - 1; ++i) {
        if (!used[i]) continue;
        tlb[i] = (uint8_t)idx;
        int r = i & ((1 << cur->rb) - 1), g = (i >> cur->rb) & ((1 << cur->gb) - 1), b = i >> (cur->rb + cur->gb);
        r <<= 8 - cur->rb; g <<= 8 - cur->gb; b <<= 8 - cur->bb;
        table[idx * 3 + 0] = (uint8_t)(r | r >> cur->rb | r >> (cur->rb * 2) | r >> (cur->rb * 3));
        table[idx * 3 + 1] = (uint8_t)(g | g >> cur->gb | g >> (cur->gb * 2) | g >> (cur->gb * 3));
        table[idx * 3 + 2] = (uint8_t)(b | b >> cur->bb | b >> (cur->bb * 2) | b >> (cur->bb * 3));
        ++idx;
    }
    *has_t = used[tlb_size - 1];
    const int table_bits = imax(2, bit_log(idx - 1)), table_size = 1 << table_bits;
    const int same = cur->rb == prev->rb && cur->gb == prev->gb && cur->bb == prev->bb;
    const int compatible = same && !*has_t;
    uint8_t hdr[18] = { 0x21, 0xF9, 0x04, 0x05, 0, 0, 0, 0, 0x2C, 0, 0, 0, 0, 0, 0, 0, 0, 0x80 };
    hdr[4] = (uint8_t)centis; hdr[5] = (uint8_t)(centis >> 8);
    hdr[13] = (uint8_t)w; hdr[14] = (uint8_t)(w >> 8); hdr[15] = (uint8_t)h; hdr[16] = (uint8_t)(h >> 8);
    hdr[17] |= (uint8_t)(table_bits - 1);
    memcpy(out, hdr, 18); out += 18;
    memcpy(out, table, (size_t)table_size * 3); out += table_size * 3;
    *out++ = (uint8_t)table_bits;
    memset(out, 0, 260);
    out[0] = 255;
    Writer wr = { out, 8, 0 };
    int resets = 0;
    const int stride = idx;
    memset(lzw, 0xFF, (size_t)4096 * stride * sizeof(int16_t));
    int len = table_size + 2;
    put_code(&wr, bit_log(len - 1), (uint32_t)table_size);
    int last = compatible && cur->px[0] == prev->px[0] ? 0 : tlb[cur->px[0]];
    for (long i = 1; i < (long)w * h; ++i) {
        const int color = compatible && cur->px[i] == prev->px[i] ? 0 : tlb[cur->px[i]];
        const int code = lzw[last * stride + color];
        if (code < 0) {
            const int code_bits = bit_log(len - 1);
            put_code(&wr, code_bits, (uint32_t)last);
            if (len > 4095) {
                put_code(&wr, code_bits, (uint32_t)table_size);
                memset(lzw, 0xFF, (size_t)4096 * stride * sizeof(int16_t));
                len = table_size + 2; ++resets;
            } else {
                lzw[last * stride + color] = (int16_t)len;
                ++len;
            }
            last = color;
        } else last = code;
    }
    put_code(&wr, imin(12, bit_log(len - 1)), (uint32_t)last);
    put_code(&wr, imin(12, bit_log(len)), (uint32_t)(table_size + 1));
    int last_kind = 2;                                               /* blockBits == 8: nothing is left after a rollover */
    if (wr.bits > 8) {
        const int bytes = (int)((wr.bits + 7) / 8);
        wr.head[0] = (uint8_t)(bytes - 1);
        wr.head += bytes;
        wr.blocks++;
        last_kind = bytes - 1 == 255 ? 3 : 1;
    }
    *wr.head++ = 0;
    rep[0] = cur->depth; rep[1] = cur->count; rep[2] = table_bits; rep[3] = resets; rep[4] = wr.blocks; rep[5] = last_kind;
    rep[6] = *has_t; rep[7] = compatible;
    return (long)(wr.head - out0);
}

/* pixels: `frames` layers, layer l at raw + l * layer_off, rows `pitch` apart.  out: at least 32 + frames * (32 + 768 + w * h * 3 / 2 + 256) + 1 + 512
 * bytes.  report: 8 int32 per frame (may be NULL).  -> the file's length, 0 when refused */
long gifencref_encode(const uint8_t* raw, long pitch, long layer_off, int w, int h, int frames, int centis, int max_depth, int athr,
                      uint8_t* out, int32_t* report)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || frames < 1 || (long long)w * h * 4 > 0x7fffffffLL) return 0;
    static const uint8_t head[32] = { 'G', 'I', 'F', '8', '9', 'a', 0, 0, 0, 0, 0x70, 0, 0, 0x21, 0xFF, 0x0B,
                                      'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 0x03, 0x01, 0, 0, 0 };
    uint8_t* used = (uint8_t*)malloc((1 << 16) + 1);
    int16_t* lzw = (int16_t*)malloc((size_t)4096 * 256 * 2);
    Cooked prev = { (uint32_t*)malloc((size_t)w * h * 4), 0, 0, 0, 0, 0 }, cur = { (uint32_t*)malloc((size_t)w * h * 4), 0, 0, 0, 0, 0 };
    int32_t dummy[8];
    memcpy(out, head, 32);
    out[6] = (uint8_t)w; out[7] = (uint8_t)(w >> 8); out[8] = (uint8_t)h; out[9] = (uint8_t)(h >> 8);
    long pos = 32, prev_block = -1;
    max_depth = imax(1, imin(16, max_depth));
    for (int f = 0; f < frames; ++f) {
        cook(&cur, raw + f * layer_off, used, w, h, pitch, imin(max_depth, prev.depth + 160 / imax(1, prev.count)), athr);
        int has_t = 0;
        const long n = compress(out + pos, w, h, centis, &cur, &prev, used, lzw, report ? report + 8 * f : dummy, &has_t);
        if (has_t && f > 0) out[prev_block + 3] = 0x09;
        prev_block = pos; pos += n;
        Cooked t = prev; prev = cur; cur = t;
    }
    out[pos++] = 0x3B;
    free(used); free(lzw); free(prev.px); free(cur.px);
    return pos;
}

/* the cooked value of one pixel by the vector body's arithmetic (lane = x & 3) and by the scalar tail's, for the equivalence test */
void gifencref_cook_both(const uint8_t* px, int x, int y, int depth, int athr, uint32_t* vec, uint32_t* scalar)
{
    const int rb = RD[depth], gb = GD[depth], bb = BD[depth];
    const int rdiff = (1 << (8 - rb)) - 1, gdiff = (1 << (8 - gb)) - 1, bdiff = (1 << (8 - bb)) - 1;
    const short rmul = (short)((255.0f - rdiff) / 255.0f * 257), gmul = (short)((255.0f - gdiff) / 255.0f * 257), bmul = (short)((255.0f - bdiff) / 255.0f * 257);
    const int gmask = ((1 << gb) - 1) << rb, bmask = ((1 << bb) - 1) << rb << gb;
    const uint32_t transparent = 1u << (rb + gb + bb);
    const uint32_t k = (uint32_t)DITHER[(y & 3) * 4 + (x & 3)] << 12;
    const uint32_t k2 = (k >> rb) | ((k >> bb) << 16);
    const uint32_t rb2 = (uint32_t)adds16((uint16_t)(px[0] * (uint16_t)rmul), (uint16_t)k2) | (uint32_t)adds16((uint16_t)(px[2] * (uint16_t)bmul), (uint16_t)(k2 >> 16)) << 16;
    const uint32_t g2 = (uint32_t)adds16((uint16_t)(px[1] * (uint16_t)gmul), (uint16_t)(k >> gb));
    *vec = ((rb2 & 0xFFFFu) >> (16 - rb)) | ((g2 >> (16 - rb - gb)) & (uint32_t)gmask) | ((rb2 >> (32 - rb - gb - bb)) & (uint32_t)bmask);
    if ((int)px[3] < athr) *vec = transparent;
    const int k3 = (int)k;
    *scalar = px[3] < athr ? transparent : (uint32_t)(
        ((imin(65535, px[2] * bmul + (k3 >> bb)) >> (16 - rb - gb - bb)) & bmask) |
        ((imin(65535, px[1] * gmul + (k3 >> gb)) >> (16 - rb - gb)) & gmask) |
        (imin(65535, px[0] * rmul + (k3 >> rb)) >> (16 - rb)));
}
