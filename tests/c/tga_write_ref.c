/* tga_write_ref.c -- TGAEncoder (source/gamut/codecs/tga.d:57-281) as saveTGA drives it (plugins/tga.d:128-150), restated serially:
 * the header of initialize, then encodeScanline for y = height - 1 down to 0 -- convert to 3 / 4 channels, swap R and B, the similar
 * mask, the backward walk that decides the opcodes with the reference's own float comparison, the forward cursor walk that writes
 * them.  The oracle of the GPU encoder, and the host-core yardstick of tools/tga_encode_bench.py.
 *
 * comp is the SOURCE's channel count (1 l8, 2 la8, 3 rgb8, 4 rgba8); pitch may be negative.  Returns the file's length, -1 when the
 * reference refuses (a dimension above 65535, another pixel type), -2 when `cap` is too small or memory runs out.  A width or height
 * of 0 is encoded as the reference encodes it (a header and nothing else). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { uint8_t r, g, b, a; } Color;

long tgawref_encode(const uint8_t* src, long pitch, int width, int height, int comp, int enableRLE, uint8_t* out, long cap)
{
    int channels;
    long pos = 0;
    /* initialize :77-139 */
    if (width > 65535 || height > 65535 || width < 0 || height < 0) return -1;
    if (comp == 1 || comp == 3) channels = 3;
    else if (comp == 2 || comp == 4) channels = 4;
    else return -1;
    uint8_t* scanSpace = (uint8_t*)malloc((size_t)width * channels + (size_t)width * 2 + 1);
    if (!scanSpace) return -2;
    int8_t* similarMask = (int8_t*)(scanSpace + (size_t)width * channels);
    int8_t* opcode = similarMask + width;
    uint8_t header[18];
    memset(header, 0, 18);
    header[2] = enableRLE ? 10 : 2;
    header[12] = width & 0xff;
    header[13] = (width & 0xff00) >> 8;
    header[14] = height & 0xff;
    header[15] = (height & 0xff00) >> 8;
    header[16] = (uint8_t)(channels * 8);
    header[17] = 0;
    if (cap < 18) { free(scanSpace); return -2; }
    memcpy(out, header, 18); pos = 18;

#define WRITE(ptr, n) do { if (pos + (long)(n) > cap) { free(scanSpace); return -2; } memcpy(out + pos, (ptr), (n)); pos += (long)(n); } while (0)

    for (int y = height - 1; y >= 0; --y) {                                  /* plugins/tga.d:140-147 */
        const uint8_t* scanptr = src + (long)y * pitch;
        /* encodeScanline :152-280 */
        if (width == 0) continue;
        for (int x = 0; x < width; ++x) {                                    /* scanline_convert_*_to_rgb8 / rgba8 */
            if (comp == 1) { scanSpace[3 * x] = scanSpace[3 * x + 1] = scanSpace[3 * x + 2] = scanptr[x]; }
            else if (comp == 2) { scanSpace[4 * x] = scanSpace[4 * x + 1] = scanSpace[4 * x + 2] = scanptr[2 * x]; scanSpace[4 * x + 3] = scanptr[2 * x + 1]; }
            else memcpy(scanSpace + (size_t)channels * x, scanptr + (size_t)channels * x, (size_t)channels);
        }
        for (int x = 0; x < width; ++x) {                                    /* swap R and B :160-179 */
            uint8_t r = scanSpace[channels * x];
            uint8_t b = scanSpace[channels * x + 2];
            scanSpace[channels * x + 2] = r;
            scanSpace[channels * x] = b;
        }
        if (enableRLE) {
            {                                                                /* 1. :188-204 */
                Color last = { 0, 0, 0, 0 };
                for (int x = 0; x < width; ++x) {
                    Color c;
                    c.r = scanSpace[channels * x];
                    c.g = scanSpace[channels * x + 1];
                    c.b = scanSpace[channels * x + 2];
                    c.a = (channels == 3) ? 255 : scanSpace[x * 4 + 3];
                    int similar = c.r == last.r && c.g == last.g && c.b == last.b && c.a == last.a;
                    similarMask[x] = similar ? 1 : 0;
                    last = c;
                }
                similarMask[0] = 0;
            }
            int numSame = 0;                                                 /* 2. :206-244 */
            int numDifferent = 0;
            for (int x = width - 1; x >= 0; --x) {
                float bppRaw = (1 + numDifferent * channels) / (float)numDifferent;      /* (a division by zero gives +inf: IEEE 754) */
                float bppRLE = (1 + channels) / (float)numSame;
                if (bppRaw <= bppRLE) opcode[x] = (int8_t)numDifferent;
                else opcode[x] = (int8_t)(0x80 | numSame);
                if (similarMask[x]) {
                    numSame += 1;
                    if (numSame >= 127) numSame = 127;
                    numDifferent = 0;
                } else {
                    numDifferent += 1;
                    if (numDifferent >= 127) numDifferent = 127;
                    numSame = 0;
                }
            }
            int x = 0;                                                       /* 3. :251-269 */
            for (; x < width; ) {
                int8_t hint = opcode[x];
                WRITE(&hint, 1);
                int num = (hint & 127) + 1;
                size_t nbytes = (hint >= 0) ? (size_t)num * channels : (size_t)channels;
                if (x + ((hint >= 0) ? num : 1) > width) { free(scanSpace); return -3; }   /* (the reference would read behind scanSpace) */
                WRITE(&scanSpace[(size_t)x * channels], nbytes);
                x += num;
            }
            if (x != width) { free(scanSpace); return -3; }                  /* assert(x == _width) :269 */
        } else {
            WRITE(scanSpace, (size_t)width * channels);
        }
    }
    free(scanSpace);
    return pos;
}
