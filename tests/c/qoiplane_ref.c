/* qoiplane_ref.c -- the 8-bit grey slice of the reference's QOIX loader restated serially, for the tests: what qoix_lz4_decode
 * (source/gamut/plugins/qoix.d:350-473) does with an 8-bit file of 1 or 2 channels, that is the container checks and the LZ4 block as
 * in qoix_ref.c (included below for them) and qoiplane_decode (source/gamut/codecs/qoiplane.d:377-541) with the reference's scanline
 * structure: one pass over posy / posx, `run` counted down, the top pixel read from channel 0 of the OUTPUT line above.
 *
 * This is the library's behaviour with gamut_hip_qoix_set_plane(1).  Deviation P1 of gamut_amd/csrc/qoix.hip is part of this reading:
 * a nibble read at byte index >= size refuses the file (the reference has no input bound).  The closing four bytes ARE decoded.
 *
 * planeref_load(data, len, channels, out, out_cap, info) -> as qoixref_load: header verdict (0 ok, 1 refused, 2 codec not built) |
 * detected << 4 | decoded << 5; a colour file is handed to qoixref_load.  channels: 0, 1 or 2 for a grey file. */
#include "qoix_ref.c"

/* qoiplane.d:379-411 on the bytes the sub-codec is handed */
static int plane_header_ok(bytes_t hdr, long size, int compression_seen)
{
    uint32_t w = rd32(hdr + 4), h = rd32(hdr + 8);
    if (size < 25 + 4) return 0;
    if (w == 0 || h == 0) return 0;
    if (hdr[13] < 1 || hdr[13] > 2) return 0;
    if (hdr[15] > 1) return 0;
    if (hdr[14] != 8) return 0;
    if (hdr[12] > 1) return 0;
    if (compression_seen != 0) return 0;
    if (rd32(hdr) != 0x716F6978u) return 0;
    if (h >= 400000000u / w) return 0;
    return 1;
}

static int plane_header(bytes_t d, long len, int32_t* info, long* sub)
{
    int rc = header(d, len, info, sub);
    if (rc == 2 && d[14] == 8) return plane_header_ok(d, *sub, 0) ? 0 : 1;    /* qoix.d:445-454 */
    return rc;
}

typedef struct { bytes_t bytes; long size, p; int hi, ok; } nibbles_t;

static int read_nibble(nibbles_t* s)                                          /* qoiplane.d:430-440 */
{
    int r;
    if (s->p >= s->size) { s->ok = 0; return 0; }                             /* DEVIATION P1 */
    if (s->hi) r = s->bytes[s->p] >> 4;
    else r = s->bytes[s->p++] & 15;
    s->hi = !s->hi;
    return r;
}

static int read_ubyte(nibbles_t* s) { int hi = read_nibble(s) << 4; return hi | read_nibble(s); }    /* :442-447 */

/* qoiplane.d:413-540 */
static int plane_decode(bytes_t bytes, long size, int channels, uint8_t* out)
{
    uint32_t width = rd32(bytes + 4), height = rd32(bytes + 8), posx, posy;
    long pitch = (long)width * channels, num_pixels = (long)width * height, decoded_pixels = 0;
    uint8_t px_l = 0, px_a = 255, ref_l, ref_a;
    long run = 0;
    nibbles_t s;
    s.bytes = bytes; s.size = size; s.p = 25; s.hi = 1; s.ok = 1;
    for (posy = 0; posy < height; ++posy) {
        uint8_t* line = out + pitch * posy;
        const uint8_t* above = posy > 0 ? out + pitch * (posy - 1) : NULL;
        for (posx = 0; posx < width; ++posx) {
            ref_l = px_l; ref_a = px_a;
            if (run > 0) run--;
            else if (decoded_pixels < num_pixels) {
                for (;;) {
                    int op = read_nibble(&s);
                    if (!s.ok) return 0;
                    if (op == 15) {                                           /* REPEAT2 */
                        run = read_ubyte(&s) + 3;
                        if (run == 258) run = 0x7fffffff;
                    } else if ((op & 12) == 12) run = op & 3;                 /* REPEAT1 */
                    else {
                        int top = posy > 0 ? above[(size_t)posx * channels] : ref_l, avg = (top + ref_l + 1) / 2;
                        if ((op & 8) == 0) px_l = (uint8_t)(avg + op - 4);    /* DIFF1 */
                        else if ((op & 14) == 8) px_l = (uint8_t)(avg + (((op & 1) << 4) + read_nibble(&s)) - 16);      /* DIFF2 */
                        else if (op == 10) px_l = (uint8_t)read_ubyte(&s);    /* DIRECT */
                        else {
                            int diff = read_nibble(&s);
                            if (diff == 0) { px_l = (uint8_t)read_ubyte(&s); px_a = (uint8_t)read_ubyte(&s); }          /* LA */
                            else {                                            /* ADIFF, then the next op */
                                if (!s.ok) return 0;
                                px_a = (uint8_t)(ref_a + diff - 8);
                                continue;
                            }
                        }
                    }
                    break;
                }
                if (!s.ok) return 0;
                decoded_pixels++;
            }
            line[(size_t)posx * channels] = px_l;
            if (channels == 2) line[(size_t)posx * 2 + 1] = px_a;
        }
    }
    return 1;
}

long planeref_load(const uint8_t* data, long len, int channels, uint8_t* out, long out_cap, int32_t* info)
{
    long sub = 0, res;
    int rc = plane_header(data, len, info, &sub), ok;
    if (rc == 0 && info[3] >= 3) return qoixref_load(data, len, channels, out, out_cap, info);
    res = rc | (long)info[11] << 4;
    if (rc != 0 || !out) return res;
    if (channels < 0 || channels > 2) return res;
    if (channels == 0) channels = info[3];
    if ((long)(uint32_t)info[0] * (uint32_t)info[1] * channels > out_cap) return res;
    if (info[6] == 1) {
        uint8_t* dec = (uint8_t*)malloc((size_t)sub + 1);                     /* qoix.d:394-397 */
        if (!dec) return res;
        memcpy(dec, data, 25);
        dec[16] = 0;
        ok = lz4_fast(data, 29, len, dec + 25, sub - 25) && plane_header_ok(dec, sub, dec[16]) && plane_decode(dec, sub, channels, out);
        free(dec);
    } else ok = plane_decode(data, sub, channels, out);
    return res | (long)(ok != 0) << 5;
}
