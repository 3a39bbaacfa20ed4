/* gif_ref.c -- GIFDecoder (source/gamut/codecs/gif.d) and loadGIF (source/gamut/plugins/gif.d:57-103) restated serially, for the tests:
 * the same two passes over the file (the counting pass of parseHeader, then one decodeNextFrame per layer), the same state carried from
 * one into the other, the same prefix-chain LZW table and the same pixel stepping.  The memory stream is io.d's: a read fails when the
 * bytes are not all there, a skip fails only when it would end PAST the end of the file.
 *
 * Deliberate deviations, the same as gamut_amd/csrc/gif_host.hip (in each the reference touches memory it does not own):
 *   - both palette buffers are calloc'd (the reference's are uninitialised malloc memory);
 *   - a frame with neither a local nor a global colour table is refused (the reference dereferences null);
 *   - a frame with frameX + max(frameW, 1) > logicalScreenWidth is refused (the reference wraps into the next row and writes past its block);
 *   - a screen of more than 2^29 - 1 pixels is refused (the reference's int byte counts overflow).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { short prefix; uint8_t first, suffix; } LZWCode;

typedef struct {
    const uint8_t* data; long len, pos;
    int isGIF89, W, H, layers; float fps; uint8_t aspectByte;
    uint8_t *gctBuf, *gct, *lct, *pal; int gctSize, lctSize;
    int frameX, frameY, frameW, frameH, curX, curY, pass, interlaced;
    int transparent;
    uint8_t *background, *history, *out; int firstFrame;
    int disposal, transFlag, delay, transIndex;                       /* GCE */
    LZWCode* codes;
} Dec;

static int rd(Dec* d, void* dst, long n) { if (d->len - d->pos < n) return 0; memcpy(dst, d->data + d->pos, (size_t)n); d->pos += n; return 1; }
static int rd8(Dec* d, int* err) { uint8_t v; if (!rd(d, &v, 1)) { *err = 1; return 0; } *err = 0; return v; }
static int rd16(Dec* d, int* err)
{
    uint8_t v[2];
    if (d->len - d->pos < 2) { d->pos = d->len; *err = 1; return 0; }
    rd(d, v, 2); *err = 0; return v[0] | v[1] << 8;
}
static int skip(Dec* d, long n) { if (d->pos + n > d->len) return 0; d->pos += n; return 1; }
static int durationMs(const Dec* d) { return d->delay == 0 || d->delay == 1 ? 100 : d->delay * 10; }

static void colortable(Dec* d, uint8_t* p, int n, int transp, int* err)
{
    *err = 0;
    for (int i = 0; i < n; ++i) {
        if (!rd(d, p + 4 * i, 3)) { *err = 1; return; }
        p[4 * i + 3] = transp == i ? 0 : 255;
    }
}

static void skipSubblocks(Dec* d, int* err)
{
    int size;
    do {
        size = rd8(d, err); if (*err) return;
        if (!skip(d, size)) { *err = 1; return; }
    } while (size);
    *err = 0;
}

static void graphicsControl(Dec* d, int* err)
{
    int size = rd8(d, err); if (*err) return;
    if (size != 4) { *err = 1; return; }
    int rdit = rd8(d, err); if (*err) return;
    d->disposal = (rdit >> 2) & 3;
    d->transFlag = rdit & 1;
    d->delay = rd16(d, err); if (*err) return;
    d->transIndex = rd8(d, err); if (*err) return;
    if (d->transparent >= 0 && d->gct) d->gct[4 * d->transparent + 3] = 255;
    if (d->transFlag) {
        d->transparent = d->transIndex;
        if (d->transparent >= 0 && d->gct) d->gct[4 * d->transparent + 3] = 0;
    } else d->transparent = -1;
    int zero = rd8(d, err); if (*err) return;
    if (zero != 0) { *err = 1; return; }
    *err = 0;
}

static const int kStep[4] = { 8, 8, 4, 2 }, kStart[4] = { 0, 4, 2, 1 };

static void outCode(Dec* d, int code)
{
    if (d->codes[code].prefix >= 0) outCode(d, d->codes[code].prefix);
    if (d->curY >= d->H) return;
    long pIndex = (long)d->curY * d->W + d->curX;
    d->history[pIndex] = 1;
    const uint8_t* c = d->pal + d->codes[code].suffix * 4;
    if (c[3] > 128) { uint8_t* p = d->out + pIndex * 4; p[0] = c[0]; p[1] = c[1]; p[2] = c[2]; p[3] = 255; }
    d->curX += 1;
    if (d->curX >= d->frameX + d->frameW) {
        d->curX = d->frameX;
        if (d->interlaced) {
            d->curY += kStep[d->pass];
            if (d->curY >= d->frameY + d->frameH && d->pass < 3) { d->pass += 1; d->curY = d->frameY + kStart[d->pass]; }
        } else d->curY += 1;
    }
}

static void imageData(Dec* d, int* err, int needDecode)
{
    *err = 0;
    int lzw_cs = rd8(d, err); if (*err) return;
    if (lzw_cs > 12) { *err = 1; return; }
    int clear = 1 << lzw_cs, first = 1, codesize = lzw_cs + 1, codemask = (1 << codesize) - 1, bits = 0, valid_bits = 0;
    for (int i = 0; i < clear; ++i) { d->codes[i].prefix = -1; d->codes[i].first = (uint8_t)i; d->codes[i].suffix = (uint8_t)i; }
    int avail = clear + 2, oldcode = -1, len = 0;
    for (;;) {
        if (valid_bits < codesize) {
            if (len == 0) {
                len = rd8(d, err); if (*err) return;
                if (len == 0) return;
            }
            --len;
            int nb = rd8(d, err); if (*err) return;
            bits |= nb << valid_bits;
            valid_bits += 8;
        } else {
            int code = bits & codemask;
            bits >>= codesize;
            valid_bits -= codesize;
            if (code == clear) {
                codesize = lzw_cs + 1; codemask = (1 << codesize) - 1; avail = clear + 2; oldcode = -1; first = 0;
            } else if (code == clear + 1) {
                if (!skip(d, len)) { *err = 1; return; }
                len = rd8(d, err); if (*err) return;
                while (len > 0) {
                    if (!skip(d, len)) { *err = 1; return; }
                    len = rd8(d, err); if (*err) return;
                }
                return;
            } else if (code <= avail) {
                if (first) { *err = 1; return; }
                if (oldcode >= 0) {
                    LZWCode* p = &d->codes[avail++];
                    if (avail > 8192) { *err = 1; return; }
                    p->prefix = (short)oldcode;
                    p->first = d->codes[oldcode].first;
                    p->suffix = code == avail ? p->first : d->codes[code].first;
                } else if (code == avail) { *err = 1; return; }
                if (needDecode) outCode(d, code);
                if ((avail & codemask) == 0 && avail <= 0x0FFF) { codesize++; codemask = (1 << codesize) - 1; }
                oldcode = code;
            } else { *err = 1; return; }
        }
    }
}

static void lzwImage(Dec* d, int* err, int needDecode)
{
    d->frameX = rd16(d, err); if (*err) return;
    d->frameY = rd16(d, err); if (*err) return;
    d->frameW = rd16(d, err); if (*err) return;
    d->frameH = rd16(d, err); if (*err) return;
    int flags = rd8(d, err); if (*err) return;
    d->interlaced = (flags & 0x40) != 0;
    if (flags & 0x80) {
        d->lctSize = 1 << ((flags & 7) + 1);
        int transp = d->transFlag ? d->transparent : -1;
        if (needDecode) { colortable(d, d->lct, d->lctSize, transp, err); if (*err) return; }
        else if (!skip(d, d->lctSize * 3)) { *err = 1; return; }
        d->pal = d->lct;
    } else d->pal = d->gct;
    if (!d->pal) { *err = 1; return; }                                                     /* DEVIATION */
    if (d->frameX + (d->frameW > 1 ? d->frameW : 1) > d->W) { *err = 1; return; }           /* DEVIATION */
    d->pass = 0; d->curX = d->frameX; d->curY = d->frameY;
    imageData(d, err, needDecode);
}

/* 0: end of stream, 1: one frame, -1: error */
static int parseFrame(Dec* d, int* err, int needDecode)
{
    long pcount = (long)d->W * d->H;
    if (d->firstFrame) {
        if (d->out) { memset(d->out, 0, 4 * (size_t)pcount); memset(d->background, 0, 4 * (size_t)pcount); memset(d->history, 0, (size_t)pcount); }
        d->firstFrame = 0;
    } else if (needDecode) {
        int dispose = d->disposal;
        if (dispose == 3) dispose = 2;
        if (dispose == 2)
            for (long pi = 0; pi < pcount; ++pi) if (d->history[pi]) memcpy(d->out + pi * 4, d->background + pi * 4, 4);
        memcpy(d->background, d->out, 4 * (size_t)pcount);
    }
    for (;;) {
        int sep = rd8(d, err); if (*err) return -1;
        if (sep == 0x2C) { lzwImage(d, err, needDecode); if (*err) return -1; return 1; }
        else if (sep == 0x3B) return 0;
        else if (sep == 0x21) {
            int label = rd8(d, err); if (*err) return -1;
            switch (label) {
            case 0x01: if (!skip(d, 13)) { *err = 1; return -1; } skipSubblocks(d, err); if (*err) return -1; break;
            case 0xF9: graphicsControl(d, err); if (*err) return -1; break;
            case 0xFE: skipSubblocks(d, err); if (*err) return -1; break;
            case 0xFF: { int bs = rd8(d, err); if (*err) return -1; if (!skip(d, bs)) { *err = 1; return -1; } skipSubblocks(d, err); if (*err) return -1; break; }
            default: *err = 1; return -1;
            }
        } else { *err = 1; return -1; }
    }
}

static void freeDec(Dec* d) { free(d->gctBuf); free(d->lct); free(d->out); free(d->background); free(d->history); free(d->codes); }

/* info: width, height, layers, is_gif89; finfo: pixel aspect ratio, fps.  out == NULL: GIFDecoder.open alone.  Otherwise out receives
 * layers * w * h * 4 bytes (out_cap must hold them).  Returns 1 when the reference (with the deviations above) accepts the file. */
int gifref_load(const uint8_t* data, long len, uint8_t* out, long out_cap, int32_t* info, float* finfo)
{
    Dec d; memset(&d, 0, sizeof d);
    d.data = data; d.len = len;
    int err = 0;
    uint8_t magic[6];
    if (!rd(&d, magic, 6)) return 0;
    if (!memcmp(magic, "GIF87a", 6)) d.isGIF89 = 0; else if (!memcmp(magic, "GIF89a", 6)) d.isGIF89 = 1; else return 0;
    d.W = rd16(&d, &err); if (err) return 0;
    d.H = rd16(&d, &err); if (err) return 0;
    int flags = rd8(&d, &err); if (err) return 0;
    rd8(&d, &err); if (err) return 0;
    d.aspectByte = (uint8_t)rd8(&d, &err); if (err) return 0;
    d.transparent = -1;
    long pcount = (long)d.W * d.H;
    if (pcount > 0x1FFFFFFFL) return 0;                                                     /* DEVIATION */
    d.gctBuf = calloc(1024, 1); d.lct = calloc(1024, 1); d.codes = malloc(8192 * sizeof(LZWCode));
    if (out) { d.out = malloc(4 * (size_t)pcount + 1); d.background = malloc(4 * (size_t)pcount + 1); d.history = malloc((size_t)pcount + 1); }
    if (flags & 0x80) {
        d.gct = d.gctBuf; d.gctSize = 1 << ((flags & 7) + 1);
        colortable(&d, d.gct, d.gctSize, -1, &err); if (err) { freeDec(&d); return 0; }
    } else { d.gct = NULL; d.gctSize = 0; }
    d.pal = d.gct;
    long offset = d.pos;
    d.layers = 0;
    double sum = 0.0;
    d.firstFrame = 1;
    for (;;) {
        int res = parseFrame(&d, &err, 0);
        if (err) { freeDec(&d); return 0; }
        if (res == 0) break;
        d.layers++;
        sum += durationMs(&d);
    }
    d.fps = sum == 0 ? 10.0f : (float)(d.layers * 1000.0f / sum);
    d.pos = offset;
    d.firstFrame = 1;
    info[0] = d.W; info[1] = d.H; info[2] = d.layers; info[3] = d.isGIF89;
    finfo[0] = d.aspectByte == 0 ? -1.0f : (d.aspectByte + 15.0f) / 64;
    finfo[1] = d.fps;
    if (!out) { freeDec(&d); return 1; }
    if ((long)d.layers * pcount * 4 > out_cap) { freeDec(&d); return 0; }
    for (int l = 0; l < d.layers; ++l) {
        int res = parseFrame(&d, &err, 1);
        if (err || res != 1) { freeDec(&d); return 0; }
        memcpy(out + (size_t)l * (size_t)pcount * 4, d.out, (size_t)pcount * 4);
    }
    freeDec(&d);
    return 1;
}
